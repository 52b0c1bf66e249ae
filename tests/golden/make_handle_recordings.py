"""What ``HipBertForward`` says to the library, per model family, recorded on the CPU: ``python tests/golden/make_handle_recordings.py`` writes
``tests/golden/handle_recordings.json``; ``tests/test_handle_recording_host.py`` imports ``CASES`` and ``record`` from here and compares.

``HipBertForward`` reaches the library through ``_lib.load()`` only.  ``RecordingLib`` stands in for the object that returns: it keeps every call in order —
``create`` with the eight ``kr_bert_cfg`` fields, the operand type and the low-half switch; ``load`` with the name, the element count and the sha256 of the
floats behind the pointer; ``finalize``; ``destroy`` — and needs no GPU.  Each case builds a tiny model from the per-family builders of ``tests/*_util.py``
(seeded numpy weights), makes the handle the way ``_HipModuleMixin._synced_hip`` does, and calls ``sync(module)`` twice (the second is the fast path: no call)
or ``load_state(arrays)`` once.  The recording is of the commit that introduced it and is not regenerated when the Python side is reorganised: that it still
matches is the point."""
import ctypes as C
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "handle_recordings.json")
ATTRIBUTES = ("hidden", "vocab", "ff", "ff_pad", "heads", "kv_heads", "out_dim", "num_labels", "colbert_dim", "position_padding_idx", "decoder_attention")


class RecordingLib:
    """the part of the C ABI that ``HipBertForward.__init__`` / ``sync`` / ``load_state`` call"""

    def __init__(self):
        self.calls = []

    def kr_encoder_create_ex(self, cfg, device_index, dt, lo, handle):
        c = cfg._obj
        self.calls.append(["create", [c.hidden, c.layers, c.heads, c.intermediate, c.vocab, c.max_pos, c.type_vocab, float(c.ln_eps)], int(dt), int(lo)])
        handle._obj.value = 1
        return 0

    def kr_encoder_load_weight(self, h, name, ptr, numel):
        data = bytes((C.c_float * int(numel)).from_address(int(ptr)))
        self.calls.append(["load", name.decode(), int(numel), hashlib.sha256(data).hexdigest()])
        return 0

    def kr_encoder_finalize(self, h):
        self.calls.append(["finalize"])
        return 0

    def kr_encoder_operand_dtype(self, h):
        return 1

    def kr_encoder_residual_lo(self, h):
        return 1

    def kr_encoder_destroy(self, h):
        self.calls.append(["destroy"])
        return 0


def handle_for(m, config=None):
    """the handle ``_HipModuleMixin._synced_hip`` would make for module ``m`` (device 0); ``config``: in the place of ``m.config``"""
    from kirag_amd.retriever.encoders import HipBertForward
    return HipBertForward(config or m.config, 0, rename=getattr(type(m), "_hip_rename", None), extra=getattr(type(m), "_hip_extra", None),
                          decoder_attention=getattr(m, "_decoder_attention", None))


def _loaded(m, state, allow_missing=()):
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=False)
    assert not res.unexpected_keys and all(any(a in k for a in allow_missing) for k in res.missing_keys), res
    return m.float().eval()


# ---- the cases: name -> callable returning ("sync", module[, config in the place of module.config]) or ("load_state", config, arrays[, HipBertForward kwargs]) ----
def _bert():
    import m3_util as M3
    from kirag_amd.retriever.encoders import E5Encoder
    return "sync", M3.hf_backbone("bert", M3.backbone("bert"), cls=E5Encoder)


def _xlmr_pad3():
    import xlmr_util as X
    return "sync", X.hf_model(X.cfg(128, 2, 2, 256, 200, 66, P=3), X.weights(128, 2, 256, 200, 66), "cpu")


def _mpnet():
    import mpnet_util as MP
    return "sync", MP.hf_model(MP.cfg(128, 2, 4, 256, 200, 66), MP.weights(128, 2, 4, 256, 200, 66), "cpu")


def _nomic():
    import nomic_util as N
    return "sync", N.hf_model(N.cfg(128, 2, 2, 256, 200), N.weights(128, 2, 2, 256, 200), "cpu")


def _modern(types=None, FF=320):
    """``types``: the handle's config names these layer types (HF's own config class refuses a list with one type only, so the module keeps the default list:
    its parameters are the same)"""
    import modernbert_util as M
    m = M.hf_model(M.cfg(128, 3, 4, FF, 100), M.weights(128, 3, FF, 100), "cpu")
    return ("sync", m) if types is None else ("sync", m, M.cfg(128, 3, 4, FF, 100, types=types))


def _t5_relu():
    import t5_util as T
    return "sync", T.hf_model(T.cfg(128, 2, 2, 256, 200), T.weights(128, 2, 2, 256, 200), "cpu")


def _t5_gated_dense():
    import t5_util as T
    from kirag_amd.retriever.encoders import T5E5Encoder
    c = T.cfg(128, 2, 4, 256, 200, ff="gated-gelu")
    w = T.weights(128, 2, 4, 256, 200, ff="gated-gelu")
    w["encoder.embed_tokens.weight"] = w["shared.weight"]
    m = _loaded(T5E5Encoder(T.hf_config(c)), w)
    m.set_dense(torch.from_numpy(T.dense_weight(256, 128)))
    return "sync", m


def _deberta():
    import deberta_util as DB
    c = DB.cfg(norm="layer_norm")
    return "sync", DB.hf_model(c, DB.weights(c))


def _decoder(kind, **extra):
    import decoder_util as D
    cfg = D.hf_config(kind, **extra)
    return "sync", D.hf_model(cfg, D.weights(cfg))


def _mistral():
    import decoder_util as D
    from transformers import MistralConfig, MistralModel
    cfg = MistralConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, intermediate_size=D.FF, vocab_size=D.VOCAB,
                        max_position_embeddings=D.MAX_POS, rms_norm_eps=1e-6, hidden_act="silu", rope_parameters={"rope_theta": 100.0, "rope_type": "default"},
                        attention_dropout=0.0, tie_word_embeddings=False, pad_token_id=0, sliding_window=None)
    return "sync", _loaded(MistralModel(cfg), D.weights(cfg))


def _eurobert():
    import eurobert_util as EU
    cfg = EU.hf_config("euro-64")
    return "sync", EU.hf_model(cfg, EU.weights(cfg))


def _qwen2_bidirectional():
    _, m = _decoder("qwen2-32")
    m._decoder_attention = 0.0          # what set_attention("bidirectional") leaves on a decoder twin
    return "sync", m


def _jina3():
    import jina3_util as J
    cfg = J.hf_config("jina-64")
    return "sync", J.hf_model(cfg, J.weights(cfg))


def _reranker(kind):
    import reranker_util as R
    from kirag_amd.retriever import rerankers as RR
    c = R.cfg(kind, 128, 2, 2, 256)
    return "sync", R.hf_classifier(kind, c, R.weights(kind, 128, 2, 256), cls=RR.XLMRobertaReranker if kind == "xlmr" else RR.BertReranker)


def _modern_reranker_mean():
    import modernbert_reranker_util as MR
    from kirag_amd.retriever.rerankers import ModernBertReranker
    return "sync", MR.hf_classifier(MR.cfg(128, 4, pooling="mean"), MR.weights(128), cls=ModernBertReranker)


def _deberta_reranker():
    import deberta_util as DB
    from kirag_amd.retriever.rerankers import DebertaV2Reranker
    c = DB.cfg(labels=1)
    w = {**DB.weights(c), **DB.head(c.hidden_size, 1)}
    return "sync", _loaded(DebertaV2Reranker(DB.hf_config(c)), {(DB._HF_HEAD[k] if k in DB.HEAD else "deberta." + k): v for k, v in w.items()})


def _splade_tied():
    import splade_util as SP
    from kirag_amd.retriever.splade import BertSpladeEncoder
    return "sync", SP.hf_mlm("h64", SP.VOCABS[0], SP.tied_weights(SP.VOCABS[0]), cls=BertSpladeEncoder, tie=True)


def _m3(kind):
    import m3_util as M3
    from kirag_amd.retriever import m3
    m = M3.hf_backbone(kind, M3.backbone(kind), cls=m3.XLMRobertaM3Encoder if kind == "xlmr" else m3.BertM3Encoder)
    hw = {k: torch.from_numpy(v) for k, v in M3.heads(M3.SHAPES[kind][0], 128).items()}
    m.set_heads({"weight": hw[M3.HEADS[0]], "bias": hw[M3.HEADS[1]]}, {"weight": hw[M3.HEADS[2]], "bias": hw[M3.HEADS[3]]})
    return "sync", m


def _state_bert():
    from oracle import encoder_np as E
    cfg = SimpleNamespace(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=300, max_position_embeddings=64,
                          type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")
    return "load_state", cfg, dict(E.synth_weights(128, 2, 512, 300, 64, seed=5))


def _state_modern():
    import modernbert_util as M
    return "load_state", M.cfg(128, 3, 4, 320, 100), M.weights(128, 3, 320, 100)


def _state_gqa():
    import decoder_util as D
    cfg = D.hf_config("qwen2-32")
    return "load_state", cfg, D.weights(cfg)


CASES = {
    "bert": _bert,
    "xlmr_pad_token_id_3": _xlmr_pad3,
    "mpnet": _mpnet,
    "nomic_bert": _nomic,
    "modernbert_ff320": _modern,
    "modernbert_all_global": lambda: _modern(types=["full_attention"] * 3, FF=256),
    "modernbert_all_sliding": lambda: _modern(types=["sliding_attention"] * 3, FF=256),
    "t5_relu": _t5_relu,
    "t5_gated_dense": _t5_gated_dense,
    "deberta_layer_norm": _deberta,
    "qwen2_4x32_kv2": lambda: _decoder("qwen2-32"),
    "llama_4x32_kv1": lambda: _decoder("llama-32", num_key_value_heads=1),
    "mistral": _mistral,
    "eurobert": _eurobert,
    "qwen2_bidirectional": _qwen2_bidirectional,
    "jina_v3": _jina3,
    "bert_reranker": lambda: _reranker("bert"),
    "xlmr_reranker": lambda: _reranker("xlmr"),
    "modernbert_reranker_mean": _modern_reranker_mean,
    "deberta_reranker": _deberta_reranker,
    "bert_splade_tied": _splade_tied,
    "m3_xlmr": lambda: _m3("xlmr"),
    "m3_bert": lambda: _m3("bert"),
    "load_state_bert": _state_bert,
    "load_state_modernbert": _state_modern,
    "load_state_gqa": _state_gqa,
}


def record(name: str) -> dict:
    """run case ``name`` against a ``RecordingLib``: the ordered calls, the handle's attributes afterwards, the calls of a second ``sync``"""
    from kirag_amd import _lib
    from kirag_amd.retriever.encoders import HipBertForward
    lib = RecordingLib()
    real, _lib.load = _lib.load, lambda: lib
    try:
        how, *what = CASES[name]()
        if how == "sync":
            hip = handle_for(*what)
            hip.sync(what[0])
            n = len(lib.calls)
            hip.sync(what[0])
            second = lib.calls[n:]
        else:
            hip = HipBertForward(what[0], 0)
            hip.load_state(what[1])
            n, second = len(lib.calls), None
        out = {"calls": lib.calls[:n], "attributes": {k: getattr(hip, k) for k in ATTRIBUTES},
               "flags": {k: v for k, v in sorted(vars(hip).items()) if k.startswith("is_")}, "second_sync": second}
        hip._h = None       # nothing to destroy
    finally:
        _lib.load = real
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump({name: record(name) for name in CASES}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
