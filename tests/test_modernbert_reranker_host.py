"""Host-side tests of the ModernBERT cross-encoder rerankers: the dispatch of BGEReranker.from_pretrained to ModernBertReranker under both poolings, every
refusal by field name from config.json alone, the parameter-name map on the real HF task class (with and without the optional biases), the
save_pretrained -> from_pretrained round trip, the float64 head of the test helper against HF's logits (the formula the GPU tests compare the library
with), and the fences: RERANKER_MAP and the C header (the same 50 functions, ABI 9)."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modernbert_reranker_util as U  # noqa: E402
import modernbert_util as M  # noqa: E402

from kirag_amd import _lib  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever import rerankers as RR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, HEADS = 128, 2


def _tiny(labels=1, pooling="cls", biases=False, cls=None, **extra):
    return U.hf_classifier(U.cfg(H, HEADS, labels, pooling, biases, **extra), U.weights(H, labels, biases), cls=cls)


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_dispatch_and_round_trip(pooling, tmp_path):
    """a saved ModernBertForSequenceClassification folder loads as ModernBertReranker through the registry, parameters equal; save_model -> load_model
    round-trips; a CPU model in eval mode has no fallback and train mode is HF's own forward"""
    from transformers import ModernBertForSequenceClassification
    ref = _tiny(3, pooling, True)
    d = str(tmp_path / "ckpt")
    ref.save_pretrained(d)
    m = RR.load_reranker("BGEReranker", d)
    assert type(m) is RR.ModernBertReranker and isinstance(m, ModernBertForSequenceClassification) and m.config.classifier_pooling == pooling
    assert m._pool == ENC.POOL_CLASSIFY == 2 and float(m._hip_pooling) == U.POOLINGS[pooling]
    want = ref.state_dict()
    assert set(m.state_dict()) == set(want) and all(torch.equal(v, want[k]) for k, v in m.state_dict().items())       # the setting is no parameter and no buffer
    rr = RR.BaseReranker("BGEReranker", d)
    d2 = str(tmp_path / "again")
    rr.save_model(d2)
    rr.load_model(d2)
    assert type(rr.reranker) is RR.ModernBertReranker and all(torch.equal(v, want[k]) for k, v in rr.reranker.state_dict().items())
    ids, mask = U.pairs(3, 16, seed=1)
    args = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))
    with pytest.raises(RuntimeError, match="HIP path only"):
        m.eval()(**args)
    out = m.train()(**args, token_type_ids=torch.zeros_like(args["input_ids"])).logits          # token types, should a tokenizer emit them, are dropped
    assert out.requires_grad and out.shape == (3, 3) and np.abs(out.detach().double().numpy() - U.hf_logits(ref, ids, mask)).max() < 1e-5
    assert set(RR.RERANKER_MAP) == {"BGEReranker"} and RR.RERANKER_MAP["BGEReranker"] is RR.BGEReranker


REFUSALS = [({"classifier_activation": "silu"}, "classifier_activation"), ({"classifier_pooling": "max"}, "classifier_pooling"),
            ({"num_labels": 65}, "num_labels=65"), ({"hidden_size": 64, "num_attention_heads": 1}, "hidden_size=64"),
            ({"hidden_size": 2176, "num_attention_heads": 34}, "hidden_size=2176"), ({"num_attention_heads": 1}, "num_attention_heads=1"),
            ({"hidden_activation": "silu"}, "hidden_activation"), ({"layer_types": ["full_attention", "chunked_attention", "sliding_attention"]}, "layer_types"),
            ({"rope_parameters": {M.FULL: {"rope_type": "yarn", "rope_theta": 160000.0, "factor": 8.0, "original_max_position_embeddings": 512},
                                  M.SLIDING: {"rope_type": "default", "rope_theta": 10000.0}}}, "attention_scaling")]


@pytest.mark.parametrize("change,field", REFUSALS, ids=[f for _, f in REFUSALS])
def test_refused_by_field_name_from_config_json_alone(change, field, tmp_path, monkeypatch):
    """the folder holds config.json and nothing else (no weight can be read), and loading the library is an error: NotImplementedError beginning
    model_type='modernbert': and naming the field"""
    d = str(tmp_path / "cfg")
    os.makedirs(d)
    cfg = M.hf_config(U.cfg(H, HEADS)).to_dict()
    if "num_labels" in change:
        n = change["num_labels"]
        cfg["id2label"] = {str(i): f"LABEL_{i}" for i in range(n)}; cfg["label2id"] = {f"LABEL_{i}": i for i in range(n)}
    else:
        cfg.update(change)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(NotImplementedError, match=r"^model_type='modernbert': .*" + re.escape(field)):
        RR.load_reranker("BGEReranker", d)


def test_the_accepted_config_is_not_refused():
    RR.check_modern_config(M.hf_config(U.cfg(H, HEADS, 64, "mean", True)))
    RR.check_modern_config(M.hf_config(U.cfg(2048, 32)).to_dict())
    RR.check_modern_config(M.hf_config(U.cfg(128, 4)))


@pytest.mark.parametrize("biases", [False, True])
def test_rename_map_covers_hf_state_dict_exactly(biases):
    """every parameter of the HF class lands, exactly once, on a name the library knows: ModernBertModel's names without `model.`, and the head's own"""
    m = _tiny(3, "cls", biases, cls=RR.ModernBertReranker)
    names = [RR.modern_rename(n) for n, _ in m.named_parameters()]
    back = set(M.weights(H, U.LAYERS, U.FF, U.VOCAB))
    head = set(U.HEAD if biases else U.HEAD_REQUIRED)
    norm_biases = {n for n in names if n.endswith("norm.bias") and n not in head} if biases else set()
    assert norm_biases == ({"embeddings.norm.bias", "final_norm.bias"} | {f"layers.{l}.mlp_norm.bias" for l in range(U.LAYERS)}
                           | {f"layers.{l}.attn_norm.bias" for l in range(1, U.LAYERS)} if biases else set())
    assert set(names) == back | head | norm_biases and len(names) == len(set(names))
    assert set(names) == {RR.modern_rename(k) for k in m.state_dict()}                        # no buffer travels in the state dict
    shapes = {RR.modern_rename(n): tuple(p.shape) for n, p in m.named_parameters()}
    assert shapes[U.HEAD[0]] == (H, H) and shapes[U.HEAD[2]] == (H,) and shapes[U.HEAD[4]] == (3, H) and shapes[U.HEAD[5]] == (3,)
    assert (U.HEAD[1] in shapes) == (U.HEAD[3] in shapes) == biases
    assert RR.ModernBertReranker._hip_rename is RR.modern_rename
    assert [(n, float(t)) for n, t in RR.ModernBertReranker._hip_extra(m)] == [(U.POOLING_NAME, 0.0)]
    for name in ("_synced_hip", "_hip_forward", "invalidate_hip_weights", "train", "load_state_dict", "_apply"):
        assert getattr(RR.ModernBertReranker, name) is getattr(RR.XLMRobertaReranker, name), name


@pytest.mark.parametrize("pooling", ["cls", "mean"])
@pytest.mark.parametrize("biases", [False, True])
def test_float64_head_by_hand_reproduces_hf(pooling, biases):
    """pins the formula in the helper, not in the library: the float64 head on HF's last_hidden_state is HF's logits, and every mutation moves them"""
    m = _tiny(3, pooling, biases)
    for S, side in ((12, "right"), (150, "left")):
        ids, mask = U.pairs(5, S, side, seed=S)
        ref = U.hf_logits(m, ids, mask)
        assert np.abs(U.head_by_hand(m, ids, mask) - ref).max() < 1e-5
        lh = U.hf_last_hidden(m, ids, mask)
        w = {k: v for k, v in U.weights(H, 3, biases).items() if k in U.HEAD}
        assert np.abs(U.head64(U.pooled_rows(lh, mask, pooling), w, 1e-5) - ref).max() < 1e-5
        logit, bound = U.head_bound(U.pooled_rows(lh, mask, pooling), w, 1e-5)
        assert np.abs(logit - ref).max() < 1e-5 and (bound > 0).all() and bound.max() < 0.1
        for b in U.MUTATIONS:
            assert np.abs(U.head_by_hand(m, ids, mask, broken=b) - ref).max() > 0.1, b


def test_header_keeps_its_functions_and_documents_the_names():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert re.search(r"^#define KR_POOL_CLASSIFY 2\b", hdr, re.M) and re.search(r"^#define KR_ABI_VERSION 9\b", hdr, re.M)
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50 and _lib.ABI_VERSION == 9
    for name in U.HEAD + (U.POOLING_NAME,):
        assert '"%s"' % name in hdr, name
