"""Shared pieces of the native grouped-query attention tests (tests/test_gpu_gqa.py): the HF twin with a WRONG KV head per query head (the reference the
teeth test measures against), the batches every check runs on, and the one small batch per untouched family whose outputs are pinned bit for bit to those of
the library as it was before native GQA (tests/golden/gqa_parent_families.npz).

The recorded file.  It was made once, on an MI355X, with the library of the commit before native GQA (0f5aa26) built by
`make -C kirag_amd/csrc BUILD=build_ab OUT=<path>` and loaded in a process of its own:
    KIRAG_AMD_LIB=<path> python tests/gqa_util.py tests/golden/gqa_parent_families.npz
It holds the bit patterns (uint32) of every family's embeddings and last hidden state.  A clean checkout cannot build its own parent, which is why the comparison
is against a recording and not against a second library.  What the pin means afterwards: "this commit did not change these families' bits".  A later change that
alters their rounding ON PURPOSE re-records the file the same way from ITS parent commit's library (or, where that change is itself the intended difference, from
its own library after its own parity tests pass) and says so in its message; a failure of the pin is then a question to answer, not a defect in GQA."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gqa_parent_families.npz")
# one shape more than tests/decoder_util.py has: 6 x 64 over 2 KV heads WITHOUT biases, so that the QKV projection is EPI_QKV_ROT, which (unlike Qwen2's
# EPI_QKV_ROTB) also runs on the 256 x 256 main loop: F = H + 2A = 640 is no multiple of 256, the loop's last tile column is partial and straddles v | nothing
D.SHAPES.setdefault("llama-384", ("llama", 384, 6, 2))
KINDS = ("qwen2-32", "llama-64", "qwen2-384", "llama-32", "llama-384")
# widths: 12 / 40 / 64 take the register-staged kernel with 4 / 2 / 2 heads per block, 150 / 300 the DMA ring (and k_attn_lds under KIRAG_AMD_ATTN_LDS=1)
SHORT, LONG = (12, 40, 64), (150, 300)
WRONG = ("mod", "neighbour")


def kv_map(heads, kv, how="right"):
    """the KV head query head h reads: h // group (HF's repeat_kv), or one of the two wrong ones — h % kv_heads, the neighbouring group"""
    g = heads // kv
    return [h // g if how == "right" else h % kv if how == "mod" else (h // g + 1) % kv for h in range(heads)]


def mapped_weights(cfg, w, how, which="kv"):
    """the checkpoint on `heads` KV heads, query head h carrying the k / v rows (and biases) of KV head kv_map(how)[h]; `which`: the projections that take the
    mapping `how` ('k', 'v' or 'kv'), the others take the right one.  how = 'right' is expand_kv."""
    heads, kv = cfg.num_attention_heads, cfg.num_key_value_heads
    d = cfg.hidden_size // heads
    out = {}
    for name, t in w.items():
        p = next((x for x in "kv" if f"self_attn.{x}_proj." in name), None)
        if p is None:
            out[name] = t
            continue
        m = kv_map(heads, kv, how if p in which else "right")
        out[name] = np.ascontiguousarray(t.reshape(kv, d, *t.shape[1:])[m].reshape(heads * d, *t.shape[1:]))
    return out


def batches(seed=0):
    """(ids, mask, tag): right / left padding, holes, a ragged batch with 1-token and full rows, one long sequence next to short ones"""
    out = []
    for S in SHORT:
        out.append(D.tokens(3, S, "R", seed + S) + (("R", S),))
        out.append(D.tokens(3, S, "L", seed + S + 1, holes=2 if S > 12 else 1) + (("L+holes", S),))
    out.append(D.tokens(5, 64, "R", seed + 7, lens=[5, 7, 33, 1, 64]) + (("ragged", 64),))
    for S in LONG:
        out.append(D.tokens(2, S, "R", seed + S, lens=[S, S // 2 + 3], holes=3) + (("R+holes", S),))
        out.append(D.tokens(2, S, "L", seed + S + 1) + (("L", S),))
    return out


# ---------------------------------------------------------------------------------------------------------
# the families native GQA does not touch
# ---------------------------------------------------------------------------------------------------------
def family_handles():
    """name -> (HipBertForward, ids, mask, pool): BERT at both head widths, MPNet, NomicBert (the rotating QKV epilogue with A = H), ModernBert (global and
    local layers), DeBERTa — one small ragged batch each, wide enough for two q-tiles"""
    from kirag_amd.retriever.encoders import HipBertForward
    from oracle import encoder_np as E
    import deberta_util as DB
    import modernbert_util as MB
    import mpnet_util as MP
    import nomic_util as N

    def hip(cfg, w):
        h = HipBertForward(cfg, 0)
        h.load_state(w)
        return h
    out = {}
    ids, mask = E.synth_tokens(5, 40, seed=21, ragged=True, vocab_lo=5, vocab_hi=300, min_len=3)
    for heads in (2, 4):
        cfg = SimpleNamespace(hidden_size=128, num_hidden_layers=2, num_attention_heads=heads, intermediate_size=256, vocab_size=300, max_position_embeddings=512,
                              type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")
        out["bert-%d" % (128 // heads)] = (hip(cfg, E.synth_weights(128, 2, 256, 300, 512, seed=5)), ids, mask, 0)
    out["mpnet"] = (hip(MP.cfg(128, 2, 2, 256, 300), MP.weights(128, 2, 2, 256, 300)), ids, mask, 0)
    out["nomic-64"] = (hip(N.cfg(128, 2, 2, 256, 300), N.weights(128, 2, 2, 256, 300)), ids, mask, 0)
    out["nomic-32"] = (hip(N.cfg(128, 2, 4, 256, 300), N.weights(128, 2, 4, 256, 300)), ids, mask, 0)
    out["modernbert"] = (hip(MB.cfg(128, 3, 2, 256, 300, local_attention=16), MB.weights(128, 3, 256, 300)), ids, mask, 0)
    c = DB.cfg()
    dids, dmask = DB.tokens(4, 40, seed=3)
    out["deberta"] = (hip(c, DB.weights(c)), np.asarray(dids), np.asarray(dmask), 0)
    return out


def family_outputs():
    """name -> uint32 bit patterns of [embeddings (pool 1, then pool 0) | last hidden state of the pool-0 forward] of the family's batch"""
    out = {}
    for name, (h, ids, mask, _) in family_handles().items():
        parts = []
        for pool in (1, 0):      # mean pooling last: its forward leaves every row of the last layer
            parts.append(np.ascontiguousarray(h.forward_np(ids, mask, pool), np.float32).ravel())
        parts.append(np.ascontiguousarray(h.last_hidden(*ids.shape).numpy(), np.float32).ravel())
        out[name] = np.concatenate(parts).view(np.uint32)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = family_outputs()
    np.savez_compressed(sys.argv[1], **res)
    print("recorded", {k: v.size for k, v in res.items()}, "with", os.environ.get("KIRAG_AMD_LIB", "the tree's library"))
