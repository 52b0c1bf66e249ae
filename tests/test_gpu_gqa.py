"""GPU tests of native grouped-query attention on decoder handles: k_proj / v_proj reach the library as [A, H] (A = kv_heads d_h), K and V^T exist once per KV
head and both attention kernels read head h / group.

The yardstick is exact: a handle built from the HF tensors and one built from expand_kv's [H, H] tensors compute every q, k and v element as the same dot
product in the same MFMA order (the projection loops are independent of tiling and column position), and an attention block sees the same K / V^T bytes
either way — so last hidden state and embeddings are equal to the last bit, and any differing bit is an addressing defect.  Against HF (fp32, eager attention,
the unexpanded grouped config) the bars are those of tests/test_gpu_decoder.py for the same shapes.  The shapes are the tiny ones of tests/decoder_util.py:
4 x 32 over 2 KV heads with biases, 2 x 64 over 1 (multi-query), 6 x 64 over 2 (group 3: a 2-head block straddles two KV groups), 4 x 32 over 2 without biases,
and (tests/gqa_util.py) 6 x 64 over 2 without biases: EPI_QKV_ROT on the 256 x 256 main loop at F = 640, no multiple of 256."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402
import gqa_util as G  # noqa: E402
from test_gpu_decoder import COS_BAR, HIDDEN_BAR, SCORE_BAR  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL = -22
POOLS = (D.POOL_MEAN, D.POOL_LAST)
TILES = (256, 130, 128, 64, 32)


def _hip(cfg, w, attention=1.0):
    from kirag_amd.retriever.encoders import HipBertForward

    class H(HipBertForward):
        DECODER_ATTENTION = float(attention)
    h = H(cfg, 0)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


@pytest.fixture(scope="module")
def pairs():
    """(kind, attention) -> (config, weights, handle from the HF tensors, handle from expand_kv's), made once"""
    cache = {}

    def get(kind, attention=1.0):
        if (kind, attention) not in cache:
            cfg = D.hf_config(kind)
            w = D.weights(cfg)
            cache[(kind, attention)] = (cfg, w, _hip(cfg, w, attention), _hip(cfg, G.mapped_weights(cfg, w, "right"), attention))
        return cache[(kind, attention)]
    return get


@pytest.fixture(scope="module")
def references():
    """kind -> [(ids, mask, tag, HF last_hidden_state)] on the batches of gqa_util.batches(), computed once (CPU, fp32, eager attention, grouped config)"""
    cache = {}

    def get(kind):
        if kind not in cache:
            cfg = D.hf_config(kind)
            m = D.hf_model(cfg, D.weights(cfg))
            cache[kind] = [(ids, mask, tag, D.hf_last_hidden(m, ids, mask)) for ids, mask, tag in G.batches()]
        return cache[kind]
    return get


# ---------------------------------------------------------------------------------------------------------
# 1. the gate: fails without the feature
# ---------------------------------------------------------------------------------------------------------
def test_grouped_tensors_load_finalize_and_run_every_entry_point():
    """Before native GQA, layers.0.self_attn.k_proj.weight with A * H < H * H elements was KR_EINVAL.  Now it loads, the handle finalizes from the HF state
    dict as it is and runs kr_encoder_forward, _forward_tt and _forward_packed with pools 0 and 5 — to the same bits as the expanded handle."""
    from kirag_amd import _lib
    from kirag_amd.retriever.encoders import expand_kv
    lib = _lib.load()
    cfg = D.hf_config("qwen2-32")
    w = D.weights(cfg)
    H, heads, kv = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads
    A = kv * (H // heads)
    inv = D.hf_model(cfg, w).rotary_emb.inv_freq.numpy()
    ids, mask = D.tokens(3, 20, "R", 1)
    B, S = ids.shape
    tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32); tt = np.zeros_like(ids)
    results = []
    for expanded in (False, True):
        bc = _lib.BertCfg(H, cfg.num_hidden_layers, heads, cfg.intermediate_size, cfg.vocab_size, 512, 1, 1e-6)
        h = C.c_void_p()
        assert lib.kr_encoder_create_ex(C.byref(bc), 0, -1, -1, C.byref(h)) == 0
        try:
            def load(name, arr):
                a = np.ascontiguousarray(arr, np.float32)
                return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)
            assert load(D.INV_FREQ_NAME, inv) == 0 and load(D.SETTING, [1.0]) == 0, lib.kr_last_error()
            if not expanded:
                k0 = w["layers.0.self_attn.k_proj.weight"]
                assert k0.size == A * H < H * H
                assert load("layers.0.self_attn.k_proj.weight", k0) == 0, lib.kr_last_error()        # the gate
                assert load("layers.0.self_attn.k_proj.weight", np.zeros((A // 2, H))) == KR_EINVAL and b"A % 64 == 0" in lib.kr_last_error()
            for k, v in w.items():
                assert load(k, expand_kv(k, v, heads, kv) if expanded else v) == 0, (k, lib.kr_last_error())
            assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
            outs = {}
            for pool in POOLS:
                o = [np.full((B, H), 7.0, np.float32) for _ in range(3)]
                assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, o[0].ctypes.data, None) == 0, lib.kr_last_error()
                assert lib.kr_encoder_forward_tt(h, ids.ctypes.data, mask.ctypes.data, tt.ctypes.data, B, S, pool, o[1].ctypes.data, None) == 0, lib.kr_last_error()
                assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), pool, o[2].ctypes.data, None) == 0, lib.kr_last_error()
                assert np.isfinite(o[0]).all() and np.allclose(np.linalg.norm(o[0], axis=1), 1, atol=1e-5)
                assert _same(o[0], o[1]) and _same(o[0], o[2]), pool
                outs[pool] = o[0]
            if not expanded:       # fixed at the first finalize: the same A again is fine, [H, H] is not
                assert load("layers.1.self_attn.v_proj.weight", w["layers.1.self_attn.v_proj.weight"]) == 0
                assert load("layers.1.self_attn.v_proj.weight", expand_kv("layers.1.self_attn.v_proj.weight", w["layers.1.self_attn.v_proj.weight"], heads, kv)) == KR_EINVAL
                assert b"after kr_encoder_finalize" in lib.kr_last_error()
            results.append(outs)
        finally:
            lib.kr_encoder_destroy(h)
    for pool in POOLS:
        assert _same(results[0][pool], results[1][pool]), pool


# ---------------------------------------------------------------------------------------------------------
# 2. bit identity against the expanded handle
# ---------------------------------------------------------------------------------------------------------
def _both(hn, he, ids, mask, pool):
    on, oe = hn.forward_np(ids, mask, pool), he.forward_np(ids, mask, pool)
    ln, le = hn.last_hidden(*ids.shape).numpy(), he.last_hidden(*ids.shape).numpy()
    assert np.isfinite(on).all() and np.isfinite(ln).all()
    return _same(on, oe) and _same(ln, le)


@pytest.mark.parametrize("attention", [1.0, 0.0], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_native_and_expanded_handles_agree_to_the_last_bit(kind, attention, pairs, monkeypatch):
    """Bound 0, derived (see the module docstring).  Every batch of gqa_util.batches() — right / left padding, holes, ragged lengths, S in {12, 40, 64} on
    the register-staged kernel with 4 / 2 / 2 heads per block, S in {150, 300} on the DMA ring and, under KIRAG_AMD_ATTN_LDS=1, on k_attn_lds with one head
    per block — with pools 0 and 5; the ragged batch through kr_encoder_forward_packed; every KIRAG_AMD_PROJ_TILE on a short, a medium and a long batch."""
    cfg, w, hn, he = pairs(kind, attention)
    assert hn.kv_heads < hn.heads
    for ids, mask, tag in G.batches():
        for pool in POOLS:
            assert _both(hn, he, ids, mask, pool), (tag, pool)
            if tag[1] in G.LONG:
                monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
                assert _both(hn, he, ids, mask, pool), (tag, pool, "attn_lds")
                monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
        if tag in (("R", 12), ("ragged", 64), ("R+holes", 300)):
            for tile in TILES:
                monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
                assert _both(hn, he, ids, mask, D.POOL_MEAN), (tag, tile)
            monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
        if tag[0] == "ragged":
            import torch
            tok = torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))); lens = torch.from_numpy(mask.sum(1).astype(np.int32))
            for pool in POOLS:
                pn, pe = hn.forward_packed(tok, lens, ids.shape[1], pool).cpu().numpy(), he.forward_packed(tok, lens, ids.shape[1], pool).cpu().numpy()
                assert _same(pn, pe) and _same(pn, hn.forward_np(ids, mask, pool)), pool


# ---------------------------------------------------------------------------------------------------------
# 3. against HF, 4. with teeth
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
def test_parity_with_hf_on_the_grouped_config(kind, pairs, references):
    """last_hidden_state on attended rows within 3e-2 of Qwen2Model / LlamaModel (fp32, eager attention, num_key_value_heads as in the checkpoint), embeddings
    within 1 - cos 5e-5 and scores within 1e-3 for both pools: the bars of tests/test_gpu_decoder.py"""
    cfg, w, hn, _ = pairs(kind)
    worst = 0.0
    for ids, mask, tag, ref in references(kind):
        keep = mask.astype(bool)
        for pool in POOLS:
            out = hn.forward_np(ids, mask, pool)
            want = D.pool_np(ref, mask, pool)
            cos, ds = _cos_gap(out, want), float(np.abs(out @ out.T - want @ want.T).max())
            assert cos <= COS_BAR and ds <= SCORE_BAR, (tag, pool, cos, ds)
        lh = hn.last_hidden(*ids.shape).numpy()
        err = float(np.abs(lh - ref)[keep].max())
        worst = max(worst, err)
        assert np.isfinite(lh).all() and not lh[~keep].any() and err <= HIDDEN_BAR, (tag, err)
    print(f"[{kind}] native GQA last_hidden_state vs HF fp32 eager: worst {worst:.2e} (bar {HIDDEN_BAR})")


@pytest.mark.parametrize("kind", [k for k in G.KINDS if D.SHAPES[k][3] > 1])
def test_reading_the_wrong_kv_head_would_show(kind, pairs, references):
    """Precondition on the reference (the HF twin on the CPU), then the library against it: a model whose query heads read KV head h % kv_heads, or the
    neighbouring group's, for K, for V or for both, differs from the reference by more than 10 x the bar on some attended row of every batch — and the
    library's rows lie within the bar of the reference, so at least 9 x the bar away from each of them."""
    cfg, w, hn, _ = pairs(kind)
    big = D.expanded_config(cfg)
    refs = references(kind)
    picked = [r for r in refs if r[2] in (("L+holes", 12), ("R", 40), ("ragged", 64), ("R+holes", 150))]      # one batch per kernel path; 6 wrong models each
    assert len(picked) == 4
    weakest = np.inf
    wrong = {(how, which): D.hf_model(big, G.mapped_weights(cfg, w, how, which)) for how in G.WRONG for which in ("k", "v", "kv")}
    assert np.array_equal(D.hf_last_hidden(D.hf_model(big, G.mapped_weights(cfg, w, "right")), picked[0][0], picked[0][1]), picked[0][3])
    for ids, mask, tag, ref in picked:
        keep = mask.astype(bool)
        hn.forward_np(ids, mask, D.POOL_MEAN)
        lh = hn.last_hidden(*ids.shape).numpy()
        assert float(np.abs(lh - ref)[keep].max()) <= HIDDEN_BAR
        for key, m in wrong.items():
            other = D.hf_last_hidden(m, ids, mask)
            d = float(np.abs(other - ref)[keep].max())
            weakest = min(weakest, d)
            assert d > 10 * HIDDEN_BAR, ("precondition", tag, key, d)
            assert float(np.abs(lh - other)[keep].max()) > 9 * HIDDEN_BAR, (tag, key)
    print(f"[{kind}] weakest wrong-KV-head distance {weakest:.2f} (required > {10 * HIDDEN_BAR})")


# ---------------------------------------------------------------------------------------------------------
# 5. the other families
# ---------------------------------------------------------------------------------------------------------
def test_other_families_compute_what_they_did_before():
    """BERT (64- and 32-wide heads), MPNet, NomicBert, ModernBert and DeBERTa handles on one small batch each: embeddings and last hidden state equal, bit for
    bit, those recorded from the library as it was before native GQA.  The file was recorded once and its origin cannot be read off it: tests/gqa_util.py
    says how it was made, and how a later change that alters these families' rounding on purpose re-records it — a failure here after such a change is not
    a defect of grouped-query attention."""
    gold = np.load(G.GOLDEN, allow_pickle=False)
    got = G.family_outputs()
    assert sorted(got) == sorted(gold.files)
    for name, bits in got.items():
        assert bits.shape == gold[name].shape and np.array_equal(bits, gold[name]), name
