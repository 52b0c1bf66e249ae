"""GPU tests of DeBERTa-v2 / v3 checkpoints (microsoft/deberta-v3-* fine-tunes: DebertaV2Model = BERT's post-LN layer without a position table, every attention
score carrying q_i . PK[p] + k_j . PQ[p] with p the log bucket of the column difference).  Reference: transformers.DebertaV2Model in fp32 on the CPU (its
attention is eager only) on synthetic weights under which the position terms decide the output (deberta_util.weights: each part of the disentangled attention,
broken alone, moves some row by more than 10 x the bar — asserted below on the float64 restatement, after that restatement agrees with HF).  Bars: the
project's 3e-2 per element of last_hidden_state on attended rows, 1 - cos <= 5e-5 and every score within 1e-3 for both pools.  Tiny shapes: H 128 as 2 x 64
and 4 x 32 heads, 2 layers, FF 256, B <= 8; a reference is computed once per case."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deberta_util as D  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL, KR_ESTATE, KR_ERANGE = -22, -1, -34
POOL_MEAN, POOL_CLS, POOL_CLASSIFY = 0, 1, 2
HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
V3, SMALL = (256, 512), (32, 128)            # (position_buckets, max_relative_positions): every v3 checkpoint's; one whose log zone and clamp S = 150 reaches
# (Bk, M), S: at (256, 512) the log zone starts at |r| = 129 and S = 512 reaches bucket 255; at (32, 128) S = 40 reaches the log zone, S = 150 the clamp on both sides
CASES = [(V3, 12), (V3, 40), (V3, 150), (V3, 300), (V3, 512), (SMALL, 40), (SMALL, 150)]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cos_gap(out, ref):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return float((1.0 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


@functools.lru_cache(maxsize=None)
def _model(bm, heads):
    """(config, weights, HF model) of one (Bk, M) and head layout: built once, never changed"""
    c = D.cfg(heads=heads, Bk=bm[0], M=bm[1])
    w = D.weights(c)
    return c, w, D.hf_model(c, w)


@functools.lru_cache(maxsize=None)
def _hip(bm, heads, **env):
    from kirag_amd.retriever.encoders import HipBertForward
    c, w, _ = _model(bm, heads)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = HipBertForward(c, 0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    h.load_state(w)
    assert h.is_deberta
    return h


def _raw_handle(H=128, heads=2, FF=256, layers=1, max_pos=512):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(H, layers, heads, FF, D.VOCAB, max_pos, 1, D.EPS)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _load(lib, h, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)


def test_the_names_load_and_a_forward_runs():
    """the test that fails without the feature: encoder.rel_embeddings.weight was an unknown tensor name (and the two settings unknown settings)"""
    c = D.cfg(layers=1, Bk=32, M=128)
    w = D.weights(c)
    lib, h = _raw_handle()
    try:
        assert _load(lib, h, D.SETTINGS[0], [32.0]) == 0, lib.kr_last_error()
        assert _load(lib, h, D.SETTINGS[1], [128.0]) == 0, lib.kr_last_error()
        for k, v in w.items():
            assert _load(lib, h, k, v) == 0, (k, lib.kr_last_error())
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        ids, mask = D.tokens(3, 24, seed=1)
        out = np.full((3, 128), np.float32(-7.0))
        for pool in (POOL_MEAN, POOL_CLS):
            assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, 3, 24, pool, out.ctypes.data, None) == 0, lib.kr_last_error()
            assert np.allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5)
            assert _cos_gap(out, D.pooled(D.hf_hidden(D.hf_model(c, w), ids, mask), mask, pool)) <= COS_BAR
        # KR_POOL_CLASSIFY without the head: KR_ESTATE naming the tensors
        assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, 3, 24, POOL_CLASSIFY, out.ctypes.data, None) == KR_ESTATE
        assert b"classifier.out_proj" in lib.kr_last_error()
        # S beyond max_position_embeddings
        big = np.ones((1, 513), np.int64)
        assert lib.kr_encoder_forward(h, big.ctypes.data, big.ctypes.data, 1, 513, POOL_MEAN, out.ctypes.data, None) == KR_EINVAL
        # fixed at the first finalize
        assert _load(lib, h, D.SETTINGS[0], [32.0]) == 0 and _load(lib, h, D.SETTINGS[0], [64.0]) == KR_EINVAL
        assert _load(lib, h, D.REL_NAME, np.zeros((128, 128))) == KR_EINVAL
    finally:
        lib.kr_encoder_destroy(h)


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("bm,S", CASES, ids=[f"Bk{bm[0]}-S{S}" for bm, S in CASES])
def test_parity_with_hf_fp32(bm, S, heads):
    """kr_encoder_last_hidden element-wise on attended rows, and both pools, against HF fp32: right padding, left padding, holes in the mask.  Under CLS pooling
    a left-padded row whose column 0 is masked has no reference (HF attends uniformly over masked columns there): finite only."""
    c, w, m = _model(bm, heads)
    h = _hip(bm, heads, KIRAG_AMD_CLS_FULL="1")
    B = 3 if S >= 300 else 4
    worst = {}
    mean_out, mean_ref = [], []
    for layout in ("right", "left", "holes"):
        ids, mask = D.tokens(B, S, "left" if layout == "left" else "right", seed=heads, holes=layout == "holes")
        ref = D.hf_hidden(m, ids, mask)
        att = mask.astype(bool)
        for pool in (POOL_MEAN, POOL_CLS):
            out = h.forward_np(ids, mask, pool)
            assert out.shape == (B, 128) and np.isfinite(out).all()
            hid = h.last_hidden(B, S).numpy()
            err = float(np.abs(hid - ref)[att].max())
            assert pool == POOL_CLS or (hid[~att] == 0).all()          # (CLS pooling: a masked column 0 holds the query-only row)
            has0 = att[:, 0]
            cos = _cos_gap(out[has0], D.pooled(ref, mask, pool)[has0]) if pool == POOL_CLS else _cos_gap(out, D.pooled(ref, mask, pool))
            worst[(layout, pool)] = (err, cos)
            assert err <= HIDDEN_BAR, (layout, pool, err)
            assert cos <= COS_BAR, (layout, pool, cos)
            if pool == POOL_MEAN:
                mean_out.append(out); mean_ref.append(D.pooled(ref, mask, pool))
    a, r = np.concatenate(mean_out), np.concatenate(mean_ref)
    dscore = float(np.abs(a @ a.T - r @ r.T).max())
    print(f"[Bk {bm[0]} M {bm[1]} S {S} heads {heads}] worst |hidden - HF| {max(v[0] for v in worst.values()):.2e}, 1 - cos {max(v[1] for v in worst.values()):.2e}, |q.d - ref| {dscore:.2e}")
    assert dscore <= SCORE_BAR, dscore


@pytest.mark.parametrize("heads", [2, 4])
def test_ragged_batch_and_packed_entry_point(heads):
    """lengths 5 / 7 / 33 / 1 / 64 in one batch: element-wise against HF, and kr_encoder_forward_packed gives the padded entry point's bits"""
    c, w, m = _model(V3, heads)
    h = _hip(V3, heads)
    lens = np.array([5, 7, 33, 1, 64], np.int32)
    S = 64
    rng = np.random.Generator(np.random.PCG64(11))
    ids = np.zeros((5, S), np.int64); mask = np.zeros((5, S), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(3, D.VOCAB, n); ids[b, 0] = D.CLS_ID; mask[b, :n] = 1
    ref = D.hf_hidden(m, ids, mask)
    out = h.forward_np(ids, mask, POOL_MEAN)
    hid = h.last_hidden(5, S).numpy()
    att = mask.astype(bool)
    err = float(np.abs(hid - ref)[att].max())
    print(f"[ragged heads {heads}] worst |hidden - HF| {err:.2e}")
    assert err <= HIDDEN_BAR and _cos_gap(out, D.pooled(ref, mask, POOL_MEAN)) <= COS_BAR
    toks = torch.from_numpy(np.concatenate([ids[b, :lens[b]] for b in range(5)]).astype(np.int32))
    for pool in (POOL_MEAN, POOL_CLS):
        packed = h.forward_packed(toks, torch.from_numpy(lens), S, pool)
        assert _same(packed.cpu().numpy(), h.forward_np(ids, mask, pool)), pool
    h.check()


@pytest.mark.parametrize("bm,S,heads", [(V3, 150, 2), (SMALL, 150, 4), (V3, 300, 4)])
def test_a_sequences_rows_do_not_depend_on_its_batch(bm, S, heads, monkeypatch):
    """bit-identity of a sequence's rows: alone, in a batch, in the reversed batch, from kr_encoder_forward_packed, shifted by left padding (only column
    differences enter), under every KIRAG_AMD_PROJ_TILE and under KIRAG_AMD_ATTN_LDS=1 (a DeBERTa forward runs k_attn_lds at every length: the same launches)"""
    h = _hip(bm, heads)
    B = 4
    ids, mask = D.tokens(B, S, seed=7)
    lens = mask.sum(1)
    out = {p: h.forward_np(ids, mask, p) for p in (POOL_MEAN, POOL_CLS)}
    h.forward_np(ids, mask, POOL_MEAN)                         # (the CLS shortcut keeps no rows: read them behind a mean forward)
    hid = h.last_hidden(B, S).numpy()
    assert np.ptp(out[POOL_MEAN], axis=0).min() > 0
    for p in (POOL_MEAN, POOL_CLS):
        assert _same(h.forward_np(ids[::-1].copy(), mask[::-1].copy(), p)[::-1].copy(), out[p]), p
        for b in range(B):
            n = int(lens[b])
            assert _same(h.forward_np(ids[b:b + 1, :n].copy(), mask[b:b + 1, :n].copy(), p), out[p][b:b + 1]), (p, b)      # alone, at its own width
        toks = torch.from_numpy(np.concatenate([ids[b, :lens[b]] for b in range(B)]).astype(np.int32))
        assert _same(h.forward_packed(toks, torch.from_numpy(lens.astype(np.int32)), S, p).cpu().numpy(), out[p]), p
    # left padding: the same sequences shifted to the right end of a wider batch
    Sw = min(S + 37, 512)
    lids = np.zeros((B, Sw), np.int64); lmask = np.zeros((B, Sw), np.int64)
    for b in range(B):
        n = int(lens[b])
        lids[b, Sw - n:], lmask[b, Sw - n:] = ids[b, :n], 1
    assert _same(h.forward_np(lids, lmask, POOL_MEAN), out[POOL_MEAN])
    lhid = h.last_hidden(B, Sw).numpy()
    for b in range(B):
        n = int(lens[b])
        assert _same(np.ascontiguousarray(lhid[b, Sw - n:]), np.ascontiguousarray(hid[b, :n])), b
    for tile in ("32", "64", "128", "130", "256"):
        monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", tile)
        assert _same(h.forward_np(ids, mask, POOL_MEAN), out[POOL_MEAN]), tile
        assert _same(h.last_hidden(B, S).numpy(), hid), tile
    monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
    monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
    for p in (POOL_MEAN, POOL_CLS):
        assert _same(h.forward_np(ids, mask, p), out[p]), p


def test_a_nan_in_the_position_table_is_erange():
    from kirag_amd import _lib
    from kirag_amd.retriever.encoders import HipBertForward
    c = D.cfg(layers=1, Bk=32, M=128)
    w = dict(D.weights(c))
    h = HipBertForward(c, 0)
    h.load_state(w)
    ids, mask = D.tokens(2, 16, seed=2, full=True)
    good = h.forward_np(ids, mask, POOL_MEAN)
    assert np.isfinite(good).all()
    bad = w[D.REL_NAME].copy(); bad[32 + 3, 5] = np.nan            # bucket of r = +3: every sequence of more than 3 tokens reads it
    w[D.REL_NAME] = bad
    h.load_state(w)
    with pytest.raises(_lib.KiragAmdError) as ei:
        h.forward_np(ids, mask, POOL_MEAN)
    assert ei.value.code == KR_ERANGE
    w[D.REL_NAME] = D.weights(c)[D.REL_NAME]
    h.load_state(w)
    assert _same(h.forward_np(ids, mask, POOL_MEAN), good)


def test_table_without_its_norm_and_new_values():
    """norm_rel_ebd none (no encoder.LayerNorm): R is the raw table; a same-shape reload of the table takes new values (the weight sync)"""
    from kirag_amd.retriever.encoders import HipBertForward
    c = D.cfg(heads=4, Bk=32, M=128, norm="none")
    w = D.weights(c)
    assert D.REL_LN[0] not in w
    h = HipBertForward(c, 0)
    h.load_state(w)
    m = D.hf_model(c, w)
    ids, mask = D.tokens(3, 40, seed=5)
    out = h.forward_np(ids, mask, POOL_MEAN)
    ref = D.hf_hidden(m, ids, mask)
    err = float(np.abs(h.last_hidden(3, 40).numpy() - ref)[mask.astype(bool)].max())
    print(f"[raw table] worst |hidden - HF| {err:.2e}")
    assert err <= HIDDEN_BAR and _cos_gap(out, D.pooled(ref, mask, POOL_MEAN)) <= COS_BAR
    w2 = dict(w); w2[D.REL_NAME] = -w[D.REL_NAME]
    h.load_state(w2)
    assert not _same(h.forward_np(ids, mask, POOL_MEAN), out)
    h.load_state(w)
    assert _same(h.forward_np(ids, mask, POOL_MEAN), out)


@pytest.mark.parametrize("name,pool", [("E5Encoder", POOL_MEAN), ("BGEEncoder", POOL_CLS)])
def test_the_registry_classes_reach_the_twins(tmp_path, name, pool):
    """save_pretrained a tiny DebertaV2Model; E5Encoder / BGEEncoder.from_pretrained return the DeBERTa twin, whose eval forward is the library's and whose
    train() forward is HF's own"""
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import load_retriever
    c, w, m = _model(SMALL, 2)
    d = str(tmp_path / "m")
    m.save_pretrained(d)
    enc = getattr(ENC, name).from_pretrained(d)
    twin = {"E5Encoder": ENC.DebertaV2E5Encoder, "BGEEncoder": ENC.DebertaV2BGEEncoder}[name]
    assert type(enc) is twin and type(load_retriever({"E5Encoder": "E5Retriever", "BGEEncoder": "BGERetriever"}[name], d)) is twin
    enc = enc.cuda().eval()
    ids, mask = D.tokens(4, 40, seed=3)
    with torch.no_grad():
        out = enc(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda())
    ref = D.pooled(D.hf_hidden(m, ids, mask), mask, pool)
    assert out.is_cuda and out.shape == (4, 128) and _cos_gap(out.cpu().numpy(), ref) <= COS_BAR
    assert _same(out.cpu().numpy(), _hip(SMALL, 2).forward_np(ids, mask, pool))
    enc.train()
    tr = enc(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda())
    assert tr.requires_grad and _cos_gap(tr.detach().cpu().numpy(), ref) <= 1e-5
