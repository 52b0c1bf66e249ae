"""GPU tests of bge-m3's sparse and multi-vector heads (KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT): lifecycle and refusals through the C ABI, element-wise
parity of both token-level blocks against HF fp32 + the heads in fp64 (both families, right / left padding, masks with holes, S = 12 / 40 / 150, P = 128 /
256), the teeth of those bars, the exact invariants (dense block, independence of the flags, batch invariance, +0.0 in masked slots, guard words, handles
with and without the heads, projection tilings), BGEM3Model end to end, and non-finite head weights.  Synthetic weights (m3_util); no bge-m3 checkpoint
exists offline.

Bars (m3_util.BARS): twice the worst value measured over the parity cases of this file on one MI355X (profiles/m3/measurements.txt, section 1):
    colbert, per-token 1 - cos     worst 1.0604e-07   bar 2.2e-07
    colbert, |element difference|  worst 1.8116e-04   bar 3.7e-04
    sparse, |weight difference|    worst 9.9722e-06   bar 2.0e-05
Scores (dense, sparse, MaxSim, combined): the project's 1e-3 score tolerance (m3_util.SCORE_BAR)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3_util as M  # noqa: E402
import xlmr_util as X  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL, KR_ESTATE, KR_ERANGE = -22, -1, -34
POOL_MEAN, POOL_CLS, SPARSE, COLBERT = 0, 1, 0x10, 0x20
H = 128
POISON = np.float32(-7.0)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _hf(kind):
    return M.hf_backbone(kind, M.backbone(kind), "cuda")


@functools.lru_cache(maxsize=None)
def _hip(kind, P, heads=True):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(M.cfg(kind, *M.SHAPES[kind]), 0)
    h.load_state({**M.backbone(kind), **(M.heads_for(kind, P) if heads else {})})
    return h


def _sizes(pool, B, S, P):
    return B * H, (B * S if pool & SPARSE else 0), (B * S * P if pool & COLBERT else 0)


def _split(flat, pool, B, S, P):
    nd, ns, nc = _sizes(pool, B, S, P)
    return flat[:nd].reshape(B, H), (flat[nd:nd + ns].reshape(B, S) if ns else None), (flat[nd + ns:nd + ns + nc].reshape(B, S, P) if nc else None)


def _host_forward(hip, ids, mask, pool, P, guard=64):
    """through the C ABI with a HOST out pre-filled with poison: (rc, blocks, guard words)"""
    B, S = ids.shape
    total = sum(_sizes(pool, B, S, P))
    out = np.full(total + guard, POISON)
    rc = hip._lib.kr_encoder_forward(hip._h, ids.ctypes.data, mask.ctypes.data, B, S, pool, out.ctypes.data, None)
    return rc, _split(out, pool, B, S, P), out[total:]


def _dev_forward(hip, ids, mask, pool, P, guard=64):
    """the same with a DEVICE out: the token-level blocks come straight from the kernels"""
    B, S = ids.shape
    total = sum(_sizes(pool, B, S, P))
    out = torch.full((total + guard,), float(POISON), dtype=torch.float32, device="cuda")
    i, k = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    torch.cuda.synchronize()
    rc = hip._lib.kr_encoder_forward(hip._h, i.data_ptr(), k.data_ptr(), B, S, pool, out.data_ptr(), None)
    if rc == 0:
        rc = hip._lib.kr_encoder_check(hip._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return rc, _split(o, pool, B, S, P), o[total:]


@functools.lru_cache(maxsize=None)
def _case(kind, S, P, variant):
    """one parity case, computed once: ids, mask, the reference blocks (fp64), the library's blocks (host out, CLS pooling, both flags)"""
    ids, mask = M.batch(kind, 5, S, variant, seed=S + (0 if kind == "xlmr" else 1000))
    lh = M.last_hidden(_hf(kind), ids, mask)
    ref_s, ref_c = M.ref_blocks(lh, mask, M.heads_for(kind, P))
    rc, (dense, sparse, colbert), guard = _host_forward(_hip(kind, P), ids, mask, POOL_CLS | SPARSE | COLBERT, P)
    assert rc == 0, _hip(kind, P)._lib.kr_last_error()
    assert (guard == POISON).all()
    for a in (ids, mask, ref_s, ref_c, dense, sparse, colbert):
        a.setflags(write=False)
    return ids, mask, lh, ref_s, ref_c, dense, sparse, colbert


# ---------------------------------------------------------------------------------------------------------
# 1. lifecycle and refusals through the raw handle
# ---------------------------------------------------------------------------------------------------------
def _raw_handle(heads=2, layers=1, type_vocab=1):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(H, layers, heads, 256, M.VOCAB, M.MAX_POS + 2, type_vocab, 1e-5)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _load(lib, h, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)


def _fresh(tensors, pad=True, **kw):
    lib, h = _raw_handle(**kw)
    if pad:
        assert _load(lib, h, "config.position_padding_idx", [1.0]) == 0
    for k, v in tensors.items():
        assert _load(lib, h, k, v) == 0, (k, lib.kr_last_error())
    return lib, h


def _one_layer_xlmr():
    return X.weights(H, 1, 256, M.VOCAB, M.MAX_POS + 2, seed=3)


def test_lifecycle_and_refusals_through_the_c_abi():
    back, hw = _one_layer_xlmr(), M.heads(H, 128)
    colbert = {k: hw[k] for k in M.HEADS[:2]}
    sparse = {k: hw[k] for k in M.HEADS[2:]}
    ids, mask = M.batch("xlmr", 3, 12, "right", seed=5)
    B, S = ids.shape

    def fwd(lib, h, pool, n):
        out = np.full(n, POISON)
        return lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, out.ctypes.data, None), out

    lib, h = _fresh({**back, **hw})
    try:
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        full = B * H + B * S + B * S * 128
        for pool in (POOL_MEAN, POOL_CLS):
            rc, out = fwd(lib, h, pool | SPARSE | COLBERT, full)
            assert rc == 0 and (out != POISON).all() and np.isfinite(out).all(), lib.kr_last_error()
        # pool = 3 stays refused, and so does every bit that is no flag, the flags on classify, the flags in the packed entry point
        for pool in (3, 2 | SPARSE, 2 | COLBERT, 0x40, 0x08 | SPARSE, 0x100 | POOL_CLS, SPARSE | COLBERT | 0x80, -1):
            assert fwd(lib, h, pool, full)[0] == KR_EINVAL, pool
        tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32)
        out = np.zeros(full, np.float32)
        for flags in (SPARSE, COLBERT, SPARSE | COLBERT):
            rc = lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), POOL_CLS | flags, out.ctypes.data, None)
            assert rc == KR_EINVAL and b"kr_encoder_forward_packed" in lib.kr_last_error()
        assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), POOL_CLS, out.ctypes.data, None) == 0
        # token types go through the flagged forward too
        tt = np.zeros_like(ids)
        out = np.full(full, POISON)
        assert lib.kr_encoder_forward_tt(h, ids.ctypes.data, mask.ctypes.data, tt.ctypes.data, B, S, POOL_CLS | SPARSE | COLBERT, out.ctypes.data, None) == 0
        assert _same(out, fwd(lib, h, POOL_CLS | SPARSE | COLBERT, full)[1])
        # a head is fixed at the first finalize: another P is refused, the same P takes new values
        other = M.heads(H, 256)
        assert _load(lib, h, M.HEADS[0], other[M.HEADS[0]]) == KR_EINVAL and b"P = 256" in lib.kr_last_error()
        assert _load(lib, h, M.HEADS[1], other[M.HEADS[1]]) == KR_EINVAL
        again = M.heads(H, 128, seed=99)
        before = fwd(lib, h, POOL_CLS | SPARSE | COLBERT, full)[1]
        for k in M.HEADS:
            assert _load(lib, h, k, again[k]) == 0, k
        assert lib.kr_encoder_finalize(h) == 0
        after = fwd(lib, h, POOL_CLS | SPARSE | COLBERT, full)[1]
        assert _same(before[:B * H], after[:B * H]) and np.abs(after[B * H + B * S:] - before[B * H + B * S:]).max() > 0.01
        # shapes
        assert _load(lib, h, M.HEADS[2], np.zeros(H + 1)) == KR_EINVAL
        assert _load(lib, h, M.HEADS[3], np.zeros(2)) == KR_EINVAL
    finally:
        lib.kr_encoder_destroy(h)
    # P: a multiple of 128 in 128 .. 2048; weight and bias agree
    lib, h = _fresh({})
    try:
        for P in (64, 192, 2176, 0):
            assert _load(lib, h, M.HEADS[0], np.zeros(P * H if P else H - 1)) == KR_EINVAL, P
        assert _load(lib, h, M.HEADS[1], np.zeros(100)) == KR_EINVAL
        assert _load(lib, h, M.HEADS[0], np.zeros(2048 * H)) == 0
        assert _load(lib, h, M.HEADS[1], np.zeros(128)) == KR_EINVAL and b"2048" in lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(h)
    # one head only: the other flag is KR_ESTATE naming its tensors; the missing head cannot arrive after the first finalize
    for have, flag, miss_flag, miss in ((colbert, COLBERT, SPARSE, sparse), (sparse, SPARSE, COLBERT, colbert)):
        lib, h = _fresh({**back, **have})
        try:
            assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
            assert fwd(lib, h, POOL_CLS | flag, B * H + B * S * 128)[0] == 0
            rc, _ = fwd(lib, h, POOL_CLS | miss_flag, B * H + B * S * 128)
            assert rc == KR_ESTATE and all(k.encode() in lib.kr_last_error() for k in miss), lib.kr_last_error()
            assert fwd(lib, h, POOL_CLS | SPARSE | COLBERT, B * H + B * S * 129)[0] == KR_ESTATE
            for k, v in miss.items():
                assert _load(lib, h, k, v) == KR_EINVAL and b"finalized without" in lib.kr_last_error()
        finally:
            lib.kr_encoder_destroy(h)
    # a partial pair: never loaded
    for drop in M.HEADS:
        lib, h = _fresh({**back, **{k: v for k, v in hw.items() if k != drop}})
        try:
            assert lib.kr_encoder_finalize(h) == KR_ESTATE and b"never loaded" in lib.kr_last_error() and drop.encode() in lib.kr_last_error(), drop
        finally:
            lib.kr_encoder_destroy(h)
    # other families, the classification head, the Dense head: refused at finalize, naming the tensor
    import reranker_util as R
    import t5_util as T
    others = {"T5": ({T.SETTING: [0.0], **T.weights(H, 1, 2, 256, M.VOCAB, T.RELU)}, False),
              "NomicBert": ({"config.rotary_inv_freq": np.ones(32)}, False),
              "ModernBert": ({"config.rotary_inv_freq": np.ones(32), "config.local_attention_layers": [0.0]}, False),
              "MPNet": ({"encoder.relative_attention_bias.weight": np.zeros(32 * 2)}, True),
              "classifier": ({**back, **R.head(H, 1)}, True),
              "dense.weight": ({**back, "dense.weight": T.dense_weight(8, H)}, True)}
    for word, (tensors, pad) in others.items():
        for head in (colbert, sparse):
            lib, h = _fresh({**tensors, **head}, pad=pad)
            try:
                rc = lib.kr_encoder_finalize(h)
                err = lib.kr_last_error()
                assert rc == KR_EINVAL and next(iter(head)).encode() in err and word.encode() in err, (word, err)
            finally:
                lib.kr_encoder_destroy(h)


# ---------------------------------------------------------------------------------------------------------
# 2. element-wise parity with the reference
# ---------------------------------------------------------------------------------------------------------
VARIANTS = ("right", "left", "holes")
PARITY = [(kind, S, P) for kind in ("xlmr", "bert") for S in (12, 40, 150) for P in (128, 256)]


def parity_figures(kind, S, P, variant):
    ids, mask, lh, ref_s, ref_c, dense, sparse, colbert = _case(kind, S, P, variant)
    cos, elem = M.colbert_errors(colbert, ref_c, mask)
    return cos, elem, float(np.abs(sparse - ref_s)[mask != 0].max())


@pytest.mark.parametrize("kind,S,P", PARITY)
def test_both_blocks_match_the_reference_element_by_element(kind, S, P):
    for variant in VARIANTS:
        ids, mask, lh, ref_s, ref_c, dense, sparse, colbert = _case(kind, S, P, variant)
        cos, elem, dw = parity_figures(kind, S, P, variant)
        print(f"{kind} S={S} P={P} {variant}: 1-cos {cos:.3e} |d elem| {elem:.3e} |d w| {dw:.3e}")
        assert cos <= M.BARS["colbert_cos"] and elem <= M.BARS["colbert_elem"] and dw <= M.BARS["sparse"], (variant, cos, elem, dw)
        # attended vectors are unit vectors, the dense block is the CLS embedding
        assert np.abs(np.linalg.norm(colbert[mask != 0].astype(np.float64), axis=-1) - 1.0).max() < 1e-6
        ref_d = torch.nn.functional.normalize(lh[:, 0], dim=-1).numpy()
        assert np.abs((dense * ref_d).sum(-1) - 1.0).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------
# 3. teeth
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_every_mutant_of_the_heads_is_far_outside_the_bars(kind):
    """each broken restatement moves the block it touches by more than 10 bars on the reference itself, and the library stays inside one bar of the whole one"""
    P = 128
    pos = att = 0
    for S in (12, 40, 150):
        for variant in VARIANTS:
            ids, mask, lh, ref_s, ref_c, dense, sparse, colbert = _case(kind, S, P, variant)
            k = mask != 0
            pos += int((ref_s[k] > 0).sum()); att += int(k.sum())
            for mut in M.MUTATIONS:
                mut_s, mut_c = M.ref_blocks(lh, mask, M.heads_for(kind, P), broken=mut)
                if mut in ("no_colbert_bias", "no_norm", "neighbour_row"):
                    assert M.colbert_errors(mut_c, ref_c, mask)[1] > 10 * M.BARS["colbert_elem"], (mut, S, variant)
                    assert M.colbert_errors(colbert, mut_c, mask)[1] > 9 * M.BARS["colbert_elem"], (mut, S, variant)
                if mut in ("no_sparse_bias", "no_relu", "neighbour_row"):
                    assert np.abs(mut_s - ref_s)[k].max() > 10 * M.BARS["sparse"], (mut, S, variant)
                    assert np.abs(mut_s - sparse)[k].max() > 9 * M.BARS["sparse"], (mut, S, variant)
            for mut in ("no_colbert_bias", "neighbour_row"):      # the direction alone (what the normalisation leaves of them): far outside the cosine bar too
                assert M.colbert_errors(M.ref_blocks(lh, mask, M.heads_for(kind, P), broken=mut)[1], ref_c, mask)[0] > 10 * M.BARS["colbert_cos"], (mut, S, variant)
    share = pos / att
    print(f"{kind}: {share:.3f} of {att} attended tokens have a positive reference weight")
    assert 0.25 <= share <= 0.75, share


# ---------------------------------------------------------------------------------------------------------
# 4. exact invariants
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,S,variant", [("xlmr", 40, "holes"), ("bert", 150, "left"), ("xlmr", 12, "right")])
def test_exact_invariants_of_the_out_layout(kind, S, variant):
    P = 128
    ids, mask, lh, ref_s, ref_c, dense, sparse, colbert = _case(kind, S, P, variant)
    hip, plain = _hip(kind, P), _hip(kind, P, heads=False)
    B = len(ids)
    for base in (POOL_MEAN, POOL_CLS):
        rc, (d0, _, _), g = _host_forward(hip, ids, mask, base, P)
        assert rc == 0 and (g == POISON).all()
        # pools 0 / 1 on a handle with the heads equal a handle without them
        assert _same(d0, _host_forward(plain, ids, mask, base, P)[1][0])
        got = {}
        for flags in (SPARSE, COLBERT, SPARSE | COLBERT):
            for fwd in (_host_forward, _dev_forward):
                rc, (d, s, c), g = fwd(hip, ids, mask, base | flags, P)
                assert rc == 0, hip._lib.kr_last_error()
                assert (g == POISON).all(), "guard words behind the last block"
                assert _same(d, d0), "the dense block is the unflagged call's"
                got[(flags, fwd is _dev_forward)] = (s, c)
        for dev in (False, True):
            # the sparse block with and without 0x20, the colbert block with and without 0x10, host and device out, either base pool
            assert _same(got[(SPARSE, dev)][0], sparse) and _same(got[(SPARSE | COLBERT, dev)][0], sparse)
            assert _same(got[(COLBERT, dev)][1], colbert) and _same(got[(SPARSE | COLBERT, dev)][1], colbert)
    # masked slots are exactly +0.0 (the out was poison), attended ones are written
    k = mask != 0
    assert (sparse.view(np.uint32)[~k] == 0).all() and (colbert.view(np.uint32)[~k] == 0).all()
    assert (colbert[k] != POISON).all() and (np.abs(colbert[k]).sum(-1) > 0).all()
    # a sequence alone, in the batch, in the reversed batch
    rc, (_, s_r, c_r), _ = _host_forward(hip, ids[::-1].copy(), mask[::-1].copy(), POOL_CLS | SPARSE | COLBERT, P)
    assert rc == 0 and _same(s_r[::-1], sparse) and _same(c_r[::-1], colbert)
    for b in (0, 1, B - 1):      # (row 1 of the holes variant has a masked column 0: CLS pooling packs a query-only row for it)
        rc, (_, s_1, c_1), _ = _host_forward(hip, ids[b:b + 1].copy(), mask[b:b + 1].copy(), POOL_CLS | SPARSE | COLBERT, P)
        assert rc == 0 and _same(s_1[0], sparse[b]) and _same(c_1[0], colbert[b])


@pytest.mark.parametrize("kind,S,P", [("xlmr", 40, 256), ("bert", 150, 128)])
def test_projection_tilings_agree_on_the_colbert_block(kind, S, P, monkeypatch):
    ids, mask, lh, ref_s, ref_c, dense, sparse, colbert = _case(kind, S, P, "holes")
    for tile in ("32", "64", "128", "130", "256"):
        monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", tile)
        rc, (d, s, c), _ = _host_forward(_hip(kind, P), ids, mask, POOL_CLS | SPARSE | COLBERT, P)
        assert rc == 0 and _same(c, colbert) and _same(s, sparse) and _same(d, dense), tile


# ---------------------------------------------------------------------------------------------------------
# 5. BGEM3Model end to end
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _m3():
    from kirag_amd.retriever.m3 import BGEM3Model, XLMRobertaM3Encoder
    hw = M.heads_for("xlmr", 128)
    enc = M.hf_backbone("xlmr", M.backbone("xlmr"), "cuda", cls=XLMRobertaM3Encoder)
    enc.set_heads({"weight": torch.from_numpy(hw[M.HEADS[0]]), "bias": torch.from_numpy(hw[M.HEADS[1]])},
                  {"weight": torch.from_numpy(hw[M.HEADS[2]]), "bias": torch.from_numpy(hw[M.HEADS[3]])})
    return BGEM3Model(enc, tokenizer=X.toy_tokenizer()), hw


def test_encode_returns_what_the_raw_blocks_hold():
    m3, hw = _m3()
    sents = M.texts(7, seed=4)
    out = m3.encode(sents, batch_size=4, return_dense=True, return_sparse=True, return_colbert_vecs=True)
    assert set(out) == {"dense_vecs", "lexical_weights", "colbert_vecs"} and out["dense_vecs"].shape == (7, H)
    tok = m3.tokenizer
    skip = {tok.cls_token_id, tok.eos_token_id, tok.pad_token_id, tok.unk_token_id}
    for s in range(0, 7, 4):
        enc = tok(sents[s:s + 4], padding=True, return_tensors="np")
        ids, mask = enc["input_ids"].astype(np.int64), enc["attention_mask"].astype(np.int64)
        rc, (d, sp, c), _ = _host_forward(_hip("xlmr", 128), ids, mask, POOL_CLS | SPARSE | COLBERT, 128)
        assert rc == 0 and _same(out["dense_vecs"][s:s + 4], d)
        for b in range(len(ids)):
            n = int(mask[b].sum())
            assert _same(out["colbert_vecs"][s + b], c[b, 1:n]) and out["colbert_vecs"][s + b].shape == (n - 1, 128)
            want = {}
            for i, w in zip(ids[b, :n], sp[b, :n]):
                if int(i) not in skip and w > 0:
                    want[str(int(i))] = max(float(w), want.get(str(int(i)), 0.0))
            assert out["lexical_weights"][s + b] == want
    only = m3.encode(sents[:3])
    assert only["lexical_weights"] is None and only["colbert_vecs"] is None and _same(only["dense_vecs"], out["dense_vecs"][:3])
    from kirag_amd.retriever.m3 import BGEM3Model
    with pytest.raises(ValueError, match="padding_side"):
        BGEM3Model(m3.model, tokenizer=X.toy_tokenizer(padding_side="left")).encode(sents[:2], return_colbert_vecs=True)


def test_lexical_key_sets_scores_and_ranking_follow_the_reference():
    m3, hw = _m3()
    query = M.texts(1, seed=11, lo=8, hi=8)[0]
    passages = M.texts(64, seed=12)
    ref_q = M.ref_encode(_hf("xlmr"), hw, m3.tokenizer, [query])[0]
    ref_p = M.ref_encode(_hf("xlmr"), hw, m3.tokenizer, passages)
    got = m3.encode(passages, batch_size=64, return_sparse=True, return_colbert_vecs=True)
    # key sets: equal to the reference's for every token id whose reference weights (w . x + b, before the ReLU) are all farther than the sparse bar from 0
    inside = total = 0
    skip = m3._skip_ids()
    for (d, lw, cv, ids, w), lex in zip(ref_p, got["lexical_weights"]):
        total += len(ids)
        near = {str(int(i)) for i, x in zip(ids, w) if abs(x) <= M.BARS["sparse"] and int(i) not in skip}
        inside += sum(1 for x in w if abs(x) <= M.BARS["sparse"])
        assert set(lex) - near == set(lw) - near
        for k in set(lex) & set(lw):
            assert abs(lex[k] - lw[k]) <= M.BARS["sparse"]
    print(f"{inside} of {total} attended tokens lie within the sparse bar of 0")
    assert inside <= 0.05 * total
    # the five scores
    weights = (0.4, 0.2, 0.4)
    scores = m3.compute_score([(query, p) for p in passages], weights=weights, batch_size=64)
    ref = [M.ref_scores(ref_q, p, weights) for p in ref_p]
    worst = {}
    for key in ("dense", "sparse", "colbert", "sparse+dense", "colbert+sparse+dense"):
        assert len(scores[key]) == 64
        worst[key] = max(abs(a - r[key]) for a, r in zip(scores[key], ref))
    print("worst |score - reference|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= M.SCORE_BAR for v in worst.values()), worst
    # rerank orders the passages as the reference does wherever the reference's scores differ by more than 2 bars
    order, top = m3.rerank(query, passages, weights=weights)
    order = order.numpy()
    assert sorted(order.tolist()) == list(range(64)) and np.all(np.diff(top.numpy()) <= 0)
    r = np.array([x["colbert+sparse+dense"] for x in ref])
    assert np.abs(top.numpy() - r[order]).max() <= M.SCORE_BAR
    rank = np.empty(64, np.int64); rank[order] = np.arange(64)
    far = r[:, None] - r[None, :] > 2 * M.SCORE_BAR
    print(f"{int(far.sum())} of 2016 passage pairs are decided by the reference")
    assert far.sum() >= 1008                                               # at least half of the pairs are decided by the reference
    assert not np.any(far & (rank[:, None] > rank[None, :]))
    o5, s5 = m3.rerank(query, passages, top_k=5, weights=weights)
    assert np.array_equal(o5.numpy(), order[:5]) and _same(s5.numpy(), top.numpy()[:5])


# ---------------------------------------------------------------------------------------------------------
# 6. non-finite head weights
# ---------------------------------------------------------------------------------------------------------
def test_a_nan_in_the_colbert_weight_is_kr_erange_for_flagged_forwards_only():
    from kirag_amd.retriever.encoders import HipBertForward
    hw = {k: v.copy() for k, v in M.heads_for("xlmr", 128).items()}
    hw[M.HEADS[0]][17, 5] = np.nan
    hip = HipBertForward(M.cfg("xlmr", *M.SHAPES["xlmr"]), 0)
    hip.load_state({**M.backbone("xlmr"), **hw})
    ids, mask = M.batch("xlmr", 5, 12, "right", seed=2)
    for fwd in (_host_forward, _dev_forward):
        rc, _, _ = fwd(hip, ids, mask, POOL_CLS | COLBERT, 128)
        assert rc == KR_ERANGE, hip._lib.kr_last_error()
        rc, (d, s, _), _ = fwd(hip, ids, mask, POOL_CLS | SPARSE, 128)
        assert rc == 0 and np.isfinite(d).all() and np.isfinite(s).all()
        rc, (d, _, _), _ = fwd(hip, ids, mask, POOL_CLS, 128)
        assert rc == 0 and np.isfinite(d).all()
    # ... and a NaN sparse weight likewise
    hw = {k: v.copy() for k, v in M.heads_for("xlmr", 128).items()}
    hw[M.HEADS[2]][0, 3] = np.nan
    hip = HipBertForward(M.cfg("xlmr", *M.SHAPES["xlmr"]), 0)
    hip.load_state({**M.backbone("xlmr"), **hw})
    assert _host_forward(hip, ids, mask, POOL_CLS | SPARSE, 128)[0] == KR_ERANGE
    assert _host_forward(hip, ids, mask, POOL_CLS | COLBERT, 128)[0] == 0


def test_checkpoint_check_reports_a_bge_m3_folder(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import checkpoint_check as CC
    m3, hw = _m3()
    d = str(tmp_path / "m3")
    m3.model.save_pretrained(d)
    out = CC.check(d, CC.parse([d, "--random-tokens", "--n", "4", "--max-length", "24"]))
    assert out["kind"] == "bge-m3" and len(out["modes"]) == 4
    best = out["modes"][0]                                   # f16 + low half, the default
    assert best["finite"] and best["worst_token_1_minus_cos"] <= M.BARS["colbert_cos"] and best["worst_sparse_weight_error"] <= M.BARS["sparse"]


def test_the_heads_at_the_width_they_are_for():
    """H = 1024 and P = 1024 (bge-m3's own widths; one layer, 3 x 20 tokens with holes): k_m3_sparse takes four 256-column steps per row and k_m3_rows sixteen,
    which H = 128 / P <= 256 never do.  Checked against float64 on the library's OWN final rows (kr_encoder_last_hidden), inside a-priori bounds with
    u = 2^-24 and t = the unit roundoff of the handle's operand type (f16 2^-11, bf16 2^-8):
      sparse   |w - w64| <= (H + 2) u (sum |w_i x_i| + |b|): an fp32 FMA chain and butterfly over H terms plus the bias, in any order;
      colbert  y = Wh . xh from the 16-bit operands, A_i = sum_j |Wh_ij xh_j|, e_i = t |y_i| + (H u + t / 64) A_i (the 16-bit store; fp32 accumulation in any
               order; the rows are read back decoded to 19 bits, which re-rounds about 1 element in 256 to the neighbouring 16-bit value);
               |v_i / |v| - ref_i| <= (e_i + |ref_i| |e|) / |v| + 8 u for v = y + bias (a perturbation of a normalised vector, and the fp32 norm and division)."""
    from kirag_amd.retriever.encoders import HipBertForward
    HW, P, B, S = 1024, 1024, 3, 20
    c = X.cfg(HW, 1, 16, 1024, M.VOCAB, M.MAX_POS + 2)
    hw = M.heads(HW, P, seed=41)
    hip = HipBertForward(c, 0)
    hip.load_state({**X.weights(HW, 1, 1024, M.VOCAB, M.MAX_POS + 2, seed=5), **hw})
    ids, mask = M.batch("xlmr", B, S, "holes", seed=9)
    dense, sparse, colbert = hip.forward_np(ids, mask, POOL_CLS | SPARSE | COLBERT)
    x = hip.last_hidden(B, S).double().numpy()
    k = mask != 0
    u, t = 2.0 ** -24, (2.0 ** -11 if hip.operand_dtype == "f16" else 2.0 ** -8)
    half = torch.float16 if hip.operand_dtype == "f16" else torch.bfloat16
    assert (sparse.view(np.uint32)[~k] == 0).all() and (colbert.view(np.uint32)[~k] == 0).all() and np.isfinite(colbert).all()
    ws, bs = hw[M.HEADS[2]].astype(np.float64)[0], float(hw[M.HEADS[3]][0])
    pre = x @ ws + bs
    bound = (HW + 2) * u * (np.abs(x) @ np.abs(ws) + abs(bs))
    err = np.abs(sparse.astype(np.float64) - np.maximum(pre, 0.0))
    print(f"sparse: worst |w - w64| {err[k].max():.3e}, smallest bound {bound[k].min():.3e}")
    assert (err[k] <= bound[k]).all() and (pre[k] > 0).any() and (pre[k] < 0).any()
    Wh = torch.from_numpy(hw[M.HEADS[0]]).to(half).double().numpy()
    xh = torch.from_numpy(x).float().to(half).double().numpy()
    y = xh @ Wh.T
    A = np.abs(xh) @ np.abs(Wh).T
    e = t * np.abs(y) + (HW * u + t / 64) * A
    v = y + hw[M.HEADS[1]].astype(np.float64)
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    ref = v / n
    bnd = (e + np.abs(ref) * np.linalg.norm(e, axis=-1, keepdims=True)) / n + 8 * u
    errc = np.abs(colbert.astype(np.float64) - ref)
    print(f"colbert: worst |element - float64| {errc[k].max():.3e}, worst error / bound {(errc[k] / bnd[k]).max():.3f}")
    assert (errc[k] <= bnd[k]).all()
    assert np.abs(np.linalg.norm(colbert[k].astype(np.float64), axis=-1) - 1.0).max() < 1e-6
