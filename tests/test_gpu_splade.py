"""GPU tests of the SPLADE head (KR_POOL_SPLADE): the contract through the C ABI, element-wise parity of all B x V weights against
``transformers.BertForMaskedLM`` fp32 + log1p(relu(.)) max-pooled in fp64 (both head widths, V = 1031 and 1280, right / left padding, masks with holes,
sequence boundaries inside 32-row blocks, a sequence across 256-row tiles, an all-masked sequence), the teeth of that bar, the exact invariants (a sequence
alone / in a batch / reversed / packed, every projection tiling, call after call, pools 0 / 1 untouched), non-finite head weights, and SpladeModel end to
end.  Synthetic weights (splade_util); no SPLADE checkpoint exists offline.

Bar (splade_util.BAR): |w - reference w|, twice the worst value measured over the parity cases of this file on one MI355X
(profiles/splade/measurements.txt, section 1):
    worst 3.4594e-03   bar 7.0e-03"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splade_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL, KR_ESTATE, KR_ERANGE = -22, -1, -34
POOL_MEAN, POOL_CLS, SPLADE = 0, 1, 4
H = U.H
POISON = np.float32(-7.0)
KINDS = (("h32", 1031), ("h64", 1280))


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _weights(V):
    return {**U.backbone(V), **U.head(V)}


@functools.lru_cache(maxsize=None)
def _hf(kind, V):
    return U.hf_mlm(kind, V, _weights(V), "cuda")


@functools.lru_cache(maxsize=None)
def _hip(kind, V, head=True):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(U.lib_cfg(kind, V), 0)
    h.load_state(_weights(V) if head else U.backbone(V))
    return h


def _host_forward(hip, ids, mask, pool, width, guard=64):
    """through the C ABI with a HOST out pre-filled with poison: (rc, [B, width], guard words)"""
    B, S = ids.shape
    out = np.full(B * width + guard, POISON)
    rc = hip._lib.kr_encoder_forward(hip._h, ids.ctypes.data, mask.ctypes.data, B, S, pool, out.ctypes.data, None)
    return rc, out[:B * width].reshape(B, width), out[B * width:]


def _dev_forward(hip, ids, mask, pool, width, guard=64):
    """the same with a DEVICE out: the reduction runs in the caller's buffer"""
    B, S = ids.shape
    out = torch.full((B * width + guard,), float(POISON), dtype=torch.float32, device="cuda")
    i, k = torch.tensor(ids).cuda(), torch.tensor(mask).cuda()
    torch.cuda.synchronize()
    rc = hip._lib.kr_encoder_forward(hip._h, i.data_ptr(), k.data_ptr(), B, S, pool, out.data_ptr(), None)
    if rc == 0:
        rc = hip._lib.kr_encoder_check(hip._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return rc, o[:B * width].reshape(B, width), o[B * width:]


def _packed_forward(hip, ids, mask, pool, width):
    """kr_encoder_forward_packed on the attended ids of a right-padded batch"""
    B, S = ids.shape
    tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32)
    out = np.full(B * width, POISON)
    rc = hip._lib.kr_encoder_forward_packed(hip._h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), pool, out.ctypes.data, None)
    return rc, out.reshape(B, width)


@functools.lru_cache(maxsize=None)
def _case(kind, V, name):
    """one parity case, computed once: ids, mask, the reference (fp64), the library's [B, V] (host out)"""
    ids, mask = U.case_batch(name, V)
    ref = U.reference(_hf(kind, V), ids, mask)
    rc, got, guard = _host_forward(_hip(kind, V), ids, mask, SPLADE, V)
    assert rc == 0, _hip(kind, V)._lib.kr_last_error()
    assert (guard == POISON).all()
    for a in (ids, mask, ref, got):
        a.setflags(write=False)
    return ids, mask, ref, got


# ---------------------------------------------------------------------------------------------------------
# 1. the contract through the raw handle
# ---------------------------------------------------------------------------------------------------------
V0 = 1031


def _raw_handle(heads=2, layers=1, V=V0):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(H, layers, heads, U.FF, V, U.MAX_POS, 2, U.LN_EPS)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _load(lib, h, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)


def _fresh(tensors, **kw):
    lib, h = _raw_handle(**kw)
    for k, v in tensors.items():
        assert _load(lib, h, k, v) == 0, (k, lib.kr_last_error())
    return lib, h


def _one_layer(V=V0):
    return dict(U.E.synth_weights(H, 1, U.FF, V, U.MAX_POS, seed=3))


def test_pool_4_and_the_six_names_are_accepted():
    """the test that fails without the feature: pool = 4 was KR_EINVAL and the six names were unknown tensor names"""
    back, hw = _one_layer(), U.head(V0)
    ids, mask = U.batch(V0, [12, 5, 9], 12, seed=5)
    lib, h = _fresh(back)
    try:
        for k in U.MLM:
            assert _load(lib, h, k, hw[k]) == 0, (k, lib.kr_last_error())
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        out = np.full(3 * V0, POISON)
        assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, 3, 12, SPLADE, out.ctypes.data, None) == 0, lib.kr_last_error()
        assert np.isfinite(out).all() and (out >= 0).all() and (out > 0).any() and (out == 0).any()
    finally:
        lib.kr_encoder_destroy(h)


def test_lifecycle_and_refusals_through_the_c_abi():
    back, hw = _one_layer(), U.head(V0)
    ids, mask = U.batch(V0, [12, 5, 9], 12, seed=5)
    B, S = ids.shape

    def fwd(lib, h, pool, n=B * V0):
        out = np.full(n, POISON)
        return lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, out.ctypes.data, None), out

    # without the head: KR_ESTATE naming the tensors; the head cannot arrive after the first finalize
    lib, h = _fresh(back)
    try:
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        rc, _ = fwd(lib, h, SPLADE)
        assert rc == KR_ESTATE and b"cls.predictions.decoder" in lib.kr_last_error() and b"cls.predictions.transform" in lib.kr_last_error()
        for k in U.MLM:
            assert _load(lib, h, k, hw[k]) == KR_EINVAL and b"finalized without" in lib.kr_last_error(), k
        assert fwd(lib, h, POOL_MEAN, B * H)[0] == 0
    finally:
        lib.kr_encoder_destroy(h)
    # with it: the flags, the refused values and bits stay refused; all three entry points take the pool
    lib, h = _fresh({**back, **hw})
    try:
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        rc, base = fwd(lib, h, SPLADE)
        assert rc == 0 and (base != POISON).all(), lib.kr_last_error()
        for pool in (SPLADE | 0x10, SPLADE | 0x20, SPLADE | 0x30, 3, 5, 6, SPLADE | 0x08, SPLADE | 0x40, SPLADE | 0x80, SPLADE | 0x100, 0x10, 0x20):
            rc, _ = fwd(lib, h, pool, B * V0 + B * S * 2)
            assert rc == (KR_ESTATE if pool in (0x10, 0x20) else KR_EINVAL), pool
        tt = np.zeros_like(ids)
        out = np.full(B * V0, POISON)
        assert lib.kr_encoder_forward_tt(h, ids.ctypes.data, mask.ctypes.data, tt.ctypes.data, B, S, SPLADE, out.ctypes.data, None) == 0
        assert _same(out, base)
        tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32)
        out = np.full(B * V0, POISON)
        assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), SPLADE, out.ctypes.data, None) == 0
        assert _same(out, base)
        # a decoder with V +- 1 rows, and the other shapes
        for rows in (V0 - 1, V0 + 1):
            assert _load(lib, h, U.MLM[4], np.zeros(rows * H)) == KR_EINVAL and b"vocab_size" in lib.kr_last_error(), rows
            assert _load(lib, h, U.MLM[5], np.zeros(rows)) == KR_EINVAL, rows
        assert _load(lib, h, U.MLM[0], np.zeros(H * H + 1)) == KR_EINVAL
        for k in U.MLM[1:4]:
            assert _load(lib, h, k, np.zeros(H + 1)) == KR_EINVAL, k
        # the same shapes take new values; the backbone's pools do not move
        mean_before = fwd(lib, h, POOL_MEAN, B * H)[1]
        again = U.head(V0, seed=99)
        for k in U.MLM:
            assert _load(lib, h, k, again[k]) == 0, k
        assert fwd(lib, h, SPLADE)[0] == KR_ESTATE        # between load and finalize
        assert lib.kr_encoder_finalize(h) == 0
        rc, after = fwd(lib, h, SPLADE)
        assert rc == 0 and np.abs(after - base).max() > 0.1
        assert _same(fwd(lib, h, POOL_MEAN, B * H)[1], mean_before)
    finally:
        lib.kr_encoder_destroy(h)
    # a partial set: never loaded, naming the missing tensor
    for drop in U.MLM:
        lib, h = _fresh({**back, **{k: v for k, v in hw.items() if k != drop}})
        try:
            assert lib.kr_encoder_finalize(h) == KR_ESTATE and b"never loaded" in lib.kr_last_error() and drop.encode() in lib.kr_last_error(), drop
        finally:
            lib.kr_encoder_destroy(h)
    # other families, the classification head, an M3 head: refused at finalize, naming the tensor
    import m3_util as M
    import reranker_util as R
    import t5_util as T
    m3 = M.heads(H, 128)
    others = {"T5": {T.SETTING: [0.0], **T.weights(H, 1, 2, U.FF, V0, T.RELU)},
              "NomicBert": {"config.rotary_inv_freq": np.ones(32)},
              "classifier": {**back, **R.head(H, 1)},
              "sparse_linear": {**back, M.HEADS[2]: m3[M.HEADS[2]], M.HEADS[3]: m3[M.HEADS[3]]},
              "colbert_linear": {**back, M.HEADS[0]: m3[M.HEADS[0]], M.HEADS[1]: m3[M.HEADS[1]]}}
    for word, tensors in others.items():
        lib, h = _fresh({**tensors, **hw})
        try:
            rc = lib.kr_encoder_finalize(h)
            err = lib.kr_last_error()
            assert rc == KR_EINVAL and U.MLM[0].encode() in err and word.encode() in err, (word, err)
        finally:
            lib.kr_encoder_destroy(h)


# ---------------------------------------------------------------------------------------------------------
# 2. element-wise parity with the reference
# ---------------------------------------------------------------------------------------------------------
PARITY = [(kind, V, name) for kind, V in KINDS for name in U.CASES]


@pytest.mark.parametrize("kind,V,name", PARITY)
def test_every_weight_matches_the_reference(kind, V, name):
    ids, mask, ref, got = _case(kind, V, name)
    share = U.zero_share(ref)
    print(f"splade parity {kind} V={V} {name}: zero share {share:.3f}  worst |dw| {np.abs(got - ref).max():.4e}  largest w {ref.max():.3f}")
    assert U.ZERO_SHARE[0] <= share <= U.ZERO_SHARE[1], share          # on the REFERENCE: the ReLU is exercised and not everything is clipped
    assert got.shape == ref.shape == (ids.shape[0], V) and np.isfinite(got).all() and (got >= 0).all()
    assert np.abs(got - ref).max() <= U.BAR
    for b in np.flatnonzero(mask.sum(1) == 0):         # an all-masked sequence: V times +0.0
        assert _same(got[b], np.zeros(V, np.float32))
    rc, dev, guard = _dev_forward(_hip(kind, V), ids, mask, SPLADE, V)
    assert rc == 0 and _same(dev, got) and (guard == POISON).all()


@pytest.mark.parametrize("broken", U.MUTATIONS)
def test_the_bar_has_teeth(broken):
    """each broken head, applied to the reference, moves some entry by more than 10 x the bar; the whole head restated by hand does not"""
    kind, V = KINDS[0]
    worst, whole = 0.0, 0.0
    for name in ("s12_left", "s40_holes", "ragged", "masked"):
        ids, mask, ref, _ = _case(kind, V, name)
        worst = max(worst, float(np.abs(U.by_hand(_hf(kind, V), _weights(V), ids, mask, broken) - ref).max()))
        whole = max(whole, float(np.abs(U.by_hand(_hf(kind, V), _weights(V), ids, mask) - ref).max()))
    print(f"splade teeth {broken}: moves {worst:.4e} (whole head by hand: {whole:.2e})")
    assert U.BAR > 0 and worst > 10 * U.BAR and whole < U.BAR / 10


# ---------------------------------------------------------------------------------------------------------
# 3. bit identity
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,V", KINDS)
def test_a_row_does_not_depend_on_its_batch_or_entry_point(kind, V):
    hip = _hip(kind, V)
    ids, mask, _, got = _case(kind, V, "ragged")
    B, S = ids.shape
    rc, again, _ = _host_forward(hip, ids, mask, SPLADE, V)
    assert rc == 0 and _same(again, got)                                       # call after call: the atomics
    rc, rev, _ = _host_forward(hip, ids[::-1].copy(), mask[::-1].copy(), SPLADE, V)
    assert rc == 0 and _same(rev[::-1], got)
    for b in range(B):
        rc, one, _ = _host_forward(hip, ids[b:b + 1].copy(), mask[b:b + 1].copy(), SPLADE, V)
        assert rc == 0 and _same(one[0], got[b]), b
    rc, packed = _packed_forward(hip, ids, mask, SPLADE, V)
    assert rc == 0 and _same(packed, got)


@pytest.mark.parametrize("tile", ["256", "130", "128", "64", "32"])
def test_every_projection_tiling_gives_the_same_bits(tile, monkeypatch):
    kind, V = KINDS[0]
    monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", tile)
    for name in ("ragged", "long", "masked"):
        ids, mask, _, got = _case(kind, V, name)
        rc, forced, guard = _host_forward(_hip(kind, V), ids, mask, SPLADE, V)
        assert rc == 0 and _same(forced, got) and (guard == POISON).all(), (tile, name)


@pytest.mark.parametrize("kind,V", KINDS)
def test_pools_0_and_1_equal_a_handle_without_the_head(kind, V):
    ids, mask, _, _ = _case(kind, V, "s40_holes")
    for pool in (POOL_MEAN, POOL_CLS):
        rc_a, a, _ = _host_forward(_hip(kind, V), ids, mask, pool, H)
        rc_b, b, _ = _host_forward(_hip(kind, V, head=False), ids, mask, pool, H)
        assert rc_a == 0 and rc_b == 0 and _same(a, b), pool


# ---------------------------------------------------------------------------------------------------------
# 4. non-finite head weights
# ---------------------------------------------------------------------------------------------------------
def test_a_nan_in_the_decoder_is_kr_erange_for_the_splade_pool_only():
    from kirag_amd.retriever.encoders import HipBertForward
    kind, V = KINDS[0]
    w = dict(_weights(V))
    bad = w[U.MLM[4]].copy(); bad[17, 5] = np.nan
    w[U.MLM[4]] = bad
    hip = HipBertForward(U.lib_cfg(kind, V), 0)
    hip.load_state(w)
    ids, mask, _, _ = _case(kind, V, "s12_right")
    rc, _, _ = _host_forward(hip, ids, mask, SPLADE, V)
    assert rc == KR_ERANGE, hip._lib.kr_last_error()
    rc, _, _ = _dev_forward(hip, ids, mask, SPLADE, V)
    assert rc == KR_ERANGE
    for pool in (POOL_MEAN, POOL_CLS):
        rc, out, _ = _host_forward(hip, ids, mask, pool, H)
        assert rc == 0 and np.isfinite(out).all(), pool


# ---------------------------------------------------------------------------------------------------------
# 5. SpladeModel end to end (a tied model, as real checkpoints are)
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _surface():
    import reranker_util as R
    from kirag_amd.retriever.splade import BertSpladeEncoder, SpladeModel
    tok = R.bert_pair_tokenizer()
    V = tok.vocab_size
    w = U.tied_weights(V)
    ref = U.hf_mlm("h64", V, w, "cuda", tie=True)
    twin = U.hf_mlm("h64", V, w, "cuda", cls=BertSpladeEncoder, tie=True)
    return tok, ref, SpladeModel(twin, tokenizer=tok)


def _ref_vectors(texts):
    tok, ref, _ = _surface()
    enc = tok(list(texts), padding=True, truncation=True, max_length=512, return_tensors="np")
    return U.reference(ref, enc["input_ids"].astype(np.int64), enc["attention_mask"].astype(np.int64))


def test_splade_model_encode_scores_and_rerank():
    import reranker_util as R
    tok, _, model = _surface()
    texts = R.passages(24, seed=4)
    ref = _ref_vectors(texts)
    assert 0.05 < U.zero_share(ref) < 0.98
    dense = model.encode_dense(texts, batch_size=7)                  # other batches than the reference's one: a row does not depend on them
    assert dense.is_cuda and tuple(dense.shape) == ref.shape
    assert np.abs(dense.cpu().numpy() - ref).max() <= U.BAR
    # key sets: every token whose reference weight exceeds 2 x the bar is present, nothing with a reference weight of 0 - 2 x bar ... is required
    got = model.encode(texts, batch_size=7)
    for b, d in enumerate(got):
        want = U.ref_token_weights(ref[b], tok, U.BAR)
        sure = {k for k, x in want.items() if x > 2 * U.BAR}
        assert sure <= set(d) and all(x > 0 for x in d.values()) and tok.pad_token not in d
        assert all(abs(d[k] - want.get(k, 0.0)) <= U.BAR for k in d)
    top = model.encode(texts[:3], top_k=5)
    assert all(len(d) == 5 for d in top)
    # compute_score: within (number of shared keys) x bar x (largest weight) of the reference's dot product; a key counts as shared when either side holds it
    pairs = [(texts[i], texts[i + 12]) for i in range(12)]
    scores = model.compute_score(pairs)
    g = dense.cpu().numpy().astype(np.float64)
    pad = tok.pad_token_id
    for (i, s) in enumerate(scores):
        a, b = ref[i].copy(), ref[i + 12].copy()
        a[pad] = b[pad] = 0
        shared = int((((a > 0) | (g[i] > 0)) & ((b > 0) | (g[i + 12] > 0))).sum())
        tol = shared * U.BAR * float(ref.max())
        assert shared > 0 and abs(s - float(a @ b)) <= tol, (i, s, float(a @ b), tol)


def test_rerank_orders_64_passages_as_the_reference_does():
    import reranker_util as R
    tok, _, model = _surface()
    query, passages = R.passages(1, seed=11, lo=8, hi=12)[0], R.passages(64, seed=12)
    ref = _ref_vectors([query] + passages)
    pad = tok.pad_token_id
    q = ref[0].copy(); q[pad] = 0
    p = ref[1:].copy(); p[:, pad] = 0
    want = p @ q
    g = model.encode_dense([query] + passages, batch_size=64).cpu().numpy()
    shared = int((((q > 0) | (g[0] > 0)) & ((p > 0) | (g[1:] > 0))).sum(1).max())          # a key counts as shared when either side holds it
    tol = shared * U.BAR * float(ref.max())
    order, scores = model.rerank(query, passages)
    assert tuple(order.shape) == (64,) and sorted(order.tolist()) == list(range(64))
    assert np.abs(scores.numpy() - want[order.numpy()]).max() <= tol
    pos = {int(i): r for r, i in enumerate(order.tolist())}
    checked = 0
    for i in range(64):
        for j in range(64):
            if want[i] - want[j] > 2 * tol:
                assert pos[i] < pos[j], (i, j)
                checked += 1
    assert checked > 64                       # the tolerance leaves an ordering to check
    top, top_scores = model.rerank(query, passages, top_k=5)
    assert top.tolist() == order[:5].tolist() and torch.equal(top_scores, scores[:5])
    from kirag_amd.retriever import rerankers as RR
    assert RR.HYBRID_RERANKER_MAP["SPLADE"] is type(model) and list(RR.RERANKER_MAP) == ["BGEReranker"]
