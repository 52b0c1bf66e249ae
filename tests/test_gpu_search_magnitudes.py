"""GPU tests of the search's exactness OFF the unit sphere: inputs scaled by powers of two down to 2^-120 and up to overflow, mixed row norms in one index,
rows and queries with inf / NaN elements, scores that round to signed zeros.  The reference everywhere is oracle.search_np.search_canonical on the same fp32
arrays: rows identical and scores bit-identical, except for zero scores, which are compared by value (a zero may come back with either sign: the header's
zero rule).  The corpora are built so that a wrong answer is visible: tests/test_search_magnitudes_host.py asserts that with the oracle alone.

What these cases caught when they were written (profiles/magnitudes/measurements.txt has the case-by-case record):
  * the certificate's error bound was computed from fp32 sums of squares, which are subnormal or 0 for inputs below ~2^-64: pass 1 then certified the 16-bit
    top-k of a corpus it must refuse;
  * -0.0 and +0.0 were ranked as different scores by the sort keys but as ties by the merges."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import search_np as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magnitude_util as M  # noqa: E402
from test_gpu_search import byte_everywhere  # noqa: E402,F401  (the fixture: small blocks take the int8 pre-scan at every index size)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(s, i, so, io, tag, zeros_by_value=True):
    """rows identical; scores bit-identical, zeros by value"""
    assert np.array_equal(i, io), (tag, "rows", int((i != io).sum()), i[(i != io).any(axis=1)][:1], io[(i != io).any(axis=1)][:1])
    ne = _bits(s) != _bits(so)
    if zeros_by_value:
        ne &= ~((s == 0) & (so == 0))
    assert not ne.any(), (tag, "score bits", s[ne][:4], so[ne][:4])


def _index(d, x, coarse="bf16"):
    from kirag_amd.retriever.index import FlatIPIndex
    ix = FlatIPIndex(d, device=0, coarse_dtype=coarse)
    ix.add(x)
    return ix


def _all_modes(ix, q, k, so, io, tag):
    """modes 0 (auto), 1 (exact scan only), 2 (fp64 pass only) against the oracle; returns the statistics of the mode-0 search"""
    st0 = None
    for mode in (0, 1, 2):
        ix.stats(reset=True)
        s, i = ix.search(q, k, mode=mode)
        st = ix.stats()
        _same(s, i, so, io, (tag, "mode", mode))
        if mode == 0:
            st0 = st
            assert st["queries"] == len(q) and st["certified"] + st["fallback"] == len(q), (tag, st)
    return st0


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. scale sweep on the cluster corpus
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cluster(n, d, nq):
    q, x = M.dense_cluster(n, d, nq, seed=n + d)
    q.setflags(write=False); x.setflags(write=False)
    return q, x


@functools.lru_cache(maxsize=None)
def _cluster_oracle(n, d, nq, k, eq, ex):
    q, x = _cluster(n, d, nq)
    if (eq, ex) == (0, 0):
        return S.search_canonical(q, x, k)
    qs, xs = M.scaled(q, x, eq, ex)
    return S.search_canonical(qs, xs, k)


def _scale_case(n, d, nq, k, coarse, eq, ex, tag):
    q, x = _cluster(n, d, nq)
    qs, xs = M.scaled(q, x, eq, ex)
    so, io = _cluster_oracle(n, d, nq, k, eq, ex)
    ix = _index(d, xs, coarse)
    st = _all_modes(ix, qs, k, so, io, tag)
    print(f"[{tag}] pass 1 certified {st['certified']} of {nq} queries (fine {st['fine']}, exact {st['exact']})")
    # invariance: where the scaling is exact and no score is subnormal or inf, the scaled search asks the unscaled question
    if M.scaling_is_exact(q, qs, eq) and M.scaling_is_exact(x, xs, ex) and M.scores_normal(so) and -125 < eq + ex < 126:
        _, io0 = _cluster_oracle(n, d, nq, k, 0, 0)
        s, i = ix.search(qs, k)
        assert np.array_equal(i, io0), (tag, "invariance")


_PAIRS = [("bf16", eq, ex) for eq, ex in M.SCALE_PAIRS] + [("f16", eq, ex) for eq, ex in M.SCALE_PAIRS + M.F16_ONLY_PAIRS]


@pytest.mark.parametrize("coarse,eq,ex", _PAIRS)
@pytest.mark.parametrize("n,d,nq,k", M.CLUSTER_SHAPES)
def test_cluster_scale_sweep_vs_canonical(n, d, nq, k, coarse, eq, ex):
    """The corpus of test_dense_cluster_forces_exact_fallback (rows closer together than one 16-bit step: the 16-bit top-k misses half of the exact one) with
    queries scaled by 2^eq and rows by 2^ex.  At unit scale the certificate refuses this corpus; it must refuse it - or be right - at every scale."""
    _scale_case(n, d, nq, k, coarse, eq, ex, f"cluster {n}x{d} nq {nq} {coarse} q 2^{eq} x 2^{ex}")


@pytest.mark.parametrize("coarse,eq,ex", _PAIRS)
def test_cluster_scale_sweep_through_the_byte_prescan(byte_everywhere, coarse, eq, ex):
    """The same sweep with the int8 final round on (k_quant8_rows / k_scan8_prep bounds)."""
    n, d, nq, k = M.CLUSTER_SHAPES[1]
    _scale_case(n, d, nq, k, coarse, eq, ex, f"cluster+byte {n}x{d} nq {nq} {coarse} q 2^{eq} x 2^{ex}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. mixed magnitudes in one index
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [4, 40])
def test_mixed_row_norms_in_one_index(nq):
    """Row norms log-uniform in [2^-10, 2^10]: the bounds are set by the largest rows, the answer holds rows of every size."""
    n, d, k = 20000, 384, 20
    q, x, _ = M.mixed_norms(n, d, nq, seed=nq)
    so, io = S.search_canonical(q, x, k)
    _all_modes(_index(d, x), q, k, so, io, f"mixed norms nq {nq}")


@pytest.mark.parametrize("nq", [4, 40])
def test_unit_corpus_with_one_huge_and_one_tiny_row(nq):
    n, d, k = 20000, 384, 20
    q, x, (big, small) = M.two_outlier_norms(n, d, nq, seed=100 + nq)
    so, io = S.search_canonical(q, x, k)
    _all_modes(_index(d, x), q, k, so, io, f"outlier norms nq {nq}")


@pytest.mark.parametrize("nq", [4, 40])
def test_mixed_row_norms_added_in_two_calls_small_half_first(nq):
    """The same rows through two index_data calls, the small-norm half first: the bounds grow after the first search."""
    from kirag_amd.retriever.index import Indexer
    n, d, k = 20000, 384, 20
    q, x, norms = M.mixed_norms(n, d, nq, seed=nq)
    x = np.ascontiguousarray(x[np.argsort(norms, kind="stable")])
    ix = Indexer(d)
    ix.index_data([str(j) for j in range(n // 2)], x[:n // 2])
    b1 = ix.index.bounds()
    so, io = S.search_canonical(q, x[:n // 2], k)
    s, i = ix.index.search(q, k)
    _same(s, i, so, io, "first half")
    ix.index_data([str(j) for j in range(n // 2, n)], x[n // 2:])
    b2 = ix.index.bounds()
    assert (b2 > b1).all(), (b1, b2)
    so, io = S.search_canonical(q, x, k)
    _all_modes(ix.index, q, k, so, io, f"two adds nq {nq}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. non-finite elements
# ---------------------------------------------------------------------------------------------------------------------------------------
def _nonfinite_case(n, d, nq, k, tag):
    q, x, rows = M.nonfinite_rows(n, d, nq, seed=n + d)
    so, io = S.search_canonical(q, x, k)
    _all_modes(_index(d, x), q, k, so, io, tag + " rows")
    q2, x2, col = M.inf_query(n, d, nq, k, seed=n + d + 1)
    so2, io2 = S.search_canonical(q2, x2, k)
    ix = _index(d, x2)
    _all_modes(ix, q2, k, so2, io2, tag + " query")
    s, i = ix.search(q2, k)
    assert np.isposinf(s[0]).all() and np.array_equal(i[0], np.nonzero(x2[:, col] > 0)[0][:k])     # the mass tie at +inf, by row ascending


@pytest.mark.parametrize("n,d,nq,k", [(700, 64, 4, 20), (30000, 384, 4, 20)])
def test_rows_and_queries_with_inf_and_nan_elements(n, d, nq, k):
    """Single rows with one +inf, one -inf, +inf and -inf (a NaN score), one NaN element, +inf where one query is exactly 0; a query with one +inf element.
    (Fewer than k real scores stays undefined and is not tested.)"""
    _nonfinite_case(n, d, nq, k, f"non-finite {n}x{d}")


def test_rows_and_queries_with_inf_and_nan_elements_through_the_byte_prescan(byte_everywhere):
    _nonfinite_case(30000, 384, 4, 20, "non-finite+byte 30000x384")


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. signed zeros
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 64, 96])
def test_signed_zero_scores_tie_and_resolve_by_row(k):
    """Scores -0, +0, +0, -0, ...: one score.  Rows in plain ascending order in every mode; the zeros by value."""
    q, x = M.signed_zero_corpus()
    so, io = S.search_canonical(q, x, k)
    assert np.array_equal(io, np.tile(np.arange(k), (2, 1)))
    ix = _index(64, x)
    for mode in (0, 1, 2):
        s, i = ix.search(q, k, mode=mode)
        assert np.array_equal(i, io), (mode, i[0, :12])
        assert (s == 0).all() and np.array_equal(s, so)                   # ==: -0.0 equals +0.0


def test_signed_zero_shard_lists_through_both_merges():
    """The signed-zero corpus as two shards: the shards' own lists through kr_topk_merge and kr_topk_merge_device against S.merge_shards and the unsharded
    oracle; every output slot of the device merge is written (the output is pre-filled with a sentinel)."""
    import torch
    from kirag_amd import _lib
    lib = _lib.load()
    q, x = M.signed_zero_corpus()
    k, cut, nq = 10, 40, 2
    so, io = S.search_canonical(q, x, k)
    parts = [(_index(64, x[:cut]).search(q, k), 0), (_index(64, x[cut:]).search(q, k), cut)]
    sc = np.ascontiguousarray(np.stack([p[0][0] for p in parts])); ids = np.ascontiguousarray(np.stack([p[0][1] + p[1] for p in parts]))
    oa, ob = S.search_canonical(q, x[:cut], k), S.search_canonical(q, x[cut:], k)
    want_s, want_i = S.merge_shards([oa[0], ob[0]], [oa[1], ob[1] + cut], k)
    assert np.array_equal(want_i, io)
    ms = np.full((nq, k), np.nan, np.float32); mi = np.full((nq, k), -777, np.int64)
    _lib.check(lib.kr_topk_merge(sc.ctypes.data, ids.ctypes.data, 2, nq, k, ms.ctypes.data, mi.ctypes.data))
    assert np.array_equal(mi, want_i) and np.array_equal(ms, want_s)      # by value
    dsc, dids = torch.from_numpy(sc).cuda(), torch.from_numpy(ids).cuda()
    os_ = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda"); oi = torch.full((nq, k), -777, dtype=torch.int64, device="cuda")
    _lib.check(lib.kr_topk_merge_device(dsc.data_ptr(), nq * k, dids.data_ptr(), nq * k, 2, nq, k, os_.data_ptr(), oi.data_ptr(), 0, None))
    torch.cuda.synchronize()
    got_i, got_s = oi.cpu().numpy(), os_.cpu().numpy()
    assert not (got_i == -777).any() and not np.isnan(got_s).any(), got_i   # every slot written
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. split form: the error bound travels in the exchanged block
# ---------------------------------------------------------------------------------------------------------------------------------------
def _split_search(x, cuts, q, k):
    """two row shards in one process: coarse half -> gather by hand -> global theta -> re-rank half -> finish -> kr_topk_merge"""
    import torch
    from kirag_amd import _lib
    from kirag_amd.retriever.index import FlatIPIndex
    nq, d = q.shape
    shards = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ix = FlatIPIndex(d, device=0); ix.add(torch.from_numpy(x[a:b]).cuda()); shards.append((ix, a))
    qd = torch.from_numpy(q).cuda()
    tks = [torch.empty((nq, k + 1), dtype=torch.float32, device="cuda") for _ in shards]
    for (ix, a), tk in zip(shards, tks):
        ix.search_coarse_async(qd, k, tk)
    gathered = torch.cat(tks[::-1], dim=0).contiguous()
    outs = []
    for ix, a in shards:
        theta = torch.empty((nq,), dtype=torch.float32, device="cuda")
        sc = torch.empty((nq, k), dtype=torch.float32, device="cuda"); rw = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        ix.search_global_theta(gathered, len(shards), theta)
        ix.search_rerank_async(theta, sc, rw)
        ix.finish()
        r = rw.cpu().numpy()
        outs.append((sc.cpu().numpy(), np.where(r >= 0, r + a, -1)))
    sc_all = np.ascontiguousarray(np.stack([o[0] for o in outs])); id_all = np.ascontiguousarray(np.stack([o[1] for o in outs]))
    ms = np.empty((nq, k), np.float32); mi = np.empty((nq, k), np.int64)
    _lib.check(_lib.load().kr_topk_merge(sc_all.ctypes.data, id_all.ctypes.data, len(shards), nq, k, ms.ctypes.data, mi.ctypes.data))
    return ms, mi


@pytest.mark.parametrize("eq,ex", [(-77, 0), (0, -77)])
def test_split_search_of_the_scaled_cluster_two_uneven_shards(eq, ex):
    """kr_index_search_coarse_async / global_theta / rerank_async on the scaled cluster: an understated eps travels in the exchanged block and raises theta."""
    n, d, nq, k = M.CLUSTER_SHAPES[0]
    q, x = _cluster(n, d, nq)
    qs, xs = M.scaled(q, x, eq, ex)
    so, io = _cluster_oracle(n, d, nq, k, eq, ex)
    ms, mi = _split_search(xs, [0, 1100, n], qs, k)
    _same(ms, mi, so, io, f"split q 2^{eq} x 2^{ex}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# F. kr_score_topk (the exact scan alone)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _score_topk(q, x, k):
    from kirag_amd import _lib
    q = np.ascontiguousarray(q, np.float32); x = np.ascontiguousarray(x, np.float32)
    sc = np.empty((len(q), k), np.float32); rows = np.empty((len(q), k), np.int64)
    _lib.check(_lib.load().kr_score_topk(q.ctypes.data, len(q), x.ctypes.data, len(x), q.shape[1], k, sc.ctypes.data, rows.ctypes.data, 0, None))
    return sc, rows


@pytest.mark.parametrize("eq,ex", [(-77, 0), (60, 60)])
def test_score_topk_scaled_cluster(eq, ex):
    q, x = M.dense_cluster(700, 128, 2, seed=828)
    qs, xs = M.scaled(q, x, eq, ex)
    so, io = S.search_canonical(qs, xs, 20)
    s, i = _score_topk(qs, xs, 20)
    _same(s, i, so, io, f"score_topk q 2^{eq} x 2^{ex}")


def test_score_topk_signed_zero_corpus():
    q, x = M.signed_zero_corpus()
    so, io = S.search_canonical(q, x, 20)
    s, i = _score_topk(q, x, 20)
    assert np.array_equal(i, io) and np.array_equal(s, so)               # rows ascending; zeros by value
