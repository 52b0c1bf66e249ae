"""Preconditions of tests/test_gpu_search_magnitudes.py, asserted with the oracle alone (no GPU): what gives those tests their teeth.

  * the cluster corpora really are below the 16-bit resolution: for every query at least half of the exact top-k is missing from the top-k of the
    bf16 / f16 rounded inputs, so a search that trusts its 16-bit ranking returns a visibly wrong answer;
  * the canonical search commutes with scaling by powers of two wherever no score is subnormal or overflows: the scaled cases ask the same
    question as the unit-scale one, and the oracle itself is sound far from the unit sphere;
  * in every non-finite case each query keeps at least k rows with a real score (fewer is undefined and the oracle refuses it);
  * the signed-zero corpus separates the two candidate orders: the oracle's (zeros tie, row ascending) differs from "+0 above -0"."""
import os
import sys

import numpy as np
import pytest

from oracle import search_np as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magnitude_util as M  # noqa: E402


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n,d,nq,k", M.CLUSTER_SHAPES + [(3000, 64, 6, 20)])
def test_cluster_is_below_the_16_bit_resolution(n, d, nq, k, dtype):
    q, x = M.dense_cluster(n, d, nq, seed=n + d)
    _, io = S.search_canonical(q, x, k)
    miss = M.missing_from(io, M.coarse_topk_emulated(q, x, k, dtype))
    print(f"[cluster {n}x{d} nq {nq} k {k} {dtype}] rows of the exact top-k missing from the 16-bit top-k, per query: {miss.tolist()}")
    # At least half of the exact top-k, for every query.  The exception is f16 at the two k = 50 shapes: its 11-bit significand leaves the ranking about half
    # right there (weakest query of (3000, 256) over seeds 0..39: 17 to 24 missing of 50, never 25; (40000, 384): 20 of 50), so "half" cannot be asked of
    # every query whatever the seed.  A third is asked instead: what the GPU tests need is that the 16-bit ranking is wrong by MANY rows for every query,
    # so that a search which trusts it cannot pass.
    need = k / 3 if (dtype == "f16" and k == 50) else k / 2
    assert (miss >= need).all(), miss
    # scaling by powers of two changes nothing about that (bf16 shares fp32's exponent range; f16 only while nothing leaves its range)
    if dtype == "bf16":
        qs, xs = M.scaled(q, x, -77, 0)
        assert M.scaling_is_exact(q, qs, -77)
        assert np.array_equal(M.coarse_topk_emulated(qs, xs, k, dtype), M.coarse_topk_emulated(q, x, k, dtype))


@pytest.mark.parametrize("eq,ex", [(-100, 0), (0, -100), (-77, 0), (0, -77), (60, 0), (0, 60), (-40, -40), (60, 60)])
def test_canonical_search_commutes_with_power_of_two_scaling(eq, ex):
    n, d, nq, k = M.CLUSTER_SHAPES[0]
    q, x = M.dense_cluster(n, d, nq, seed=n + d)
    so, io = S.search_canonical(q, x, k)
    qs, xs = M.scaled(q, x, eq, ex)
    assert M.scaling_is_exact(q, qs, eq) and M.scaling_is_exact(x, xs, ex)
    ss, is_ = S.search_canonical(qs, xs, k)
    assert M.scores_normal(S.scores_all(qs, xs))                      # no score of ANY row is subnormal or overflows
    assert np.array_equal(is_, io)
    assert np.array_equal(ss.view(np.uint32), np.ldexp(so, eq + ex).astype(np.float32).view(np.uint32))


def test_overflowing_scores_tie_at_inf_by_row():
    n, d, nq, k = M.CLUSTER_SHAPES[0]
    q, x = M.dense_cluster(n, d, nq, seed=n + d)
    ss, _ = S.search_canonical(*M.scaled(q, x, 64, 64), k)
    assert np.isfinite(ss).all() and (ss > 3.3e38).all()              # cosines ~0.98: 0.98 x 2^128 stays just below FLT_MAX
    ss, is_ = S.search_canonical(*M.scaled(q, x, 64, 65), k)
    assert np.isposinf(ss).all() and np.array_equal(is_, np.tile(np.arange(k), (nq, 1)))


@pytest.mark.parametrize("n,d,nq,k", [(700, 64, 4, 20), (30000, 384, 4, 20)])
def test_non_finite_cases_keep_k_real_scores(n, d, nq, k):
    q, x, rows = M.nonfinite_rows(n, d, nq, seed=n + d)
    sc = S.scores_all(q, x)
    assert ((~np.isnan(sc)).sum(axis=1) >= k).all()
    so, io = S.search_canonical(q, x, k)                              # returns (0), does not refuse (-2)
    assert np.isnan(sc[:, rows["both_inf"]]).all() and np.isnan(sc[:, rows["one_nan"]]).all()
    assert np.isnan(sc[0, rows["inf_at_zero_of_q0"]]) and np.isinf(sc[1:, rows["inf_at_zero_of_q0"]]).all()
    assert np.isinf(sc[:, rows["pos_inf"]]).all() and np.isinf(sc[:, rows["neg_inf"]]).all()
    for r in ("both_inf", "one_nan"):
        assert not (io == rows[r]).any()
    assert not (io[0] == rows["inf_at_zero_of_q0"]).any()
    assert np.isposinf(so[:, 0]).all()                                # every query has a +inf row on top (the sign of its element decides which)
    # the query with an inf element: +inf for the positive column entries (ties by row), NaN rows never, -inf rows last
    q2, x2, col = M.inf_query(n, d, nq, k, seed=n + d + 1)
    sc2 = S.scores_all(q2, x2)
    assert ((~np.isnan(sc2)).sum(axis=1) >= k).all()
    so2, io2 = S.search_canonical(q2, x2, k)
    pos = np.nonzero(x2[:, col] > 0)[0]
    assert np.array_equal(io2[0], pos[:k]) and np.isposinf(so2[0]).all()
    assert np.isfinite(so2[1:]).all()
    n_real = int((~np.isnan(sc2[0])).sum())
    if n_real <= 1024 and n_real <= n:                                # the whole real order where the library can be asked for it
        so_all, io_all = S.search_canonical(q2[:1], x2, n_real)
        npos = len(pos)
        assert np.isposinf(so_all[0, :npos]).all() and np.isneginf(so_all[0, npos:]).all()
        assert not np.isin(io_all[0], np.nonzero(x2[:, col] == 0)[0]).any()


def test_signed_zero_corpus_separates_the_two_orders():
    q, x = M.signed_zero_corpus()
    sc = S.scores_all(q, x)
    assert (sc == 0).all()
    assert np.array_equal(np.signbit(sc[0]), np.arange(96) % 3 == 0) and np.array_equal(np.signbit(sc[1]), np.arange(96) % 3 == 2)
    for k in (10, 64, 96):
        so, io = S.search_canonical(q, x, k)
        assert np.array_equal(io, np.tile(np.arange(k), (2, 1)))       # zeros tie: plain ascending rows
        assert np.array_equal(np.signbit(so), np.signbit(sc[:, :k]))    # the oracle returns the signed zeros as they are
        assert not np.array_equal(M.plus_zero_first_order(sc, k), io)
    # shards: the merge of the oracle's per-shard lists is the oracle's answer
    cut = 40
    parts = [S.search_canonical(q, x[:cut], 10), S.search_canonical(q, x[cut:], 10)]
    ms, mi = S.merge_shards([p[0] for p in parts], [parts[0][1], parts[1][1] + cut], 10)
    assert np.array_equal(mi, np.tile(np.arange(10), (2, 1))) and (ms == 0).all()
