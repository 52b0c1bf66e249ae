"""Shared pieces of the magnitude tests of the search (tests/test_search_magnitudes_host.py, tests/test_gpu_search_magnitudes.py): seeded numpy
builders of corpora and queries far from the unit sphere - the dense cluster below the 16-bit resolution at any power-of-two scale, mixed row norms,
rows and queries with inf / NaN elements, scores that round to signed zeros - and a numpy emulation of the 16-bit top-k that the coarse scan sees.
numpy only; every builder is a pure function of its arguments."""
import numpy as np

from oracle import search_np as S

FLT_MIN = np.float32(1.17549435e-38)

# (query exponent, row exponent): the inputs are multiplied by 2^eq and 2^ex.  Sums of squares in fp32 are subnormal or 0 below 2^-64 (the -64 pairs sit
# on that edge, -77 / -100 / -120 far below it, (-40, -40) has healthy norms whose PRODUCT is small); 2^64 and above overflow them; (64, 64) puts every score of the
# cluster (cosines ~0.98) just below FLT_MAX, (64, 65) overflows every score to +inf: a mass tie that resolves by row ascending.
SCALE_PAIRS = [(-64, 0), (0, -64), (-77, 0), (0, -77), (-40, -40), (-100, 0), (0, -100), (-120, 0), (40, 40), (64, 0), (0, 64), (100, 0), (60, 60), (64, 64),
               (64, 65)]
F16_ONLY_PAIRS = [(0, 20)]            # finite rows whose f16 copy overflows to inf
# (n, d, nq, k) of the cluster cases; the first reaches k_coarse in one direct round, the second k_coarse_q32 in several rounds, the third the 128-query tile
CLUSTER_SHAPES = [(3000, 256, 6, 50), (40000, 384, 6, 50), (40000, 384, 40, 50)]


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dense_cluster(n, d, nq, seed):
    """rows = unit(base + 2e-4 N(0, I)), queries = unit(0.2 unit + base): neighbouring scores are closer together than one bf16 / f16 step, so the 16-bit
    top-k is mostly wrong and only a certificate that REFUSES keeps the answer exact.  Returns (q, x)."""
    rng = np.random.default_rng(seed)
    base = unit(rng, 1, d)
    x = base + 2e-4 * rng.standard_normal((n, d)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = unit(rng, nq, d) * 0.2 + base
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return q, x


def scaled(q, x, eq, ex):
    """(q 2^eq, x 2^ex) in fp32.  Exact unless an element lands in the subnormal range (scaling_is_exact tells)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(q, np.float32), eq).astype(np.float32), np.ldexp(np.asarray(x, np.float32), ex).astype(np.float32)


def scaling_is_exact(a, a_scaled, e):
    """every element of a_scaled is a 2^e exactly (no bits lost to the subnormal range, nothing overflowed)"""
    with np.errstate(over="ignore", under="ignore"):
        return bool(np.array_equal(np.ldexp(a_scaled.astype(np.float64), -e), a.astype(np.float64)))


def scores_normal(s):
    """no score is inf, NaN, zero or subnormal: scaling by a power of two then commutes with the rounding of the canonical score"""
    return bool(np.isfinite(s).all() and (np.abs(s) >= FLT_MIN).all())


def better_order(scores, k):
    """k best columns per row by (score desc, column asc) in fp64 values; NaN never wins.  -0.0 == +0.0 here as in the oracle."""
    sc = np.asarray(scores, np.float64)
    out = np.empty((sc.shape[0], k), np.int64)
    for r in range(sc.shape[0]):
        keep = np.nonzero(~np.isnan(sc[r]))[0]
        order = np.lexsort((keep, -sc[r][keep]))[:k]
        out[r] = keep[order]
    return out


def coarse_topk_emulated(q, x, k, dtype):
    """The top-k a 16-bit scan would see: q and x rounded to bf16 (the oracle's f32_to_bf16_bits) or f16 (numpy), products and sums in fp64,
    (score desc, row asc).  Returns rows [nq, k]."""
    if dtype == "bf16":
        qc = S.bf16_bits_to_f32(S.f32_to_bf16_bits(q)); xc = S.bf16_bits_to_f32(S.f32_to_bf16_bits(x))
    elif dtype == "f16":
        with np.errstate(over="ignore"):
            qc = np.asarray(q, np.float32).astype(np.float16).astype(np.float32); xc = np.asarray(x, np.float32).astype(np.float16).astype(np.float32)
    else:
        raise ValueError(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = qc.astype(np.float64) @ xc.astype(np.float64).T
    return better_order(sc, k)


def missing_from(rows_exact, rows_coarse):
    """per query: how many rows of the exact top-k the coarse top-k does not hold"""
    return np.array([len(set(a.tolist()) - set(b.tolist())) for a, b in zip(rows_exact, rows_coarse)])


# ---- mixed magnitudes in one index ---------------------------------------------------------------------------------------------------------
def queries_near(rng, x, nq):
    """unit queries next to nq rows of x (the direction only: the rows may have any norm)"""
    pick = rng.choice(len(x), nq, replace=False)
    xd = x[pick].astype(np.float64); xd /= np.linalg.norm(xd, axis=1, keepdims=True)
    q = xd + 0.05 * rng.standard_normal(xd.shape) / np.sqrt(x.shape[1]) * 8
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def mixed_norms(n, d, nq, seed):
    """unit directions times norms log-uniform in [2^-10, 2^10].  Returns (q, x, norms)."""
    rng = np.random.default_rng(seed)
    x = unit(rng, n, d)
    norms = np.exp2(rng.uniform(-10.0, 10.0, n)).astype(np.float32)
    x = (x * norms[:, None]).astype(np.float32)
    return queries_near(rng, x, nq), x, norms


def two_outlier_norms(n, d, nq, seed):
    """a unit corpus with one row of norm 2^40 and one of norm 2^-40 (exact scalings of unit rows).  Returns (q, x, (big, small))."""
    rng = np.random.default_rng(seed)
    x = unit(rng, n, d)
    big, small = n // 3, 2 * n // 3 + 1
    x[big] = np.ldexp(x[big], 40); x[small] = np.ldexp(x[small], -40)
    q = queries_near(rng, x, nq)
    return q, x, (big, small)


# ---- non-finite elements -------------------------------------------------------------------------------------------------------------------
def nonfinite_rows(n, d, nq, seed):
    """A unit corpus in which five single rows hold: one +inf element; one -inf element; +inf and -inf together; one NaN element; one +inf element in a
    column where query 0 is exactly 0 (NaN for that query only).  Returns (q, x, rows) with rows = {name: row number}."""
    rng = np.random.default_rng(seed)
    x = unit(rng, n, d)
    q = unit(rng, nq, d)
    rows = {"pos_inf": n // 7, "neg_inf": n // 5, "both_inf": n // 3, "one_nan": n // 2, "inf_at_zero_of_q0": n - 3}
    col0 = 5
    q[0, col0] = 0.0
    x[rows["pos_inf"], 1] = np.inf
    x[rows["neg_inf"], 2] = -np.inf
    x[rows["both_inf"], 3] = np.inf; x[rows["both_inf"], 4] = -np.inf
    q[:, 3:5] = np.abs(q[:, 3:5])                                            # both products are then infinite with opposite signs: NaN for every query
    x[rows["one_nan"], 7] = np.nan
    x[rows["inf_at_zero_of_q0"], col0] = np.inf
    return q.astype(np.float32), x.astype(np.float32), rows


def inf_query(n, d, nq, k, seed):
    """Query 0 has one +inf element; the corpus column there has at least k positive entries, negative entries and exact zeros: scores +inf (a mass tie, by row
    ascending), -inf, and NaN (0 x inf: never returned).  The other queries are finite.  Returns (q, x, col)."""
    rng = np.random.default_rng(seed)
    x = unit(rng, n, d)
    q = unit(rng, nq, d)
    col = 9
    q[0, col] = np.inf
    zero = rng.choice(n, n // 3, replace=False)
    x[zero, col] = 0.0
    assert (x[:, col] > 0).sum() >= k and (x[:, col] < 0).any() and (x[:, col] == 0).any()
    return q.astype(np.float32), x.astype(np.float32), col


# ---- signed zeros --------------------------------------------------------------------------------------------------------------------------
def signed_zero_corpus(n=96, d=64):
    """q = (2^-100 e_0, -2^-100 e_0); row r has first column (-1, 0, +1)[r % 3] * 2^-100 * c_r with c_r = 1 + (r // 3) / 64, all other columns zero.  Every exact
    product is 0 or +-2^-200 c: the canonical scores are -0, +0, +0, ... for query 0 and +0, +0, -0, ... for query 1.  Returns (q, x)."""
    x = np.zeros((n, d), np.float32)
    r = np.arange(n)
    c = (1.0 + (r // 3) / 64.0).astype(np.float32)
    x[:, 0] = np.ldexp(np.array([-1.0, 0.0, 1.0], np.float32)[r % 3] * c, -100)
    q = np.zeros((2, d), np.float32)
    q[0, 0] = np.ldexp(np.float32(1.0), -100); q[1, 0] = -q[0, 0]
    return q, x


def plus_zero_first_order(scores, k):
    """the order a key that ranks +0.0 above -0.0 produces: (score desc with -0 < +0, row asc)"""
    s = np.asarray(scores, np.float32)
    out = np.empty((s.shape[0], k), np.int64)
    for r in range(s.shape[0]):
        neg0 = (s[r] == 0) & np.signbit(s[r])
        order = np.lexsort((np.arange(s.shape[1]), neg0.astype(np.int64), -s[r].astype(np.float64)))[:k]
        out[r] = order
    return out
