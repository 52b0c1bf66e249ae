"""Shared pieces of the late-interaction tests (tests/test_late_host.py, tests/test_gpu_late.py): the float64 MaxSim reference on the float16-rounded operands
— whole, or with ONE part broken (the teeth) —, the derived error bounds, generators for integer-exact operands and for cases in which one token decides the
score, and the ctypes call of ``kl_maxsim`` / ``kl_gather_rows_f16`` with guard words around the outputs."""
import numpy as np

SCORE_BAR = 1e-3                      # the project's score tolerance (tests/m3_util.py)
DIMS = (32, 96, 128, 256, 1024)
Q_ROWS = (1, 5, 32, 33, 70)
D_ROWS = (0, 1, 31, 32, 33, 64, 65, 200)
MUTATIONS = ("sum_for_mean", "mean_over_doc_tokens", "drop_last_doc_token", "admit_padding_row", "count_padded_query_rows")
U32, U16 = 2.0 ** -24, 2.0 ** -11     # unit roundoffs of fp32 and float16 (round to nearest)
GUARD = 64                            # guard elements on either side of an output
GUARD_F32, GUARD_U16 = np.float32(-12345.5), np.uint16(0xBEEF)


def f16(a):
    """float16 rounding (nearest even) of float32 rows, as float16"""
    return np.asarray(a, np.float32).astype(np.float16)


def ref_maxsim(q, d, reduce="mean", broken=None):
    """float64 ``sum_i max_j q_i . d_j`` (``reduce="mean"``: over the query's rows) of ONE pair, on the operands as given (the caller rounds them); a query or
    a document without rows scores 0.  ``broken``: one of MUTATIONS."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    if broken == "drop_last_doc_token":
        d = d[:-1]
    if broken == "admit_padding_row":
        d = np.concatenate((d, np.zeros((1, d.shape[1]))))
    if q.shape[0] == 0 or d.shape[0] == 0:
        return 0.0
    s = q @ d.T
    per_row = s.mean(axis=1) if broken == "mean_over_doc_tokens" else s.max(axis=1)
    total = per_row.sum()
    if broken == "sum_for_mean":
        reduce = "sum" if reduce == "mean" else "mean"
    n = q.shape[0]
    if broken == "count_padded_query_rows":
        n = -(-n // 32) * 32         # the zero rows that fill the last 32-row tile each add max_j 0 = 0 and count
    return total / n if reduce == "mean" else total


def kernel_bound(q, d, reduce="mean"):
    """Bound of |kernel - ref_maxsim| on the SAME float16 operands, derived from the kernel's rounding points (the method of proj_probe_util.error_bound):
         a product of two float16 values has 22 significant bits: exact in fp32
         fp32 accumulation over P in an order the MFMA does not specify: at most one rounding per product, gamma_P sum_k |q_ik d_jk|
         the max over j picks a value, no rounding: |max_j a_j - max_j b_j| <= max_j |a_j - b_j|
         the fp32 sum over the n query rows: gamma_n sum_i (|m_i| + e_i)
         the mean: one correctly rounded division
       Never tuned to a measurement."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    n, P = q.shape
    if n == 0 or d.shape[0] == 0:
        return 0.0
    gp, gn = P * U32 / (1 - P * U32), n * U32 / (1 - n * U32)
    e = gp * (np.abs(q) @ np.abs(d).T).max(axis=1)
    m = np.abs((q @ d.T).max(axis=1))
    b = e.sum() + gn * (m + e).sum()
    if reduce == "mean":
        b = b / n + U32 * (abs(ref_maxsim(q, d, "mean")) + b / n)
    return float(b)


def rounding_bound(q, d):
    """Bound of |ref_maxsim(f16(q), f16(d), "mean") - ref_maxsim(q, d, "mean")| for UNROUNDED float32 rows: every element x becomes x (1 + delta) + eta with
    |delta| <= 2^-11 and |eta| <= 2^-25 (eta only in float16's subnormal range), so
         |q^_k d^_k - q_k d_k| <= (2 2^-11 + 2^-22) |q_k d_k| + 2^-25 (1 + 2^-11) (|q_k| + |d_k|) + 2^-50
    summed over k, the max over j of that for every query row (a max moves by no more than its entries), the mean over the rows.  For rows of norm <= 1 the
    first term is at most 2 2^-11 (1 + 2^-11) by Cauchy-Schwarz."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    P = q.shape[1]
    a = 2 * U16 * (1 + U16) * (np.abs(q) @ np.abs(d).T)
    sub = 2.0 ** -25 * (1 + U16) * (np.abs(q).sum(1)[:, None] + np.abs(d).sum(1)[None, :]) + P * 2.0 ** -50
    return float((a + sub).max(axis=1).mean())


# ---- generators ----
def exact_rows(n, P, seed):
    """n rows of small integers times 2^-2 (float16): every product is an integer times 2^-4 below 2^4 and every fp32 sum over P <= 1024 elements and over
    <= 70 rows an integer times 2^-4 below 2^24 2^-4 — exact whatever the order.  A few columns carry larger values so that the row maxima differ."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, size=(n, P)).astype(np.float32)
    a[:, : min(P, 8)] = rng.integers(-7, 8, size=(n, min(P, 8)))
    return (a * 0.25).astype(np.float16)


def unit_rows(n, P, seed):
    """n float32 rows of norm 1 (normal directions)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, P))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def decisive_doc(P, nq, nd, row, seed, negative=False):
    """(q, d) float16: every query row is close to one direction c; the document's rows are random directions except row ``row``, the only one near c — the
    max of EVERY query row sits there, so dropping it moves a mean by about 0.8.  ``negative``: every document row is near -c (all products negative, about
    -0.9) and row ``row`` is the least negative (about -0.2): a zero padding row would beat them all."""
    rng = np.random.default_rng(seed)
    c = _unit(rng.standard_normal(P))
    q = _unit(c + 0.3 * _unit(rng.standard_normal((nq, P))))
    if negative:
        d = _unit(-c + 0.3 * _unit(rng.standard_normal((nd, P))))
        d[row] = -0.2 * c           # q_i . c > 0 for every row, so this one stays negative too
    else:
        d = _unit(rng.standard_normal((nd, P)))
        d[row] = c
    return f16(q), f16(d)


def decisive_query(P, nq, nd, row, seed):
    """(q, d) float16: random directions, except that query row ``row`` equals document row 0 (its max is 1, the other rows' about 3 / sqrt(P) .. 0.6):
    leaving that row out of the sum moves ``reduce="sum"`` by about 1."""
    rng = np.random.default_rng(seed)
    q, d = _unit(rng.standard_normal((nq, P))), _unit(rng.standard_normal((nd, P)))
    q[row] = d[0]
    return f16(q), f16(d)


# ---- the library, called directly ----
def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if np.asarray(a).dtype == np.float16 else np.uint32)


def offsets(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off


def run_maxsim(lib, queries, docs, pair_q, pair_d, P, reduce, device=0):
    """``kl_maxsim`` on lists of float16 arrays; returns (rc, fp32 scores [npairs], guards untouched?)"""
    import torch
    cat = lambda rows: np.concatenate([np.asarray(r, np.float16).reshape(-1, P) for r in rows] + [np.empty((0, P), np.float16)])
    dev = torch.device("cuda", device)
    qd, dd = torch.from_numpy(cat(queries)).to(dev), torch.from_numpy(cat(docs)).to(dev)
    q_off, d_off = offsets(queries), offsets(docs)
    pq, pd = np.ascontiguousarray(pair_q, dtype=np.int64), np.ascontiguousarray(pair_d, dtype=np.int64)
    n = len(pq)
    out = torch.full((n + 2 * GUARD,), float(GUARD_F32), dtype=torch.float32, device=dev)
    rc = lib.kl_maxsim(qd.data_ptr(), q_off.ctypes.data, len(queries), dd.data_ptr(), d_off.ctypes.data, len(docs), pq.ctypes.data, pd.ctypes.data, n, P,
                       {"sum": 0, "mean": 1}[reduce], out[GUARD:].data_ptr(), device, int(torch.cuda.current_stream(dev).cuda_stream))
    res = out.cpu().numpy()
    intact = bool((res[:GUARD] == GUARD_F32).all() and (res[GUARD + n:] == GUARD_F32).all())
    return rc, res[GUARD:GUARD + n].copy(), intact


def run_gather(lib, block, src_row, device=0):
    """``kl_gather_rows_f16`` on a float32 array [R, P]; returns (rc, uint16 bits [T, P], guards untouched?)"""
    import torch
    dev = torch.device("cuda", device)
    block = np.ascontiguousarray(block, np.float32)
    P = block.shape[1]
    src = np.ascontiguousarray(src_row, dtype=np.int64)
    T = len(src)
    bd = torch.from_numpy(block).to(dev)
    out = torch.full((T * P + 2 * GUARD,), int(np.int16(np.uint16(GUARD_U16).view(np.int16))), dtype=torch.int16, device=dev)
    rc = lib.kl_gather_rows_f16(bd.data_ptr(), src.ctypes.data, T, P, out[GUARD:].data_ptr(), device, int(torch.cuda.current_stream(dev).cuda_stream))
    res = out.cpu().numpy().view(np.uint16)
    intact = bool((res[:GUARD] == GUARD_U16).all() and (res[GUARD + T * P:] == GUARD_U16).all())
    return rc, res[GUARD:GUARD + T * P].reshape(T, P).copy(), intact
