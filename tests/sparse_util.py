"""Shared pieces of the sparse-retrieval tests (tests/test_sparse_host.py, tests/test_gpu_sparse.py): the reference — numpy float32, restating the result
definition of include/kirag_sparse.h literally (ascending terms, one ``np.float32`` multiply then one add, ``lexsort`` by (-score, row) over the rows with
s > 0), whole or with ONE part broken (the teeth) —, the float64 sum with its a-priori bound, generators, and the ctypes calls of ``ks_search`` /
``ks_count_positive`` / ``ks_compact_rows`` with guard words around the outputs."""
import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)
GUARD = 64                            # guard elements on either side of an output
GUARD_F32, GUARD_I64, GUARD_I32, GUARD_U16 = np.float32(-12345.5), np.int64(-0x0123456789ABCDEF), np.int32(-0x1234567), np.uint16(0xBEEF)
MUTATIONS = ("descending_terms", "fused_multiply_add", "float32_weights")
VOCABS = (97, 1031, 30522)
QUERY_TERMS = (1, 2, 33, 200)
KS = (1, 10, 100, 1024)


class Corpus:
    """a forward CSR over V terms: ``row_off`` int64, ``terms`` int32 ascending within a row, ``w32`` the float32 weights before rounding and ``w16`` after"""

    def __init__(self, V, row_off, terms, w32):
        self.V, self.row_off, self.terms = int(V), np.asarray(row_off, np.int64), np.asarray(terms, np.int32)
        self.w32 = np.asarray(w32, np.float32)
        self.w16 = self.w32.astype(np.float16)
        self.N = len(self.row_off) - 1
        self._by_term = None

    def row(self, r):
        a, b = self.row_off[r], self.row_off[r + 1]
        return self.terms[a:b], self.w16[a:b]

    def pairs(self, r0=0, r1=None):
        """the rows as (terms, weights) pairs, the form SparseIndexer.index_data takes"""
        return [self.row(r) for r in range(r0, self.N if r1 is None else r1)]

    def by_term(self):
        """entries sorted by term (the test's own lookup, a plain sort): (term starts [V + 1], row of entry, position of entry)"""
        if self._by_term is None:
            rows = np.repeat(np.arange(self.N, dtype=np.int64), np.diff(self.row_off))
            order = np.argsort(self.terms, kind="stable")
            starts = np.zeros(self.V + 1, np.int64)
            np.cumsum(np.bincount(self.terms, minlength=self.V), out=starts[1:])
            self._by_term = (starts, rows[order], order)
        return self._by_term


def ref_scores(c, q_term, q_w, broken=None):
    """float32 [N]: s = 0; for the query's terms in ascending order: s = fl32(s + fl32(q * float(d))) on the rows that hold the term"""
    starts, rows, pos = c.by_term()
    q_term, q_w = np.asarray(q_term, np.int64), np.asarray(q_w, np.float32)
    order = np.argsort(q_term)
    if broken == "descending_terms":
        order = order[::-1]
    d_all = c.w32 if broken == "float32_weights" else c.w16.astype(np.float32)
    s = np.zeros(c.N, np.float32)
    for i in order:
        a, b = starts[q_term[i]], starts[q_term[i] + 1]
        r, d = rows[a:b], d_all[pos[a:b]]
        if broken == "fused_multiply_add":
            s[r] = (s[r].astype(np.float64) + np.float64(q_w[i]) * d.astype(np.float64)).astype(np.float32)      # the product is exact in float64
        else:
            s[r] = (s[r] + (q_w[i] * d).astype(np.float32)).astype(np.float32)
    return s


def ranking(s):
    """the rows with s > 0 by (score descending, row ascending)"""
    pos = np.flatnonzero(s > 0)
    return pos[np.lexsort((pos, -s[pos].astype(np.float64)))]


def ref_search(c, q_term, q_w, k, broken=None):
    """(scores fp32 [k], rows int64 [k]) as ks_search leaves them: missing places hold row -1 and +0.0"""
    s = ref_scores(c, q_term, q_w, broken)
    top = ranking(s)[:k]
    scores, rows = np.zeros(k, np.float32), np.full(k, -1, np.int64)
    scores[:len(top)], rows[:len(top)] = s[top], top
    return scores, rows


def scores64(c, q_term, q_w):
    """(float64 sum of q * d per row, the a-priori bound gamma_m * that sum, m = the query's term count): weights are positive, so the sum is its own sum of
    absolute values and the standard inner-product bound |fl(x . y) - x . y| <= gamma_m |x| . |y| applies to the float32 loop in any order"""
    starts, rows, pos = c.by_term()
    s = np.zeros(c.N, np.float64)
    for t, w in zip(np.asarray(q_term, np.int64), np.asarray(q_w, np.float64)):
        a, b = starts[t], starts[t + 1]
        s[rows[a:b]] += w * c.w16[pos[a:b]].astype(np.float64)
    m = max(len(q_term), 1)
    return s, m * U32 / (1 - m * U32) * s


# ---- generators ----
def random_corpus(V, N, seed, lo=1, hi=40):
    """N rows of ``lo .. hi`` candidate terms each (duplicates merged, so a row holds 1 .. hi terms), small term ids more frequent (u^2), float32 weights in
    [0.05, 3): after float16 rounding >= 2^-10, so with query weights >= 0.1 no product or sum is subnormal"""
    rng = np.random.default_rng(seed)
    hi = min(hi, V)
    count = rng.integers(lo, hi + 1, N)
    cand = np.minimum((V * rng.random((N, hi)) ** 2).astype(np.int64), V - 1)
    use = np.arange(hi)[None, :] < count[:, None]
    key = np.unique((np.arange(N, dtype=np.int64)[:, None] * V + cand)[use])            # sorted: ascending row, ascending term within a row
    rows, terms = key // V, key % V
    row_off = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=row_off[1:])
    return Corpus(V, row_off, terms, rng.uniform(0.05, 3.0, len(terms)).astype(np.float32))


def random_query(V, m, seed):
    """min(m, V) distinct terms, ascending, small ids more frequent; float32 weights in [0.1, 2)"""
    rng = np.random.default_rng(seed)
    m = min(m, V)
    t = np.unique(np.minimum((V * rng.random(4 * m) ** 2).astype(np.int64), V - 1))
    if len(t) < m:
        t = np.union1d(t, rng.permutation(np.setdiff1d(np.arange(V), t))[:m - len(t)])
    t = np.sort(rng.permutation(t)[:m])
    return t.astype(np.int32), rng.uniform(0.1, 2.0, m).astype(np.float32)


def csr(queries):
    """a list of (terms, weights) as ks_search's host CSR"""
    off = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(t) for t, _ in queries], out=off[1:])
    term = np.concatenate([np.asarray(t, np.int32) for t, _ in queries] + [np.empty(0, np.int32)])
    w = np.concatenate([np.asarray(x, np.float32) for _, x in queries] + [np.empty(0, np.float32)])
    return off, np.ascontiguousarray(term), np.ascontiguousarray(w)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the library, called directly ----
def run_search(lib, ix, queries, k, device=0):
    """``ks_search`` over the arrays of a SparseIndexer on the GPU; returns (rc, scores fp32 [nq, k], rows int64 [nq, k], guards untouched?)"""
    import torch
    dev = torch.device("cuda", device)
    q_off, q_term, q_w = csr(queries)
    nq = len(queries)
    post_off = ix._sync_tail()
    n = nq * k
    out_s = torch.full((n + 2 * GUARD,), float(GUARD_F32), dtype=torch.float32, device=dev)
    out_r = torch.full((n + 2 * GUARD,), int(GUARD_I64), dtype=torch.int64, device=dev)
    rc = lib.ks_search(ix._post.data_ptr(), ix._ptr.data_ptr(), post_off.ctypes.data, ix.ntotal, ix.vocab_size, q_off.ctypes.data, nq, q_term.ctypes.data,
                       q_w.ctypes.data, k, out_s[GUARD:].data_ptr(), out_r[GUARD:].data_ptr(), device, int(torch.cuda.current_stream(dev).cuda_stream))
    s, r = out_s.cpu().numpy(), out_r.cpu().numpy()
    intact = bool((s[:GUARD] == GUARD_F32).all() and (s[GUARD + n:] == GUARD_F32).all() and (r[:GUARD] == GUARD_I64).all() and (r[GUARD + n:] == GUARD_I64).all())
    return rc, s[GUARD:GUARD + n].reshape(nq, k).copy(), r[GUARD:GUARD + n].reshape(nq, k).copy(), intact


def torch_compact(block, skip=()):
    """the rule of ks_compact_rows in torch on the CPU: (counts int64 [B], terms int32, weight bits uint16); None when a value does not stay finite"""
    import torch
    h = torch.as_tensor(np.asarray(block, np.float32)).to(torch.float16)
    if not bool(torch.isfinite(h).all()):
        return None
    keep = h > 0
    for s in skip:
        keep[:, int(s)] = False
    return keep.sum(1).numpy().astype(np.int64), torch.nonzero(keep)[:, 1].numpy().astype(np.int32), h[keep].view(torch.int16).numpy().view(np.uint16)


def run_compact(lib, block, skip=(), row_off=None, device=0):
    """``ks_count_positive`` then ``ks_compact_rows`` on a float32 array [B, V]; ``row_off``: given instead of the one the counts give.  Returns
    (rc of the count, counts, rc of the compaction, terms int32, weight bits uint16, guards untouched?)"""
    import torch
    dev = torch.device("cuda", device)
    block = np.ascontiguousarray(block, np.float32)
    B, V = block.shape
    bd = torch.from_numpy(block).to(dev)
    sk = np.ascontiguousarray(sorted(skip), dtype=np.int32)
    counts = np.full(B, -7, np.int64)
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    rc1 = lib.ks_count_positive(bd.data_ptr(), B, V, sk.ctypes.data, len(sk), counts.ctypes.data, device, stream)
    if row_off is None:
        if rc1 != 0:
            return rc1, counts, None, None, None, True
        row_off = np.zeros(B + 1, np.int64)
        np.cumsum(counts, out=row_off[1:])
    row_off = np.ascontiguousarray(row_off, np.int64)
    n = int(row_off[-1])
    t = torch.full((n + 2 * GUARD,), int(GUARD_I32), dtype=torch.int32, device=dev)
    w = torch.full((n + 2 * GUARD,), int(np.uint16(GUARD_U16).view(np.int16)), dtype=torch.int16, device=dev)
    rc2 = lib.ks_compact_rows(bd.data_ptr(), B, V, sk.ctypes.data, len(sk), row_off.ctypes.data, t[GUARD:].data_ptr(), w[GUARD:].data_ptr(), device, stream)
    tn, wn = t.cpu().numpy(), w.cpu().numpy().view(np.uint16)
    intact = bool((tn[:GUARD] == GUARD_I32).all() and (tn[GUARD + n:] == GUARD_I32).all() and (wn[:GUARD] == GUARD_U16).all() and (wn[GUARD + n:] == GUARD_U16).all())
    return rc1, counts, rc2, tn[GUARD:GUARD + n].copy(), wn[GUARD:GUARD + n].copy(), intact
