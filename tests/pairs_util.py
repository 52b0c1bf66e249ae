"""Shared pieces of the pair-scoring tests (tests/test_pairs_host.py, tests/test_gpu_pairs.py): the ctypes call of ``kp_sparse_dot`` with guard words around
``out``, and the pair reference.  The reference is NOT a second statement of the result definition: ``sparse_util.ref_scores`` gives the score of every row
of a corpus for one query — whole, or under one of its ``MUTATIONS`` — and a pair's score is that array at the pair's row."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_util as U  # noqa: E402

EXPORTS = {"kp_abi_version", "kp_last_error", "kp_release_scratch", "kp_sparse_dot"}
POS_ZERO = np.uint32(0)               # the bit pattern of +0.0


def ref_pairs(c, queries, pair_q, pair_row, broken=None):
    """float32 [npairs]: ``sparse_util.ref_scores`` of each query over corpus ``c``, read at the pairs' rows"""
    pair_q, pair_row = np.asarray(pair_q, np.int64), np.asarray(pair_row, np.int64)
    out = np.zeros(len(pair_q), np.float32)
    for q in np.unique(pair_q):
        t, w = queries[q]
        s = U.ref_scores(c, t, w, broken) if len(t) else np.zeros(c.N, np.float32)
        sel = pair_q == q
        out[sel] = s[pair_row[sel]]
    return out


def all_pairs(nq, N):
    """every (query, row) pair, query-major"""
    return np.repeat(np.arange(nq, dtype=np.int64), N), np.tile(np.arange(N, dtype=np.int64), nq)


def corpus_of(V, rows):
    """a ``sparse_util.Corpus`` from a list of (terms, float32 weights) rows"""
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=off[1:])
    terms = np.concatenate([np.asarray(t, np.int32) for t, _ in rows] + [np.empty(0, np.int32)])
    w = np.concatenate([np.asarray(x, np.float32) for _, x in rows] + [np.empty(0, np.float32)])
    return U.Corpus(V, off, terms, w)


class DeviceCorpus:
    """the forward form of a ``sparse_util.Corpus`` on the GPU, as ``kp_sparse_dot`` takes it"""

    def __init__(self, c, device=0):
        import torch
        dev = torch.device("cuda", device)
        self.c, self.device = c, device
        self.terms = torch.from_numpy(np.ascontiguousarray(c.terms)).to(dev) if len(c.terms) else torch.empty(1, dtype=torch.int32, device=dev)
        self.weights = torch.from_numpy(np.ascontiguousarray(c.w16)).to(dev) if len(c.terms) else torch.empty(1, dtype=torch.float16, device=dev)


class IndexCorpus:
    """the same view of a SparseIndexer on the GPU: its host truth as a ``sparse_util.Corpus`` (the stored float16 weights are exact in float32) and its own
    device mirror, brought up to date"""

    def __init__(self, ix):
        ix._sync_mirror()
        self.c = U.Corpus(ix.vocab_size, ix.row_off.copy(), ix.terms.copy(), ix.weights.astype(np.float32))
        self.device, self.terms, self.weights = ix.device.index, ix._d_terms, ix._d_weights


def run_pairs(lib, dc, queries, pair_q, pair_row):
    """``kp_sparse_dot`` over a DeviceCorpus; returns (rc, scores fp32 [npairs], guards untouched?)"""
    import torch
    c = dc.c
    dev = torch.device("cuda", dc.device)
    q_off, q_term, q_w = U.csr(queries)
    pair_q, pair_row = np.ascontiguousarray(pair_q, np.int64), np.ascontiguousarray(pair_row, np.int64)
    n = len(pair_q)
    out = torch.full((n + 2 * U.GUARD,), float(U.GUARD_F32), dtype=torch.float32, device=dev)
    rc = lib.kp_sparse_dot(dc.terms.data_ptr(), dc.weights.data_ptr(), len(c.terms), c.row_off.ctypes.data, c.N, c.V, q_off.ctypes.data, len(queries),
                           q_term.ctypes.data, q_w.ctypes.data, pair_q.ctypes.data, pair_row.ctypes.data, n, out[U.GUARD:].data_ptr(), dc.device,
                           int(torch.cuda.current_stream(dev).cuda_stream))
    s = out.cpu().numpy()
    intact = bool((s[:U.GUARD] == U.GUARD_F32).all() and (s[U.GUARD + n:] == U.GUARD_F32).all())
    return rc, s[U.GUARD:U.GUARD + n].copy(), intact
