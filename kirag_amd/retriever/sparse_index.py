"""Sparse retrieval: a resident doc-range-blocked inverted index over learned sparse vectors and exact top-k over it (``libkirag_sparse.so``,
``include/kirag_sparse.h``).

``SparseIndexer(vocab_size, device=None, token_to_id=None)`` keeps

  * the host truth, the forward form: ``ids`` int64 ``[N]``, ``row_off`` int64 ``[N + 1]``, ``terms`` int32 and ``weights`` float16 ``[nnz]`` — passage ``r``
    holds the terms ``terms[row_off[r]:row_off[r + 1]]``, strictly ascending, with weights that are finite and > 0.  Ids go in and come out as decimal
    strings, as in ``Indexer``.  An id is stored once: a second add of it is refused;
  * the inverted form on the index's device, the layout of ``kirag_sparse.h``: block ``b`` owns the rows ``b R .. (b + 1) R - 1`` (``R`` is the library's
    ``ks_block_rows()``), its postings ``(local row << 16) | float16 bits`` lie in ONE tensor grown by doubling, its ``uint32[V + 1]`` pointer table is a row
    of a ``[blocks, V + 1]`` tensor.  The inversion runs on the host in numpy and is incremental: a block is inverted once, when its R-th row arrives, and
    uploaded; only the open tail block is inverted again, lazily at the next search after an add.

  * lazily, a device mirror of the forward form (``terms`` int32 and ``weights`` float16, grown by doubling; ``row_off`` stays on the host): nothing is
    uploaded until the first ``score_pairs`` call, and then only the suffix added since the last one.  An index that is only searched never holds it.

``score_pairs`` / ``rerank`` score given (query, id) pairs against the stored rows without scanning the index (``kp_sparse_dot``, ``libkirag_pairs.so``,
``include/kirag_pairs.h``): the same definition, so wherever ``search_knn`` returns an id, ``score_pairs`` gives it the same score bits.

``search_knn`` scores on the GPU and only there (``ks_search``: exact, in the summation order the header defines).  An index on ``"cpu"`` stores, returns,
saves and loads but refuses to search: there is no torch scoring path.

A passage (and a query) is any of: a ``{str(term_id): weight}`` dict (bge-m3's ``lexical_weights``); a ``{token string: weight}`` dict when a ``token_to_id``
callable was given at construction (then EVERY dict key is a token string); a ``(terms, weights)`` pair of arrays.  Duplicate terms keep the max (bge-m3's
rule).  Passage weights are rounded to float16 (nearest even) and dropped when not > 0 afterwards; query weights stay float32 and are dropped when not > 0.
A term outside ``[0, vocab_size)`` or a weight that is NaN, Inf or overflows float16 raises ``ValueError`` and nothing of the call is kept.

File format (``serialize(dir)`` / ``deserialize_from(dir)``, the one file ``sparse_index.ksparse``, little endian, the forward form; a round trip keeps every
bit, loading inverts again):

    offset  0   8 bytes   magic  b"KSPARSE1"
            8   int64     V = vocab_size
           16   int64     R = rows per block of the library that wrote the file (16384 or 32768; a record, the forward form does not depend on it)
           24   int64     N = ntotal
           32   int64     nnz
           40   24 bytes  zero (reserved)
           64   int64[N]      ids
            .   int64[N + 1]  row_off
            .   int32[nnz]    terms
            .   uint16[nnz]   the float16 weight bits
"""
from __future__ import annotations

import os
import struct
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _pairs_lib, _sparse_lib

INDEX_FILE = "sparse_index.ksparse"
MAGIC = b"KSPARSE1"
_HEADER = struct.Struct("<8sqqqq24x")
F16_MAX = 65504.0


def invert_block(row_off: np.ndarray, terms: np.ndarray, weight_bits: np.ndarray, r0: int, r1: int, V: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rows ``r0 .. r1 - 1`` of a forward CSR as one block of the inverted layout: ``(ptr uint32[V + 1], post uint32[n])``, the postings of term ``t`` at
    ``post[ptr[t]:ptr[t + 1]]`` in ascending local row, each ``(local row << 16) | weight bits``.  ``r1 - r0 <= 65536``."""
    a, b = int(row_off[r0]), int(row_off[r1])
    t = terms[a:b]
    counts = np.diff(row_off[r0:r1 + 1])
    local = np.repeat(np.arange(r1 - r0, dtype=np.uint32), counts)
    order = np.argsort(t, kind="stable")          # the rows arrive in ascending order: a stable sort by term keeps them ascending within a term
    post = (local[order] << np.uint32(16)) | weight_bits[a:b][order].astype(np.uint32)
    ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(t, minlength=V), out=ptr[1:])
    return ptr.astype(np.uint32), post.astype(np.uint32)


def _grow(arr: np.ndarray, used: int, extra: int) -> np.ndarray:
    """``arr`` with room for ``used + extra`` elements (capacity doubles), the first ``used`` kept"""
    if used + extra <= len(arr):
        return arr
    cap = max(len(arr), 1024)
    while cap < used + extra:
        cap *= 2
    out = np.empty(cap, arr.dtype)
    out[:used] = arr[:used]
    return out


class SparseIndexer:
    def __init__(self, vocab_size: int, device=None, token_to_id: Optional[Callable[[str], int]] = None):
        V = int(vocab_size)
        if V < 1 or V > (1 << 24):
            raise ValueError(f"vocab_size={V}: 1 .. 2^24")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device.type not in ("cuda", "cpu"):
            raise ValueError(f"device={device}: 'cuda[:n]' or 'cpu'")
        self.vocab_size, self.device, self.token_to_id = V, device, token_to_id
        self.block_rows = _sparse_lib.block_rows()
        self._reset()

    def _reset(self) -> None:
        self._ids = np.empty(0, np.int64)
        self._row_off = np.zeros(1, np.int64)
        self._terms = np.empty(0, np.int32)
        self._weights = np.empty(0, np.float16)
        self._n = 0
        self._row_of = {}
        self._post = torch.empty(0, dtype=torch.int32, device=self.device)                              # uint32 bit patterns
        self._ptr = torch.empty((0, self.vocab_size + 1), dtype=torch.int32, device=self.device)        # uint32 values
        self._post_off = [0]          # per closed block, plus the tail's end once the tail is inverted
        self._closed = 0              # blocks inverted for good
        self._tail_rows = 0           # rows of the open tail block that _post / _ptr reflect
        self._d_terms = self._d_weights = None      # the device mirror of the forward form, made by the first score_pairs
        self._synced = 0              # entries of _terms / _weights the mirror reflects

    # ---- the host truth ----
    @property
    def ntotal(self) -> int:
        return self._n

    @property
    def nnz(self) -> int:
        return int(self._row_off[self._n])

    @property
    def ids(self) -> np.ndarray:
        return self._ids[:self._n]

    @property
    def row_off(self) -> np.ndarray:
        return self._row_off[:self._n + 1]

    @property
    def terms(self) -> np.ndarray:
        return self._terms[:self.nnz]

    @property
    def weights(self) -> np.ndarray:
        return self._weights[:self.nnz]

    def get(self, id) -> Tuple[np.ndarray, np.ndarray]:
        """``(terms int32, weights float16)`` of one id, as stored"""
        try:
            r = self._row_of[int(id)]
        except KeyError:
            raise KeyError(f"id {id} is not in the index") from None
        a, b = int(self._row_off[r]), int(self._row_off[r + 1])
        return self._terms[a:b].copy(), self._weights[a:b].copy()

    # ---- ingest ----
    def check_new_ids(self, ids) -> np.ndarray:
        """``ids`` as int64, refused (``ValueError``) when one is not a decimal number, occurs twice or is already stored — what an add would refuse, without
        storing anything"""
        new = np.array(list(ids), dtype=np.int64).reshape(-1)
        seen = set()
        for i in new.tolist():
            if i in self._row_of or i in seen:
                raise ValueError(f"id {i} is already stored: an id holds one passage")
            seen.add(i)
        return new

    def _term_id(self, key) -> int:
        if self.token_to_id is not None:
            t = self.token_to_id(key)
            if t is None:
                raise ValueError(f"token {key!r} is unknown to token_to_id")
            return int(t)
        try:
            return int(key)
        except (TypeError, ValueError):
            raise ValueError(f"term {key!r} is not a term id: give the index a token_to_id callable to pass {{token string: weight}} dicts") from None

    def _flatten(self, vectors: Sequence, what: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """the vectors of a call as ``(row, term, float64 weight)`` arrays in the order given; terms checked against the vocabulary, weights against NaN / Inf"""
        rows, terms, weights = [], [], []
        for k, v in enumerate(vectors):
            if isinstance(v, dict):
                t = np.fromiter((self._term_id(key) for key in v), dtype=np.int64, count=len(v))
                w = np.fromiter((float(x) for x in v.values()), dtype=np.float64, count=len(v))
            else:
                if len(v) != 2:
                    raise ValueError(f"{what} {k}: a dict or a (terms, weights) pair")
                t = np.asarray(v[0]).reshape(-1)
                w = np.asarray(v[1], dtype=np.float64).reshape(-1)
                if len(t) and not np.issubdtype(t.dtype, np.integer):
                    raise ValueError(f"{what} {k}: terms are integers, got {t.dtype}")
                t = t.astype(np.int64)
                if len(t) != len(w):
                    raise ValueError(f"{what} {k}: {len(t)} terms, {len(w)} weights")
            if len(t) and (t.min() < 0 or t.max() >= self.vocab_size):
                bad = t[(t < 0) | (t >= self.vocab_size)][0]
                raise ValueError(f"{what} {k}: term {int(bad)} outside [0, vocab_size={self.vocab_size})")
            if not np.isfinite(w).all():
                raise ValueError(f"{what} {k}: a weight is NaN or Inf")
            rows.append(np.full(len(t), k, np.int64)); terms.append(t); weights.append(w)
        cat = lambda parts, dt: np.concatenate(parts) if parts else np.empty(0, dt)
        return cat(rows, np.int64), cat(terms, np.int64), cat(weights, np.float64)

    @staticmethod
    def _merge(n: int, row, term, w) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """max over duplicate (row, term), weights not > 0 dropped, ascending term within a row: ``(counts[n], terms int32, weights)``"""
        order = np.lexsort((w, term, row))
        row, term, w = row[order], term[order], w[order]
        last = np.ones(len(row), bool)
        last[:-1] = (row[1:] != row[:-1]) | (term[1:] != term[:-1])      # the largest weight of a (row, term) run comes last
        keep = last & (w > 0)
        return np.bincount(row[keep], minlength=n).astype(np.int64), term[keep].astype(np.int32), w[keep]

    def index_data(self, ids, vectors) -> None:
        """one sparse vector per id, in any of the three forms"""
        vectors = list(vectors)
        row, term, w = self._flatten(vectors, "passage")
        with np.errstate(over="ignore"):
            w16 = w.astype(np.float16)
        if np.isinf(w16).any():
            raise ValueError("a weight overflows float16")
        ids = list(ids)
        if len(ids) != len(vectors):
            raise ValueError(f"{len(ids)} ids for {len(vectors)} passages")
        new_ids = self.check_new_ids(ids)
        counts, terms, w16 = self._merge(len(vectors), row, term, w16)
        self._commit(new_ids, counts, terms, w16)

    def index_block(self, ids, block, skip_terms: Sequence[int] = ()) -> None:
        """The ``[B, vocab_size]`` block of ``forward_splade`` (on the index's device): every value that is > 0 once rounded to float16 is kept, except under
        the terms in ``skip_terms`` (the tokenizer's pad id).  On the GPU the rows are compacted by ``ks_count_positive`` / ``ks_compact_rows`` and only the
        kept (term, weight) entries visit the host; on a CPU index the same rule runs in torch.  Both give the same bits."""
        V = self.vocab_size
        if not isinstance(block, torch.Tensor) or block.dim() != 2 or block.shape[1] != V:
            raise ValueError(f"index_block: expected a [B, {V}] tensor, got {tuple(getattr(block, 'shape', ()))}")
        if block.device != self.device:
            raise ValueError(f"index_block: the block is on {block.device}, the index on {self.device}")
        B = int(block.shape[0])
        ids = list(ids)
        if len(ids) != B:
            raise ValueError(f"{len(ids)} ids for {B} passages")
        skip = np.array(sorted({int(s) for s in skip_terms if s is not None}), np.int32)
        if len(skip) and (skip.min() < 0 or skip.max() >= V):
            raise ValueError(f"index_block: skip_terms {skip.tolist()} outside [0, vocab_size={V})")
        new_ids = self.check_new_ids(ids)
        block = block.detach().float().contiguous()
        refused = "index_block: a value is NaN or does not stay finite in float16"
        if self.device.type == "cpu":
            h = block.to(torch.float16)
            if not bool(torch.isfinite(h).all()):
                raise ValueError(refused)
            keep = h > 0
            if len(skip):
                keep[:, torch.from_numpy(skip.astype(np.int64))] = False
            counts = keep.sum(dim=1).to(torch.int64).numpy()
            terms = torch.nonzero(keep)[:, 1].to(torch.int32).numpy()          # row-major: ascending term within a row
            w16 = h[keep].numpy()
        else:
            lib = _sparse_lib.load()
            counts = np.zeros(B, np.int64)
            with torch.cuda.device(self.device):
                stream = int(torch.cuda.current_stream(self.device).cuda_stream)
                rc = lib.ks_count_positive(block.data_ptr(), B, V, skip.ctypes.data, len(skip), counts.ctypes.data, self.device.index, stream)
                if rc == _sparse_lib.ERANGE:
                    raise ValueError(refused)
                _sparse_lib.check(rc)
                off = np.zeros(B + 1, np.int64)
                np.cumsum(counts, out=off[1:])
                n = int(off[-1])
                d_terms = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
                d_w = torch.empty(max(n, 1), dtype=torch.float16, device=self.device)
                rc = lib.ks_compact_rows(block.data_ptr(), B, V, skip.ctypes.data, len(skip), off.ctypes.data, d_terms.data_ptr(), d_w.data_ptr(),
                                         self.device.index, stream)
                if rc == _sparse_lib.ERANGE:
                    raise ValueError(refused)
                _sparse_lib.check(rc)
                terms, w16 = d_terms[:n].cpu().numpy(), d_w[:n].cpu().numpy()
        self._commit(new_ids, counts, terms, w16)

    def _commit(self, new_ids: np.ndarray, counts: np.ndarray, terms: np.ndarray, w16: np.ndarray) -> None:
        n, m, used = len(new_ids), len(terms), self.nnz
        self._ids = _grow(self._ids, self._n, n)
        self._row_off = _grow(self._row_off, self._n + 1, n)
        self._terms = _grow(self._terms, used, m)
        self._weights = _grow(self._weights, used, m)
        self._ids[self._n:self._n + n] = new_ids
        self._row_off[self._n + 1:self._n + 1 + n] = used + np.cumsum(counts, dtype=np.int64)
        self._terms[used:used + m] = terms
        self._weights[used:used + m] = w16
        for k, i in enumerate(new_ids.tolist()):
            self._row_of[i] = self._n + k
        self._n += n
        R = self.block_rows
        while self._n >= (self._closed + 1) * R:          # a block is inverted once, when its R-th row arrives
            self._invert_into(self._closed, self._closed * R, (self._closed + 1) * R)
            self._closed += 1
            self._tail_rows = 0

    def _drop_last(self, n: int) -> None:
        """forget the last ``n`` passages: how a caller that feeds a second container takes back a batch the other container refused"""
        keep = self._n - n
        for i in self._ids[keep:self._n].tolist():
            del self._row_of[i]
        self._n = keep
        R = self.block_rows
        if keep < self._closed * R:                        # a closed block lost rows: it is the open tail again
            self._closed = keep // R
        del self._post_off[self._closed + 1:]
        self._tail_rows = 0
        self._synced = min(self._synced, self.nnz)      # the entries behind are overwritten by the next add

    # ---- the inverted form ----
    def _invert_into(self, b: int, r0: int, r1: int) -> None:
        """invert the rows r0 .. r1 - 1 as block ``b``, the last block held: its postings go behind block b - 1's"""
        ptr, post = invert_block(self._row_off, self._terms, self._weights.view(np.uint16), r0, r1, self.vocab_size)
        del self._post_off[b + 1:]
        start = self._post_off[b]
        if start + len(post) > self._post.shape[0]:
            cap = max(int(self._post.shape[0]), 1 << 16)
            while cap < start + len(post):
                cap *= 2
            grown = torch.empty(cap, dtype=torch.int32, device=self.device)
            grown[:start] = self._post[:start]
            self._post = grown
        if b >= self._ptr.shape[0]:
            grown = torch.empty((max(1, 2 * int(self._ptr.shape[0])), self.vocab_size + 1), dtype=torch.int32, device=self.device)
            grown[:b] = self._ptr[:b]
            self._ptr = grown
        if len(post):
            self._post[start:start + len(post)] = torch.from_numpy(post.view(np.int32)).to(self.device)
        self._ptr[b] = torch.from_numpy(ptr.view(np.int32)).to(self.device)
        self._post_off.append(start + len(post))

    def _sync_tail(self) -> np.ndarray:
        """bring the open tail block up to date; the ``post_off`` array of a search: one entry per block and the end"""
        tail = self._n - self._closed * self.block_rows
        if tail > 0 and self._tail_rows != tail:
            self._invert_into(self._closed, self._closed * self.block_rows, self._n)
            self._tail_rows = tail
        return np.asarray(self._post_off[:self._closed + (1 if tail > 0 else 0) + 1], np.int64)

    # ---- search (GPU only) ----
    def _queries_csr(self, queries) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        queries = list(queries)
        row, term, w = self._flatten(queries, "query")
        w32 = w.astype(np.float32)
        if np.isinf(w32).any():
            raise ValueError("a query weight overflows float32")
        counts, terms, w32 = self._merge(len(queries), row, term, w32)
        off = np.zeros(len(queries) + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        return off, np.ascontiguousarray(terms, np.int32), np.ascontiguousarray(w32, np.float32)

    def search_arrays(self, queries, top_docs: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(scores fp32 [nq, k], rows int64 [nq, k])`` as ``ks_search`` leaves them: places without a result hold row -1 and score +0.0"""
        if self.device.type != "cuda":
            raise RuntimeError("SparseIndexer.search_knn runs on the GPU (libkirag_sparse.so): this index is on the CPU and there is no torch scoring path")
        k = int(top_docs)
        q_off, q_term, q_w = self._queries_csr(queries)
        nq = len(q_off) - 1
        post_off = self._sync_tail()
        lib = _sparse_lib.load()
        with torch.cuda.device(self.device):
            scores = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=self.device)
            rows = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=self.device)
            stream = int(torch.cuda.current_stream(self.device).cuda_stream)
            for s in range(0, max(nq, 1), _sparse_lib.MAX_QUERIES):
                e = min(nq, s + _sparse_lib.MAX_QUERIES)
                off = np.ascontiguousarray(q_off[s:e + 1] - q_off[s])
                a = int(q_off[s])
                _sparse_lib.check(lib.ks_search(self._post.data_ptr(), self._ptr.data_ptr(), post_off.ctypes.data, self._n, self.vocab_size, off.ctypes.data,
                                                e - s, q_term[a:].ctypes.data, q_w[a:].ctypes.data, k, scores[s:].data_ptr(), rows[s:].data_ptr(),
                                                self.device.index, stream))
            return scores.cpu().numpy(), rows.cpu().numpy()

    def search_knn(self, queries, top_docs: int) -> List[Tuple[List[str], List[float]]]:
        """Per query ``(ids, scores)`` of the best ``top_docs`` passages with a score > 0 by (score descending, insertion order ascending): the shape of
        ``Indexer.search_knn``, except that a query may return fewer than ``top_docs`` entries (a passage sharing no term with the query is no result)."""
        scores, rows = self.search_arrays(queries, top_docs)
        out = []
        for s, r in zip(scores, rows):
            n = int((r >= 0).sum())
            out.append(([str(i) for i in self._ids[r[:n]].tolist()], s[:n].tolist()))
        return out

    # ---- scoring given (query, id) pairs (GPU only) ----
    def _sync_mirror(self) -> None:
        """bring the device mirror of the forward form up to date: upload the entries added since the last call"""
        nnz = self.nnz
        if self._d_terms is None or nnz > self._d_terms.shape[0]:
            cap = max(int(self._d_terms.shape[0]) if self._d_terms is not None else 0, 1 << 16)
            while cap < nnz:
                cap *= 2
            terms = torch.empty(cap, dtype=torch.int32, device=self.device)
            weights = torch.empty(cap, dtype=torch.float16, device=self.device)
            if self._synced:
                terms[:self._synced] = self._d_terms[:self._synced]
                weights[:self._synced] = self._d_weights[:self._synced]
            self._d_terms, self._d_weights = terms, weights
        if nnz > self._synced:
            a = self._synced
            self._d_terms[a:nnz] = torch.from_numpy(self._terms[a:nnz]).to(self.device)
            self._d_weights[a:nnz] = torch.from_numpy(self._weights[a:nnz]).to(self.device)
            self._synced = nnz

    def rows_of(self, ids) -> np.ndarray:
        """the rows of stored ids as int64; an unknown id raises ``KeyError``"""
        ids = list(ids)
        try:
            return np.fromiter((self._row_of[int(i)] for i in ids), dtype=np.int64, count=len(ids))
        except KeyError as e:
            raise KeyError(f"id {e.args[0]} is not in the index") from None
        except ValueError:
            bad = next(i for i in ids if not str(i).strip().lstrip("+-").isdigit())
            raise KeyError(f"id {bad} is not in the index") from None

    def score_pairs(self, queries, candidates) -> List[np.ndarray]:
        """``queries``: as ``search_knn`` takes them; ``candidates``: per query a list of ids.  One fp32 array of scores per query, in the order of its ids:
        the score ``search_knn`` would give that passage (same bits), ``+0.0`` when it shares no term with the query.  A length mismatch raises ``ValueError``
        and an unknown id ``KeyError`` before anything is launched; an index on the CPU raises ``RuntimeError``."""
        queries, candidates = list(queries), list(candidates)
        if len(queries) != len(candidates):
            raise ValueError(f"{len(queries)} queries, {len(candidates)} candidate lists")
        return self.score_rows(queries, [self.rows_of(c) for c in candidates])

    def score_rows(self, queries, rows) -> List[np.ndarray]:
        """``score_pairs`` for a caller that holds row numbers (insertion order, as ``search_arrays`` returns them) instead of ids: per query an int64 array of
        rows.  A row outside ``[0, ntotal)`` is refused by the library by name."""
        queries, rows = list(queries), [np.ascontiguousarray(r, np.int64).reshape(-1) for r in rows]
        if len(queries) != len(rows):
            raise ValueError(f"{len(queries)} queries, {len(rows)} row lists")
        if self.device.type != "cuda":
            raise RuntimeError("SparseIndexer.score_pairs runs on the GPU (libkirag_pairs.so): this index is on the CPU and there is no torch scoring path")
        q_off, q_term, q_w = self._queries_csr(queries)
        sizes = [len(r) for r in rows]
        npairs = int(sum(sizes))
        if npairs == 0:
            return [np.empty(0, np.float32) for _ in rows]
        pair_q = np.repeat(np.arange(len(rows), dtype=np.int64), sizes)
        pair_row = np.ascontiguousarray(np.concatenate(rows))
        first = np.zeros(len(rows) + 1, np.int64)           # the first pair of each query
        np.cumsum(sizes, out=first[1:])
        lib = _pairs_lib.load()
        self._sync_mirror()
        with torch.cuda.device(self.device):
            out = torch.empty(npairs, dtype=torch.float32, device=self.device)
            stream = int(torch.cuda.current_stream(self.device).cuda_stream)
            for s in range(0, len(rows), _pairs_lib.MAX_QUERIES):              # the library's bounds per call: queries, then pairs
                e = min(len(rows), s + _pairs_lib.MAX_QUERIES)
                off = np.ascontiguousarray(q_off[s:e + 1] - q_off[s])
                a = int(q_off[s])
                for p0 in range(int(first[s]), int(first[e]), _pairs_lib.MAX_PAIRS):
                    p1 = min(int(first[e]), p0 + _pairs_lib.MAX_PAIRS)
                    pq = np.ascontiguousarray(pair_q[p0:p1] - s)
                    _pairs_lib.check(lib.kp_sparse_dot(self._d_terms.data_ptr(), self._d_weights.data_ptr(), self.nnz, self._row_off.ctypes.data, self._n,
                                                       self.vocab_size, off.ctypes.data, e - s, q_term[a:].ctypes.data, q_w[a:].ctypes.data, pq.ctypes.data,
                                                       pair_row[p0:].ctypes.data, p1 - p0, out[p0:].data_ptr(), self.device.index, stream))
            flat = out.cpu().numpy()
        return np.split(flat, first[1:-1])

    def rerank(self, query, candidate_ids, top_k: Optional[int] = None) -> Tuple[List[str], np.ndarray]:
        """``(ids, scores)`` of the best ``top_k`` candidates (all when ``None``) by (score descending, position in ``candidate_ids`` ascending)"""
        cand = list(candidate_ids)
        s = self.score_pairs([query], [cand])[0]
        order = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))
        if top_k is not None:
            order = order[:top_k]
        return [str(int(cand[i])) for i in order], s[order]

    # ---- files ----
    def serialize(self, dir_path) -> None:
        with open(os.path.join(dir_path, INDEX_FILE), "wb") as f:
            f.write(_HEADER.pack(MAGIC, self.vocab_size, self.block_rows, self.ntotal, self.nnz))
            f.write(self.ids.astype("<i8").tobytes())
            f.write(self.row_off.astype("<i8").tobytes())
            f.write(self.terms.astype("<i4").tobytes())
            f.write(self.weights.view(np.uint16).astype("<u2").tobytes())

    def deserialize_from(self, dir_path) -> None:
        path = os.path.join(dir_path, INDEX_FILE)
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise ValueError(f"{path}: shorter than its header")
            magic, V, R, N, nnz = _HEADER.unpack(head)
            if magic != MAGIC:
                raise ValueError(f"{path}: magic {magic!r}, expected {MAGIC!r}")
            if V != self.vocab_size:
                raise ValueError(f"{path}: V={V}, this index has vocab_size={self.vocab_size}")
            if R not in (16384, 32768):
                raise ValueError(f"{path}: R={R}: 16384 or 32768")
            if N < 0 or nnz < 0:
                raise ValueError(f"{path}: N={N}, nnz={nnz}")
            ids = np.frombuffer(f.read(8 * N), dtype="<i8")
            row_off = np.frombuffer(f.read(8 * (N + 1)), dtype="<i8")
            terms = np.frombuffer(f.read(4 * nnz), dtype="<i4")
            bits = np.frombuffer(f.read(2 * nnz), dtype="<u2")
        if len(ids) != N or len(row_off) != N + 1 or len(terms) != nnz or len(bits) != nnz:
            raise ValueError(f"{path}: truncated")
        if row_off[0] != 0 or row_off[-1] != nnz or (np.diff(row_off) < 0).any():
            raise ValueError(f"{path}: row_off does not run from 0 to nnz={nnz} without decreasing")
        if len(set(ids.tolist())) != N:
            raise ValueError(f"{path}: an id occurs twice")
        if nnz and (terms.min() < 0 or terms.max() >= V):
            raise ValueError(f"{path}: a term lies outside [0, V={V})")
        inner = np.ones(nnz, bool)
        inner[row_off[:-1][row_off[:-1] < nnz]] = False           # the first entry of a row has no predecessor in its row
        if nnz and (np.diff(terms.astype(np.int64), prepend=-1)[inner] <= 0).any():
            raise ValueError(f"{path}: the terms of a row do not ascend strictly")
        w16 = bits.astype(np.uint16).view(np.float16)
        if nnz and not (np.isfinite(w16) & (w16 > 0)).all():
            raise ValueError(f"{path}: a weight is not finite and > 0")
        self._reset()
        self._commit(ids.astype(np.int64), np.diff(row_off).astype(np.int64), terms.astype(np.int32), w16)
