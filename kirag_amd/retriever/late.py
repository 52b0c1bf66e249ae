"""Late interaction: a resident store of token vectors and MaxSim over it (``libkirag_late.so``, ``include/kirag_late.h``).

``MultiVectorStore(dim, device=None)`` keeps, per passage id, the passage's token vectors as rows of IEEE binary16:

  * ``vectors``: ONE torch tensor ``[capacity, dim]`` float16 on the store's device, grown by doubling; the first ``ntokens`` rows are in use;
  * ``offsets``: host int64 ``[ntotal + 1]`` — passage ``r`` owns the rows ``offsets[r] .. offsets[r + 1] - 1`` (none is allowed);
  * ``ids``: host int64 ``[ntotal]``; ids go in and come out as decimal strings, as in ``Indexer``.  An id is stored once: a second ``add`` of it is refused.

``maxsim`` / ``rerank`` score on the GPU and only there (``kl_maxsim``: ``sum_i max_j q_i . d_j`` over the binary16 rows, exact products summed in fp32;
``reduce="mean"`` divides by the query's row count — bge-m3's colbert score —, ``reduce="sum"`` is ColBERT's).  A store on ``"cpu"`` holds, returns, saves
and loads vectors but refuses to score: there is no torch scoring path.

Rows are rounded to binary16 (nearest even) on the way in: by ``kl_gather_rows_f16`` straight from the ``[B, S, P]`` block of a flagged forward on the device
(``add_block``: the vectors never visit the host), by torch otherwise.  Both give the same bits.  A row with a NaN or an element that does not stay finite in
binary16 is refused (``ValueError``) and nothing of that call is kept.

File format (``serialize(dir)`` / ``deserialize_from(dir)``, the one file ``token_vectors.klate``, little endian, a round trip keeps every bit):

    offset  0   8 bytes   magic  b"KLATE001"
            8   int64     dim
           16   int64     N = ntotal
           24   int64     T = ntokens
           32   32 bytes  zero (reserved)
           64   int64[N]      ids
            .   int64[N + 1]  offsets
            .   uint16[T * dim]  the binary16 rows
"""
from __future__ import annotations

import os
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _late_lib

STORE_FILE = "token_vectors.klate"
MAGIC = b"KLATE001"
_HEADER = struct.Struct("<8sqqq32x")


def _as_f16_rows(a, dim: int, what: str) -> torch.Tensor:
    """``a`` (numpy array or torch tensor, any float dtype, ``[n, dim]``) as a float16 tensor on its own device, rounded to nearest even; refused when a value
    is not finite afterwards"""
    t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] != dim or not t.dtype.is_floating_point:
        raise ValueError(f"{what}: expected float rows [n, {dim}], got {tuple(t.shape)} {t.dtype}")
    h = t.to(torch.float16)
    if not bool(torch.isfinite(h).all()):
        raise ValueError(f"{what}: a value is NaN or does not stay finite in float16")
    return h


class MultiVectorStore:
    def __init__(self, dim: int, device=None):
        dim = int(dim)
        if dim < _late_lib.MIN_DIM or dim > _late_lib.MAX_DIM or dim % 32 != 0:
            raise ValueError(f"dim={dim}: token vectors are a multiple of 32 wide, {_late_lib.MIN_DIM} .. {_late_lib.MAX_DIM}")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device.type not in ("cuda", "cpu"):
            raise ValueError(f"device={device}: 'cuda[:n]' or 'cpu'")
        self.dim, self.device = dim, device
        self.vectors = torch.empty((0, dim), dtype=torch.float16, device=device)
        self.offsets = np.zeros(1, np.int64)
        self.ids = np.empty(0, np.int64)
        self._row_of = {}

    # ---- counts ----
    @property
    def ntotal(self) -> int:
        return len(self.ids)

    @property
    def ntokens(self) -> int:
        return int(self.offsets[-1])

    # ---- ingest ----
    def _new_ids(self, ids, n: int) -> np.ndarray:
        new = np.array(list(ids), dtype=np.int64).reshape(-1)       # decimal strings or integers, as Indexer._update_id_mapping
        if len(new) != n:
            raise ValueError(f"{len(new)} ids for {n} passages")
        seen = set()
        for i in new.tolist():
            if i in self._row_of or i in seen:
                raise ValueError(f"id {i} is already stored: an id holds one passage")
            seen.add(i)
        return new

    def _reserve(self, extra: int) -> int:
        """room for ``extra`` more rows (capacity doubles); returns the first free row"""
        used, cap = self.ntokens, self.vectors.shape[0]
        if used + extra > cap:
            new_cap = max(cap, 1024)
            while new_cap < used + extra:
                new_cap *= 2
            grown = torch.empty((new_cap, self.dim), dtype=torch.float16, device=self.device)
            grown[:used] = self.vectors[:used]
            self.vectors = grown
        return used

    def _commit(self, new_ids: np.ndarray, counts: np.ndarray) -> None:
        base = self.ntotal
        self.offsets = np.concatenate((self.offsets, self.offsets[-1] + np.cumsum(counts, dtype=np.int64)))
        self.ids = np.concatenate((self.ids, new_ids))
        for k, i in enumerate(new_ids.tolist()):
            self._row_of[i] = base + k

    def check_new_ids(self, ids) -> np.ndarray:
        """``ids`` as int64, refused (``ValueError``) when one is not a decimal number, occurs twice or is already stored — what ``add`` / ``add_block`` would
        refuse, without storing anything (``BGEM3Model.index_passages`` asks before the first forward)"""
        ids = list(ids)
        return self._new_ids(ids, len(ids))

    def _drop_last(self, n: int) -> None:
        """forget the last ``n`` passages (their rows stay allocated and are overwritten by the next add): how a caller that feeds a second container takes
        back a batch the other container refused"""
        keep = self.ntotal - n
        for i in self.ids[keep:].tolist():
            del self._row_of[i]
        self.ids, self.offsets = self.ids[:keep].copy(), self.offsets[:keep + 1].copy()

    def add(self, ids, list_of_arrays) -> None:
        """one ``[n_i, dim]`` array or tensor of any float dtype per id (``n_i = 0`` is allowed)"""
        rows = [_as_f16_rows(a, self.dim, f"add: passage {k}") for k, a in enumerate(list_of_arrays)]
        new_ids = self._new_ids(ids, len(rows))
        counts = np.array([r.shape[0] for r in rows], np.int64)
        T = int(counts.sum())
        t0 = self._reserve(T)
        if T:
            self.vectors[t0:t0 + T] = torch.cat(rows).to(self.device)
        self._commit(new_ids, counts)

    def add_block(self, ids, block, attention_mask, skip_first: bool = True) -> None:
        """The colbert block ``[B, S, dim]`` fp32 of ``forward_m3`` (on the store's device) and the batch's HOST attention mask ``[B, S]``: every row keeps its
        attended columns, without the first of them when ``skip_first`` (bge-m3's ``[:, 1:]``: the vector of ``<s>`` is not a token vector).  The row numbers
        are worked out on the host; the rows are converted and packed on the device."""
        if not isinstance(block, torch.Tensor) or block.dim() != 3 or block.shape[2] != self.dim:
            raise ValueError(f"add_block: expected a [B, S, {self.dim}] tensor, got {tuple(getattr(block, 'shape', ()))}")
        if block.device != self.device:
            raise ValueError(f"add_block: the block is on {block.device}, the store on {self.device}")
        B, S = int(block.shape[0]), int(block.shape[1])
        m = torch.as_tensor(np.asarray(attention_mask) if not isinstance(attention_mask, torch.Tensor) else attention_mask).cpu() != 0
        if tuple(m.shape) != (B, S):
            raise ValueError(f"add_block: attention_mask {tuple(m.shape)} does not match the block's [{B}, {S}]")
        m = m.clone()
        if skip_first and S > 0:
            first = m.to(torch.int8).argmax(dim=1)
            has = m.any(dim=1)
            m[torch.arange(B)[has], first[has]] = False
        src = torch.nonzero(m.reshape(-1)).reshape(-1).to(torch.int64).contiguous()       # row numbers into the block seen as [B * S, dim], passage by passage
        counts = m.sum(dim=1).to(torch.int64).numpy()
        new_ids = self._new_ids(ids, B)
        T = int(src.numel())
        block = block.detach().float().contiguous()
        t0 = self._reserve(T)
        if self.device.type == "cpu":
            rows = block.reshape(B * S, self.dim)[src].to(torch.float16)
            if not bool(torch.isfinite(rows).all()):
                raise ValueError("add_block: a value is NaN or does not stay finite in float16")
            self.vectors[t0:t0 + T] = rows
        elif T:
            lib = _late_lib.load()
            src_np = src.numpy()
            with torch.cuda.device(self.device):
                rc = lib.kl_gather_rows_f16(block.data_ptr(), src_np.ctypes.data, T, self.dim, self.vectors[t0:].data_ptr(), self.device.index,
                                            int(torch.cuda.current_stream(self.device).cuda_stream))
            if rc == _late_lib.ERANGE:
                raise ValueError("add_block: a value is NaN or does not stay finite in float16")
            _late_lib.check(rc)
        self._commit(new_ids, counts)

    # ---- lookup ----
    def _rows(self, ids: Sequence) -> np.ndarray:
        try:
            return np.fromiter((self._row_of[int(i)] for i in ids), dtype=np.int64, count=len(ids))
        except KeyError as e:
            raise KeyError(f"id {e.args[0]} is not in the store") from None

    def get(self, id) -> np.ndarray:
        """the stored (rounded) rows of one id as fp32 ``[n, dim]``"""
        r = int(self._rows([id])[0])
        return self.vectors[int(self.offsets[r]):int(self.offsets[r + 1])].float().cpu().numpy()

    # ---- files ----
    def serialize(self, dir_path) -> None:
        with open(os.path.join(dir_path, STORE_FILE), "wb") as f:
            f.write(_HEADER.pack(MAGIC, self.dim, self.ntotal, self.ntokens))
            f.write(self.ids.astype("<i8").tobytes())
            f.write(self.offsets.astype("<i8").tobytes())
            f.write(self.vectors[:self.ntokens].cpu().contiguous().view(torch.int16).numpy().astype("<i2").tobytes())

    def deserialize_from(self, dir_path) -> None:
        path = os.path.join(dir_path, STORE_FILE)
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise ValueError(f"{path}: shorter than its header")
            magic, dim, N, T = _HEADER.unpack(head)
            if magic != MAGIC:
                raise ValueError(f"{path}: magic {magic!r}, expected {MAGIC!r}")
            if dim != self.dim:
                raise ValueError(f"{path}: dim={dim}, this store has dim={self.dim}")
            if N < 0 or T < 0:
                raise ValueError(f"{path}: N={N}, T={T}")
            ids = np.frombuffer(f.read(8 * N), dtype="<i8")
            offsets = np.frombuffer(f.read(8 * (N + 1)), dtype="<i8")
            raw = np.frombuffer(f.read(2 * T * dim), dtype="<i2")
        if len(ids) != N or len(offsets) != N + 1 or len(raw) != T * dim:
            raise ValueError(f"{path}: truncated")
        if offsets[0] != 0 or offsets[-1] != T or (np.diff(offsets) < 0).any():
            raise ValueError(f"{path}: offsets do not run from 0 to T={T} without decreasing")
        if len(set(ids.tolist())) != N:
            raise ValueError(f"{path}: an id occurs twice")
        self.ids, self.offsets = ids.astype(np.int64), offsets.astype(np.int64)
        self._row_of = {i: k for k, i in enumerate(self.ids.tolist())}
        self.vectors = torch.from_numpy(raw.astype(np.int16)).view(torch.float16).reshape(T, dim).to(self.device)

    # ---- scoring (GPU only) ----
    def maxsim(self, queries, candidates, reduce: str = "mean") -> List[np.ndarray]:
        """``queries``: a list of ``[n_i, dim]`` arrays or tensors (rounded to float16 as the stored rows are); ``candidates``: per query a list of ids.
        One fp32 array of scores per query, in the order of its ids.  An unknown id raises ``KeyError`` before anything is launched."""
        if self.device.type != "cuda":
            raise RuntimeError("MultiVectorStore.maxsim runs on the GPU (libkirag_late.so): this store is on the CPU and there is no torch scoring path")
        if reduce not in _late_lib.REDUCE:
            raise ValueError(f"reduce={reduce!r}: 'mean' or 'sum'")
        if len(queries) != len(candidates):
            raise ValueError(f"{len(queries)} queries, {len(candidates)} candidate lists")
        docs = [self._rows(c) for c in candidates]
        q16 = [_as_f16_rows(q, self.dim, f"maxsim: query {k}") for k, q in enumerate(queries)]
        sizes = [len(d) for d in docs]
        npairs = int(sum(sizes))
        if npairs == 0:
            return [np.empty(0, np.float32) for _ in docs]
        q_off = np.zeros(len(q16) + 1, np.int64)
        np.cumsum([t.shape[0] for t in q16], out=q_off[1:])
        pair_q = np.repeat(np.arange(len(docs), dtype=np.int64), sizes)
        pair_d = np.ascontiguousarray(np.concatenate(docs))
        lib = _late_lib.load()
        with torch.cuda.device(self.device):
            qd = torch.cat([t.to(self.device) for t in q16]).contiguous() if q_off[-1] else torch.empty((0, self.dim), dtype=torch.float16, device=self.device)
            out = torch.empty(npairs, dtype=torch.float32, device=self.device)
            _late_lib.check(lib.kl_maxsim(qd.data_ptr(), q_off.ctypes.data, len(q16), self.vectors.data_ptr(), self.offsets.ctypes.data, self.ntotal,
                                          pair_q.ctypes.data, pair_d.ctypes.data, npairs, self.dim, _late_lib.REDUCE[reduce], out.data_ptr(),
                                          self.device.index, int(torch.cuda.current_stream(self.device).cuda_stream)))
            flat = out.cpu().numpy()
        return np.split(flat, np.cumsum(sizes)[:-1])

    def rerank(self, query, candidate_ids, top_k: Optional[int] = None, reduce: str = "mean") -> Tuple[List[str], np.ndarray]:
        """``(ids, scores)`` of the best ``top_k`` candidates (all when ``None``) by (score descending, position in ``candidate_ids`` ascending)"""
        cand = list(candidate_ids)
        s = self.maxsim([query], [cand], reduce)[0]
        order = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))
        if top_k is not None:
            order = order[:top_k]
        return [str(int(cand[i])) for i in order], s[order]
