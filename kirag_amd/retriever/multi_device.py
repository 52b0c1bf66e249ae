"""``MultiDeviceIndexer``: the reference's ``Indexer`` surface (``retriever/index.py:17-83``) over row shards held by ONE process, each shard a ``kr_index``
handle on any GPU (repeats allowed: ``devices=[0, 0, 0]`` puts three shards on one GPU).  The SPMD path (``ShardedIndexer`` / ``ShardedSearcher``) needs W
processes that pass the same queries to every search; the KiRAG loop (an LLM step between hops, per-rank seeds) cannot be replicated that way, so this
class drives all shards from the caller's process instead.

Global row numbering is the insertion order, exactly as in the one-device ``Indexer``; every shard holds its rows in increasing global order, so a shard's
list sorted by (score desc, local row asc) is also sorted by (score desc, global row asc) once mapped, and ``kr_topk_merge`` of the W lists equals the
one-device answer bit for bit, ties included.  The search itself is the existing HIP path on every shard; this module only orchestrates handles, streams and
devices."""
from __future__ import annotations

import logging
import os
import pickle
from typing import List, Optional

import numpy as np

from .. import _lib
from ..parallel import ShardedSearcher
from .flat_index import FlatIPIndex
from .formats import SHARD_MANIFEST, _manifest_matches, read_faiss_flat_ip, read_native_shards, shard_range
from .index import Indexer

logger = logging.getLogger()

ENV_INDEX_DEVICES = "KIRAG_AMD_INDEX_DEVICES"


# ---- placement: which shard takes each inserted row (pure; tests/test_multi_device_host.py) -------------------------------------------------------------
class RowPlacement:
    """Row placement over ``world`` shards and the local -> global row maps.

    * ``reserve(n)`` with n > ntotal plans the next n - ntotal rows as ``world`` contiguous pieces (``shard_range``); shard s takes piece s.  Later
      appends fill that plan in insertion order.
    * Rows beyond the plan (or with no plan): each appended batch is split into ``world`` near-equal contiguous pieces (sizes differ by at most one, the
      larger ones first), one per shard in shard order.
    Every shard receives its rows in increasing global order.  The map of shard s is a list of runs ``(global_start, local_start, count)``."""

    def __init__(self, world: int):
        if world < 1:
            raise ValueError("a shard group needs at least one shard")
        self.world = int(world)
        self.ntotal = 0
        self.shard_rows = [0] * self.world
        self.runs = [[] for _ in range(self.world)]
        self._plan = None              # (first global row of the plan, row count) or None
        self._maps = [None] * self.world
        self._sorted = None

    def plan_bounds(self):
        """global row boundaries of the current plan's pieces ([world + 1]), or None"""
        if self._plan is None:
            return None
        p0, n = self._plan
        return [p0 + shard_range(n, s, self.world)[0] for s in range(self.world)] + [p0 + n]

    def reserve(self, n: int) -> List[int]:
        """Plan rows up to ``n`` in total; returns the row count each shard will hold once the plan is filled."""
        n = int(n)
        if n > self.ntotal:
            self._plan = (self.ntotal, n - self.ntotal)
        bounds = self.plan_bounds()
        if bounds is None:
            return list(self.shard_rows)
        return [self.shard_rows[s] + max(0, bounds[s + 1] - max(bounds[s], self.ntotal)) for s in range(self.world)]

    def place(self, m: int):
        """Append ``m`` rows: [(shard, offset in the batch, count)] in insertion order (pieces with count 0 left out)."""
        m = int(m)
        pieces = []
        off = 0
        while off < m:
            g = self.ntotal + off
            bounds = self.plan_bounds()
            if bounds is not None and g < bounds[-1]:
                s = next(s for s in range(self.world) if g < bounds[s + 1])
                cnt = min(m - off, bounds[s + 1] - g)
                pieces.append((s, off, cnt))
            else:
                self._plan = None
                rest = m - off
                base, extra = divmod(rest, self.world)
                o = off
                for s in range(self.world):
                    c = base + (1 if s < extra else 0)
                    if c:
                        pieces.append((s, o, c))
                    o += c
                cnt = rest
            off += cnt
            # (the global row of a piece is ntotal + its offset: recorded below, once the whole batch is placed)
        for s, o, c in pieces:
            self._record(s, self.ntotal + o, c)
        self.ntotal += m
        if self._plan is not None and self.ntotal >= self._plan[0] + self._plan[1]:
            self._plan = None
        return pieces

    def _record(self, s: int, g0: int, cnt: int):
        l0 = self.shard_rows[s]
        runs = self.runs[s]
        if runs and runs[-1][0] + runs[-1][2] == g0 and runs[-1][1] + runs[-1][2] == l0:
            runs[-1] = (runs[-1][0], runs[-1][1], runs[-1][2] + cnt)
        else:
            runs.append((g0, l0, cnt))
        self.shard_rows[s] += cnt
        self._maps[s] = None
        self._sorted = None

    def load(self, n: int):
        """State of ``n`` rows loaded as ``shard_range(n, s, world)`` per shard (``deserialize_from``)."""
        self.__init__(self.world)
        self.reserve(n)
        return self.place(n)

    def _map(self, s: int):
        mp = self._maps[s]
        if mp is None:
            r = np.array(self.runs[s], dtype=np.int64).reshape(-1, 3)
            mp = self._maps[s] = (r[:, 0], r[:, 1])
        return mp

    def to_global(self, s: int, rows: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """local rows of shard s -> global rows (vectorised; padding -1 stays -1).  ``out`` may be ``rows`` itself."""
        rows = np.asarray(rows)
        g0, l0 = self._map(s)
        if out is None:
            out = np.empty(rows.shape, np.int64)
        if len(g0) == 1 and g0[0] == l0[0]:          # identity (one shard, or shard 0 after a reservation): padding is -1 already
            if out is not rows:
                out[...] = rows
            return out
        pad = rows < 0
        if len(g0) == 1:
            np.add(rows, g0[0] - l0[0], out=out)
        elif len(g0) == 0:
            out[...] = -1
            return out
        else:
            j = np.searchsorted(l0, rows, side="right") - 1
            np.maximum(j, 0, out=j)
            np.add(rows, g0[j] - l0[j], out=out)
        out[pad] = -1
        return out

    def global_runs(self):
        """[(global_start, shard, local_start, count)] in global order"""
        if self._sorted is None:
            self._sorted = sorted((g0, s, l0, c) for s in range(self.world) for g0, l0, c in self.runs[s])
        return self._sorted


# ---- the shard group behind MultiDeviceIndexer.index ---------------------------------------------------------------------------------------------------
class _Call:
    """one outstanding group search: its buffers (taken from the pool until finished) and which shards hold a C-side call for it"""
    __slots__ = ("key", "bufs", "nq", "k", "out", "shards", "partial", "keep")


class ShardGroup:
    """The object behind ``MultiDeviceIndexer.index``: the ``FlatIPIndex`` surface the reference and this package touch (``ntotal`` (global), ``d``,
    ``coarse_dtype``, ``reserve``, ``add``, ``search``, ``search_async`` / ``finish_one`` / ``finish``, ``reconstruct_n``, ``prepare``, ``stats``) over
    ``len(devices)`` ``FlatIPIndex`` shards.  ``device`` is the first shard's GPU (where ``Indexer``'s pipeline stages host queries)."""

    is_trained = True
    MAX_OUTSTANDING = 8         # group calls in flight (each holds one C-side call per shard; a handle keeps at most 16)

    def __init__(self, d: int, devices, coarse_dtype: str = "bf16", shards=None):
        self.d = int(d)
        self.devices = [int(v) for v in devices]
        if not self.devices:
            raise ValueError("MultiDeviceIndexer needs at least one device")
        self.coarse_dtype = coarse_dtype
        self.device = self.devices[0]
        self.distinct = list(dict.fromkeys(self.devices))
        self.shards = list(shards) if shards is not None else [FlatIPIndex(self.d, device=v, coarse_dtype=coarse_dtype) for v in self.devices]
        self.placement = RowPlacement(len(self.devices))
        self._streams = None
        self._pool = {}
        self._outstanding = []

    @property
    def world(self) -> int:
        return len(self.shards)

    @property
    def ntotal(self) -> int:
        return self.placement.ntotal

    def reserve(self, n_rows: int) -> None:
        for sh, rows in zip(self.shards, self.placement.reserve(n_rows)):
            if rows > sh.ntotal:
                sh.reserve(rows)

    def add(self, x) -> None:
        """append rows in global order: each piece goes to its shard (device tensors device-to-device, ordered behind the producer's stream)"""
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"expected [n,{self.d}] embeddings, got {tuple(x.shape)}")
        for s, o, c in self.placement.place(int(x.shape[0])):
            piece = x[o:o + c]
            if not isinstance(piece, np.ndarray) and getattr(piece, "is_cuda", False) and piece.device.index != self.devices[s]:
                import torch
                piece = piece.to(torch.device("cuda", self.devices[s]))
            self.shards[s].add(piece)

    def prepare(self, nq: int = 1, k: int = 10, min_rows: int = 1) -> None:
        for sh in self.shards:
            if sh.ntotal >= max(1, min_rows):
                sh.prepare(nq, k)

    def stats(self, reset: bool = False) -> dict:
        """per-shard ``kr_search_stats`` summed (the ``last_*_ms`` timings: the slowest shard's)"""
        out = None
        for st in self.shard_stats(reset):
            if out is None:
                out = dict(st)
                continue
            for f, v in st.items():
                out[f] = max(out[f], v) if f.startswith("last_") else out[f] + v
        return out

    def shard_stats(self, reset: bool = False) -> List[dict]:
        return [sh.stats(reset) for sh in self.shards]

    def pending(self) -> List[int]:
        lib = _lib.load()
        return [int(lib.kr_index_search_pending(sh._h)) for sh in self.shards]

    def reconstruct_n(self, start: int, n: int) -> np.ndarray:
        """fp32 rows [start, start + n) in global order, read shard-run by shard-run"""
        import bisect
        start, n = int(start), int(n)
        out = np.empty((n, self.d), np.float32)
        runs = self.placement.global_runs()
        j = max(0, bisect.bisect_right(runs, (start, self.world)) - 1)
        for g0, s, l0, c in runs[j:]:
            if g0 >= start + n:
                break
            a, b = max(start, g0), min(start + n, g0 + c)
            if a < b:
                out[a - start:b - start] = self.shards[s].reconstruct_n(l0 + a - g0, b - a)
        return out

    # ---- search ----------------------------------------------------------------------------------------------------------------------------------
    def search(self, q, k: int):
        """(scores float32 [nq,k], GLOBAL rows int64 [nq,k]) of one block of queries (numpy, or a torch tensor on any device)"""
        k = self._check_k(k)
        if self.world == 1:                  # one shard: nothing to orchestrate
            s, i = self.shards[0].search(q, k)
            return s, self.placement.to_global(0, i, out=i)
        nq = int(q.shape[0])
        scores = np.empty((nq, k), np.float32); rows = np.empty((nq, k), np.int64)
        self.search_async(q, k, scores, rows)
        self.finish_one()
        return scores, rows

    def _check_k(self, k) -> int:
        k = int(k)
        if not 0 < k <= min(self.ntotal, 1024):
            raise ValueError(f"top_docs={k} must satisfy 0 < k <= min(ntotal={self.ntotal}, 1024)")
        return k

    def _stream_of(self, s: int):
        import torch
        if self._streams is None:
            self._streams = [torch.cuda.Stream(device=v) for v in self.devices]
            self._dev_streams = {v: torch.cuda.Stream(device=v) for v in self.distinct}
        return self._streams[s]

    def _buffers(self, nq: int, k: int, nfull: int, host_q: bool):
        """a free buffer set for an (nq, k) call: pinned per-shard lists [W, nq, k], the pinned query stage, the queries on every device and the
        gathered coarse block [nfull, nq, k + 1] + theta of the exchange-first split (persistent: taken while a call is outstanding)"""
        import torch
        key = (nq, k, nfull)
        free = self._pool.setdefault(key, [])
        b = free.pop() if free else {}
        if "ps" not in b:
            W = self.world
            b["ps"] = torch.empty((W, nq, k), dtype=torch.float32, pin_memory=True)
            b["pi"] = torch.empty((W, nq, k), dtype=torch.int64, pin_memory=True)
            b["qdev"] = {v: torch.empty((nq, self.d), dtype=torch.float32, device=torch.device("cuda", v)) for v in self.distinct}
            if nfull >= 2:
                b["tk"] = {v: torch.empty((nfull, nq, k + 1), dtype=torch.float32, device=torch.device("cuda", v)) for v in self.distinct}
                b["theta"] = [torch.empty((nq,), dtype=torch.float32, device=torch.device("cuda", v)) for v in self.devices]
        if host_q and "stage" not in b:
            b["stage"] = torch.empty((nq, self.d), dtype=torch.float32, pin_memory=True)
        return key, b

    def _queries(self, q, b):
        """the block's queries on every distinct device -> {device: (contiguous float32 tensor, event after which it is there)}; host queries go through
        ONE pinned stage, a device tensor is used where it is and peer-copied to the other devices (ordered behind its producer's stream)"""
        import torch
        out = {}
        if torch.is_tensor(q) and q.is_cuda:
            src = q.device.index
            qf = q.detach().to(dtype=torch.float32).contiguous()
            for v in self.distinct:
                if v == src:
                    ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(src))
                    out[v] = (qf, ev)
                    continue
                ds = self._dev_streams[v]
                with torch.cuda.stream(ds):
                    b["qdev"][v].copy_(qf, non_blocking=True)
                    ev = torch.cuda.Event(); ev.record(ds)
                out[v] = (b["qdev"][v], ev)
            return out
        host = q.detach().numpy() if torch.is_tensor(q) else q
        stage = b["stage"]
        stage.numpy()[:] = host
        for v in self.distinct:
            ds = self._dev_streams[v]
            with torch.cuda.stream(ds):
                b["qdev"][v].copy_(stage, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(ds)
            out[v] = (b["qdev"][v], ev)
        return out

    def search_async(self, q, k: int, scores_out, rows_out) -> None:
        """Enqueue one block on EVERY shard before waiting on any (each shard on its own stream); ``finish_one()`` makes the oldest block final in
        ``scores_out`` / ``rows_out`` (host arrays or CPU tensors [nq, k]).  Blocks of ``EXCHANGE_FIRST_MIN_NQ``..1024 queries take the exchange-first split
        (coarse scan on every shard -> the shards' k best coarse scores gathered once per device -> global theta -> re-rank above it), smaller ones the
        plain enqueue-only search; a shard with fewer than k rows contributes all it has, an empty one nothing."""
        import torch
        k = self._check_k(k)
        nq = int(q.shape[0])
        if q.ndim != 2 or q.shape[1] != self.d or nq == 0:
            raise ValueError(f"expected [nq>0,{self.d}] queries, got {tuple(q.shape)}")
        if len(self._outstanding) >= self.MAX_OUTSTANDING:
            raise RuntimeError("too many group searches outstanding: finish_one() first")
        self._stream_of(0)
        full = [s for s, sh in enumerate(self.shards) if sh.ntotal >= k]
        partial = [s for s, sh in enumerate(self.shards) if 0 < sh.ntotal < k]
        exchange = len(full) >= 2 and ShardedSearcher.EXCHANGE_FIRST_MIN_NQ <= nq <= 1024
        host_q = not (torch.is_tensor(q) and q.is_cuda)
        key, b = self._buffers(nq, k, len(full) if exchange else 0, host_q)
        call = _Call()
        call.key, call.bufs, call.nq, call.k = key, b, nq, k
        call.out = (scores_out.numpy() if torch.is_tensor(scores_out) else scores_out, rows_out.numpy() if torch.is_tensor(rows_out) else rows_out)
        call.shards, call.partial, call.keep = [], {}, None
        self._outstanding.append(call)
        try:
            self._enqueue(call, q, full, partial, exchange)
        except BaseException:
            self.finish_quietly()
            raise

    def _enqueue(self, call, q, full, partial, exchange):
        import torch
        b, nq, k = call.bufs, call.nq, call.k
        ps, pi = b["ps"], b["pi"]
        qs = self._queries(q, b)
        call.keep = qs
        for s in range(self.world):
            if self.shards[s].ntotal == 0:          # contributes nothing: padding in its list
                ps[s].fill_(float("-inf")); pi[s].fill_(-1)
        for s in full + partial:
            self._stream_of(s).wait_event(qs[self.devices[s]][1])
        if exchange:
            tk = {v: t.view(-1)[: len(full) * nq * (k + 1)].view(len(full), nq, k + 1) for v, t in b["tk"].items()}
            ev_c = {}
            for i, s in enumerate(full):
                v, st = self.devices[s], self._stream_of(s)
                with torch.cuda.stream(st):
                    call.shards.append(s)
                    self.shards[s].search_coarse_async(qs[v][0], k, tk[v][i])
                    ev_c[s] = torch.cuda.Event(); ev_c[s].record(st)
            # every device that re-ranks gets the whole [nshards][nq][k + 1] block once: the other devices' pieces by peer copy, stream-ordered
            ev_g = {}
            for v in dict.fromkeys(self.devices[s] for s in full):
                ds = self._dev_streams[v]
                foreign = [(i, s) for i, s in enumerate(full) if self.devices[s] != v]
                if not foreign:
                    continue
                with torch.cuda.stream(ds):
                    for i, s in foreign:
                        with torch.cuda.stream(self._stream_of(s)):      # source side: behind shard s's coarse scan
                            tk[v][i].copy_(tk[self.devices[s]][i], non_blocking=True)
                    ev_g[v] = torch.cuda.Event(); ev_g[v].record(ds)
            for s in full:
                v, st = self.devices[s], self._stream_of(s)
                for a in full:
                    if a != s and self.devices[a] == v:
                        st.wait_event(ev_c[a])
                if v in ev_g:
                    st.wait_event(ev_g[v])
                with torch.cuda.stream(st):
                    th = b["theta"][s]
                    self.shards[s].search_global_theta(tk[v].view(len(full) * nq, k + 1), len(full), th)
                    self.shards[s].search_rerank_async(th, ps[s], pi[s])
        else:
            for s in full:
                with torch.cuda.stream(self._stream_of(s)):
                    call.shards.append(s)
                    self.shards[s].search_async(qs[self.devices[s]][0], k, ps[s], pi[s])
        for s in partial:
            kl = self.shards[s].ntotal
            bufs = (torch.empty((nq, kl), dtype=torch.float32, pin_memory=True), torch.empty((nq, kl), dtype=torch.int64, pin_memory=True))
            call.partial[s] = bufs
            with torch.cuda.stream(self._stream_of(s)):
                call.shards.append(s)
                self.shards[s].search_async(qs[self.devices[s]][0], kl, *bufs)

    def finish_one(self) -> int:
        """Finish the OLDEST outstanding group search: each shard's call (queries pass 1 could not certify are re-answered inside the shard's finish),
        then the lists are mapped to global rows and merged into the caller's buffers.  Returns the number of re-answered queries over all shards."""
        if not self._outstanding:
            return 0
        call = self._outstanding[0]
        flagged = 0
        try:
            for s in call.shards:
                flagged += self.shards[s].finish_one()
        except BaseException:
            self.finish_quietly()
            raise
        self._outstanding.pop(0)
        nq, k = call.nq, call.k
        ps, pi = call.bufs["ps"].numpy(), call.bufs["pi"].numpy()
        for s, (bs, bi) in call.partial.items():
            kl = bs.shape[1]
            ps[s, :, :kl] = bs.numpy(); ps[s, :, kl:] = -np.inf
            pi[s, :, :kl] = bi.numpy(); pi[s, :, kl:] = -1
        for s in call.shards:
            self.placement.to_global(s, pi[s], out=pi[s])
        out_s, out_i = call.out
        if self.world == 1:
            out_s[...] = ps[0]; out_i[...] = pi[0]
        else:
            assert out_s.flags.c_contiguous and out_i.flags.c_contiguous and out_s.dtype == np.float32 and out_i.dtype == np.int64
            _lib.check(_lib.load().kr_topk_merge(ps.ctypes.data, pi.ctypes.data, self.world, nq, k, out_s.ctypes.data, out_i.ctypes.data))
        self._pool[call.key].append(call.bufs)
        return flagged

    def finish(self) -> None:
        """Finish everything outstanding on every shard (the error path: nothing stays pending on any handle); the results are dropped."""
        err = None
        for sh in self.shards:
            try:
                sh.finish()
            except Exception as e:          # noqa: BLE001 - the first error is raised after every shard is drained
                err = err or e
        for call in self._outstanding:
            self._pool[call.key].append(call.bufs)
        self._outstanding = []
        if err is not None:
            raise err

    def finish_quietly(self) -> None:
        """``finish()`` on the way out of another error: that error is the one the caller sees"""
        try:
            self.finish()
        except Exception:
            pass


# ---- the Indexer -----------------------------------------------------------------------------------------------------------------------------------
class MultiDeviceIndexer(Indexer):
    """``Indexer`` whose rows are split over ``devices`` (GPU ordinals, repeats allowed; None: every visible device) and driven from ONE process.
    Same surface and same results as the one-device ``Indexer`` fed the same ``index_data`` calls (ids, order, score bits, ties included); ``index`` is a
    ``ShardGroup`` (``ntotal`` is the GLOBAL row count, ``stats()`` the shards' sums, ``shard_stats()`` one dict per shard)."""

    def __init__(self, vector_sz, metric="inner_product", n_subquantizers=0, n_bits=8, devices=None, coarse_dtype="bf16", faiss_padding=False):
        if devices is None:
            import torch
            devices = list(range(torch.cuda.device_count()))
        devices = [int(v) for v in devices]
        if not devices:
            raise ValueError("MultiDeviceIndexer: no device")
        # metric / n_subquantizers are checked by Indexer before any handle exists; the placeholder is replaced right after
        super().__init__(vector_sz, metric=metric, n_subquantizers=n_subquantizers, n_bits=n_bits, coarse_dtype=coarse_dtype,
                         faiss_padding=faiss_padding, local_index=_PLACEHOLDER)
        self.index = ShardGroup(vector_sz, devices, coarse_dtype=coarse_dtype)

    @property
    def devices(self) -> List[int]:
        return list(self.index.devices)

    def _prepare_small_searches(self):
        """``Indexer``'s first-hop rule, per shard: every shard that holds at least ``PREPARE_FROM_ROWS`` rows"""
        self.index.prepare(1, 10, min_rows=self.PREPARE_FROM_ROWS)

    def deserialize_from(self, dir_path):
        """Either format ``Indexer`` / ``ShardedIndexer`` read (the native ``KRSHARD1`` shards when their manifest belongs to ``index_meta.faiss``,
        else ``index.faiss``); shard s loads rows ``shard_range(n, s, W)`` through the readers' ``row_range=``."""
        meta_file = os.path.join(dir_path, "index_meta.faiss")
        manifest = os.path.join(dir_path, SHARD_MANIFEST)
        with open(meta_file, "rb") as reader:
            id_map = pickle.load(reader)
        native = os.path.exists(manifest) and _manifest_matches(manifest, id_map)
        if os.path.exists(manifest) and not native:
            logger.warning(f'{manifest} does not belong to {meta_file} (row count or id-map checksum differ): ignoring the native shards')
        old = self.index
        W = old.world
        shards = []
        for s, v in enumerate(old.devices):
            if native:
                shards.append(read_native_shards(dir_path, device=v, coarse_dtype=old.coarse_dtype, row_range=(s, W)))
            else:
                shards.append(read_faiss_flat_ip(os.path.join(dir_path, "index.faiss"), device=v, coarse_dtype=old.coarse_dtype, row_range=(s, W)))
        group = ShardGroup(old.d, old.devices, coarse_dtype=old.coarse_dtype, shards=shards)
        n = shards[0].file_ntotal
        group.placement.load(n)
        assert [sh.ntotal for sh in shards] == group.placement.shard_rows, "shard reader and placement disagree"
        logger.info(f'Loaded {n} rows from {dir_path} into {W} shards on devices {old.devices}')
        assert len(id_map) == n, 'Deserialized index_id_to_db_id should match faiss index size'
        self.index = group
        self.index_id_to_db_id = id_map
        self._prepare_small_searches()


_PLACEHOLDER = object()       # the ``local_index`` handed to Indexer.__init__ (which then creates no handle of its own)


# ---- entry-point switch (retrieve.setup_retriever_model, faiss_index_corpus) ------------------------------------------------------------------------
def parse_index_devices(value) -> Optional[List[int]]:
    """``[0, 1]`` / ``(0, 1)`` / ``"0,1"`` / ``"0 1"`` -> [0, 1]; None or "" -> None"""
    if value is None:
        return None
    if isinstance(value, str):
        parts = [p for p in value.replace(",", " ").split() if p]
        return [int(p) for p in parts] or None
    if isinstance(value, int):
        return [value]
    out = [int(v) for v in value]
    return out or None


def index_devices(args) -> Optional[List[int]]:
    """the devices of a row-sharded single-process index: ``args.index_devices`` when set, else ``KIRAG_AMD_INDEX_DEVICES``; None: one-device ``Indexer``"""
    value = getattr(args, "index_devices", None)
    if value is None:
        value = os.environ.get(ENV_INDEX_DEVICES)
    return parse_index_devices(value)


def make_indexer(args, embedding_size: int, device: Optional[int] = None):
    """``MultiDeviceIndexer`` on ``index_devices(args)`` when given, else today's one-device ``Indexer`` (on ``device``)"""
    devices = index_devices(args)
    if devices is not None:
        logger.info(f"Index rows sharded over devices {devices} (one process)")
        return MultiDeviceIndexer(embedding_size, metric="inner_product", devices=devices)
    return Indexer(embedding_size, metric="inner_product", device=device)
