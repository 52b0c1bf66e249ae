#!/usr/bin/env python3
"""Times kl_maxsim (libkirag_late.so) on one MI355X against a torch yardstick on the same GPU and the same float16 data, and writes
profiles/late/measurements.txt (or --out).

    python tools/late_bench.py [--out FILE] [--rounds 7] [--inner 5] [--small]

One process; per shape the kernel and the yardstick ALTERNATE (kernel, torch, kernel, torch, ...) for --rounds rounds of --inner calls each after two warm-up
rounds; a round is timed with device events around its calls; the figure is the median over rounds of (round time / inner).  Shapes:

  (a) one query of 32 rows x 1000 documents of 128 rows, P = 1024 — bge-m3's rerank.  The 1000 candidates of a call are one of ten disjoint sets of a
      10 000-document store, a different set every call, so that no call finds its 262 MB in the 256 MiB Infinity Cache;
  (b) 100 queries x 100 random candidates each out of those 10 000 documents (2.6 GB of document rows per call);
  (c) P = 128, one 32-row query x 10 000 documents of 180 rows (461 MB) — a ColBERT-style shape.

The yardstick gets the documents ALREADY padded into [C, S, P] (for (b): gathered into [100, 100, S, P]) outside the timed region and runs
matmul -> amax -> mean.  The byte floor is document bytes / time, for information (6.3 TB/s is the achievable HBM copy rate of this part).  The last section
times what the store replaces: the MaxSim stage of BGEM3Model.rerank over 64 passages (one colbert_score call per pair from host arrays) against
store.rerank over the same vectors.  Refuses to run without a GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def unit_f16(n, P, gen):
    x = torch.randn((n, P), generator=gen, device="cuda", dtype=torch.float32)
    return torch.nn.functional.normalize(x, dim=-1).to(torch.float16)


def timed_rounds(fns, rounds, inner, warm=2):
    """fns: callables taking the call number; returns per fn the list of per-call milliseconds, one entry per round, the fns alternating inside a round"""
    out = [[] for _ in fns]
    call = 0
    for r in range(warm + rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(inner):
                fn(call + i)
            b.record()
            b.synchronize()
            if r >= warm:
                out[k].append(a.elapsed_time(b) / inner)
        call += inner
    return out


class Direct:
    """kl_maxsim through ctypes on prepared host arrays: the library's own time (validation, upload of the pair arrays, launch)"""
    def __init__(self, lib, q, q_off, d, d_off, P):
        self.lib, self.q, self.d, self.P = lib, q, d, P
        self.q_off, self.d_off = np.ascontiguousarray(q_off, np.int64), np.ascontiguousarray(d_off, np.int64)

    def __call__(self, pair_q, pair_d, out):
        from kirag_amd import _late_lib
        _late_lib.check(self.lib.kl_maxsim(self.q.data_ptr(), self.q_off.ctypes.data, len(self.q_off) - 1, self.d.data_ptr(), self.d_off.ctypes.data,
                                           len(self.d_off) - 1, pair_q.ctypes.data, pair_d.ctypes.data, len(pair_q), self.P, 1, out.data_ptr(), 0,
                                           int(torch.cuda.current_stream().cuda_stream)))


def yardstick(q, docs):
    """q [..., Lq, P], docs [..., C, S, P] float16 -> [..., C] float32: matmul -> amax -> mean"""
    s = torch.matmul(q.unsqueeze(-3), docs.transpose(-1, -2))
    return s.amax(dim=-1).float().mean(dim=-1)


def report(lines, name, doc_bytes, t_kernel, t_torch, diff):
    mk, mt = statistics.median(t_kernel), statistics.median(t_torch)
    lines.append(f"{name}")
    lines.append(f"    kl_maxsim   median {mk:9.4f} ms   (min {min(t_kernel):.4f}, max {max(t_kernel):.4f}; {len(t_kernel)} rounds)")
    lines.append(f"    torch       median {mt:9.4f} ms   (min {min(t_torch):.4f}, max {max(t_torch):.4f})")
    lines.append(f"    torch / kl_maxsim = {mt / mk:.2f}   document bytes {doc_bytes / 1e6:.1f} MB -> {doc_bytes / mk / 1e9:.3f} TB/s over the kernel's call time "
                 f"(6.3 TB/s copy rate: {100 * doc_bytes / mk / 1e9 / 6.3:.0f} %)")
    lines.append(f"    worst |kl_maxsim - torch| over the call's scores: {diff:.2e}")
    print("\n".join(lines[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "late", "measurements.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tenth of the documents (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("late_bench.py measures on an MI355X: no GPU found")
    from kirag_amd import _late_lib
    from kirag_amd.retriever.late import MultiVectorStore
    from kirag_amd.retriever.m3 import colbert_score
    lib = _late_lib.load()
    gen = torch.Generator(device="cuda").manual_seed(1)
    scale = 10 if args.small else 1
    lines = [f"tools/late_bench.py --rounds {args.rounds} --inner {args.inner}{' --small' if args.small else ''} on {torch.cuda.get_device_name(0)}",
             "per-call milliseconds: median over rounds of (device-event time of a round / calls in it); kernel and yardstick alternate", ""]

    # ---- (a) and (b): P = 1024, 10 000 documents of 128 rows ----
    P, S, N, Lq = 1024, 128, 10000 // scale, 32
    docs = unit_f16(N * S, P, gen)                                    # [N * S, P]: the store's layout; seen as [N, S, P] it is the yardstick's padded tensor
    d_off = np.arange(N + 1, dtype=np.int64) * S
    queries = unit_f16(100 * Lq, P, gen)
    q_off = np.arange(101, dtype=np.int64) * Lq
    direct = Direct(lib, queries, q_off, docs, d_off, P)
    C = 1000 // scale
    sets = N // C
    out_a = torch.empty(C, dtype=torch.float32, device="cuda")
    pq_a = np.zeros(C, np.int64)
    pd_sets = [np.arange(k * C, (k + 1) * C, dtype=np.int64) for k in range(sets)]
    padded = docs.view(N, S, P)
    q0 = queries[:Lq]
    res_t = {}
    k_fn = lambda i: direct(pq_a, pd_sets[i % sets], out_a)
    t_fn = lambda i: res_t.__setitem__("a", yardstick(q0, padded[(i % sets) * C:(i % sets + 1) * C]))
    tk, tt = timed_rounds([k_fn, t_fn], args.rounds, args.inner)
    k_fn(0); t_fn(0)
    report(lines, f"(a) 1 query x {Lq} rows, {C} documents x {S} rows, P = {P} (one of {sets} disjoint candidate sets per call)", C * S * P * 2, tk, tt,
           float((out_a - res_t["a"]).abs().max()))

    nq_b, c_b = 100, 100 // scale if args.small else 100
    rng = np.random.default_rng(2)
    cand = rng.integers(0, N, size=(nq_b, c_b))
    pq_b = np.repeat(np.arange(nq_b, dtype=np.int64), c_b)
    pd_b = np.ascontiguousarray(cand.reshape(-1), dtype=np.int64)
    out_b = torch.empty(nq_b * c_b, dtype=torch.float32, device="cuda")
    gathered = padded[torch.from_numpy(cand).cuda()]                  # [100, 100, S, P], outside the timed region
    qs = queries.view(nq_b, Lq, P)
    k_fn = lambda i: direct(pq_b, pd_b, out_b)
    t_fn = lambda i: res_t.__setitem__("b", yardstick(qs, gathered))
    tk, tt = timed_rounds([k_fn, t_fn], args.rounds, max(1, args.inner // 2))
    report(lines, f"(b) {nq_b} queries x {Lq} rows, {c_b} random candidates each out of {N} documents x {S} rows, P = {P}", nq_b * c_b * S * P * 2, tk, tt,
           float((out_b.view(nq_b, c_b) - res_t["b"]).abs().max()))
    del gathered, res_t["b"]

    # ---- what the store replaces: 64 passages, per-pair host path against store.rerank ----
    store = MultiVectorStore(P, device="cuda:0")
    lens = rng.integers(20, 129, size=64)
    host_p = [docs[k * S:k * S + int(n)].float().cpu().numpy() for k, n in enumerate(lens)]
    host_q = q0.float().cpu().numpy()
    ids = [str(k) for k in range(64)]
    store.add(ids, host_p)
    host_ms, store_ms = [], []
    for r in range(2 + args.rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ref = [colbert_score(host_q, p, "cuda") for p in host_p]
        torch.cuda.synchronize(); t1 = time.perf_counter()
        got = store.rerank(host_q, ids)
        t2 = time.perf_counter()
        if r >= 2:
            host_ms.append(1e3 * (t1 - t0)); store_ms.append(1e3 * (t2 - t1))
    order = np.lexsort((np.arange(64), -np.asarray(ref)))
    lines += ["", "MaxSim stage over 64 passages of 20 .. 128 rows, P = 1024, one 32-row query (host clock, ends in a device synchronise / a copy to the host)",
              f"    BGEM3Model.rerank's stage: 64 x colbert_score from host arrays   median {statistics.median(host_ms):8.3f} ms",
              f"    MultiVectorStore.rerank over the stored vectors               median {statistics.median(store_ms):8.3f} ms",
              f"    same order: {[ids[i] for i in order] == got[0]}; worst |score difference| {float(np.abs(np.asarray(ref)[order] - got[1]).max()):.2e}"]
    print("\n".join(lines[-4:]), flush=True)
    del store, docs, padded, queries, direct

    # ---- (c): P = 128, 10 000 documents of 180 rows ----
    P, S, N = 128, 180, 10000 // scale
    docs = unit_f16(N * S, P, gen)
    d_off = np.arange(N + 1, dtype=np.int64) * S
    q0 = unit_f16(Lq, P, gen)
    direct = Direct(lib, q0, np.array([0, Lq], np.int64), docs, d_off, P)
    out_c = torch.empty(N, dtype=torch.float32, device="cuda")
    pq_c, pd_c = np.zeros(N, np.int64), np.arange(N, dtype=np.int64)
    padded = docs.view(N, S, P)
    k_fn = lambda i: direct(pq_c, pd_c, out_c)
    t_fn = lambda i: res_t.__setitem__("c", yardstick(q0, padded))
    tk, tt = timed_rounds([k_fn, t_fn], args.rounds, args.inner)
    lines.append("")
    report(lines, f"(c) 1 query x {Lq} rows, {N} documents x {S} rows, P = {P}", N * S * P * 2, tk, tt, float((out_c - res_t["c"]).abs().max()))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
