#!/usr/bin/env python3
"""Times ks_search (libkirag_sparse.so) on one MI355X over a synthetic Zipf corpus against a torch yardstick on the same GPU and the same float16-rounded
data, and appends a section to profiles/sparse/measurements.txt (or --out).

    python tools/sparse_bench.py [--out FILE] [--rows 1000000] [--vocab 30522] [--draws 165] [--rounds 5] [--no-yardstick] [--no-model]

One process; per shape the kernel and the yardstick ALTERNATE for --rounds rounds after one warm-up round; a call is timed with device events around it; the
figure is the median over rounds.  The library under test is the one ``kirag_amd._sparse_lib`` loads (``KIRAG_SPARSE_LIB`` selects another build, e.g. the
other block size R); the section's title says which R it is.

Corpus: rows of ``--draws`` draws from p(t) ~ 1 / (t + 10) over the vocabulary, duplicates merged (about 150 terms a row at the defaults), uniform weights
rounded to float16; queries of 30 distinct draws from the same law.  Yardstick: ``torch.sparse_csr_tensor(corpus) @ dense queries`` then ``topk``; when
torch's sparse product does not run on this device the tool says so.  Also timed: the host inversion per block while the index is built, the ingest of a
``[64, V]`` block through ``index_block``, and (with the synthetic SPLADE model of the tests, unless --no-model) ``SpladeModel.rerank`` over 64 passages next
to ``retrieve`` over an index holding them.  Refuses to run without a GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def zipf_cdf(V):
    p = 1.0 / (np.arange(V) + 10.0)
    return np.cumsum(p / p.sum())


def zipf_rows(cdf, n, draws, rng):
    """n rows of `draws` draws, duplicates merged: (counts [n], terms int32 ascending within a row)"""
    t = np.searchsorted(cdf, rng.random((n, draws))).astype(np.int32)
    np.minimum(t, len(cdf) - 1, out=t)
    t.sort(axis=1)
    keep = np.ones_like(t, bool)
    keep[:, 1:] = t[:, 1:] != t[:, :-1]
    return keep.sum(axis=1).astype(np.int64), t[keep]


def build_index(V, N, draws, seed=1):
    """a SparseIndexer on the GPU filled block by block through its commit step (the per-passage Python loop of index_data is not what is measured here);
    returns (index, seconds spent inverting and uploading, blocks inverted)"""
    from kirag_amd.retriever.sparse_index import SparseIndexer
    ix = SparseIndexer(V, device="cuda:0")
    cdf, rng = zipf_cdf(V), np.random.default_rng(seed)
    spent, blocks = 0.0, 0
    inner = ix._invert_into

    def timed(*a):
        nonlocal spent, blocks
        t0 = time.perf_counter()
        inner(*a)
        torch.cuda.synchronize()
        spent += time.perf_counter() - t0
        blocks += 1
    ix._invert_into = timed
    step = ix.block_rows
    for r0 in range(0, N, step):
        n = min(step, N - r0)
        counts, terms = zipf_rows(cdf, n, draws, rng)
        w16 = rng.uniform(0.05, 3.0, len(terms)).astype(np.float32).astype(np.float16)
        ix._commit(np.arange(r0, r0 + n, dtype=np.int64), counts, terms, w16)
    ix._sync_tail()
    ix._invert_into = inner
    return ix, spent, blocks


def zipf_queries(V, nq, terms, seed):
    cdf, rng = zipf_cdf(V), np.random.default_rng(seed)
    out = []
    for _ in range(nq):
        t = np.unique(np.minimum(np.searchsorted(cdf, rng.random(2 * terms)), V - 1))
        t = np.sort(rng.permutation(t)[:terms]).astype(np.int32)
        out.append((t, rng.uniform(0.1, 2.0, len(t)).astype(np.float32)))
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def visited_bytes(ix, queries):
    """posting bytes the scan reads for these queries: 4 bytes x the postings under each query term, summed over the blocks"""
    df = np.bincount(ix.terms, minlength=ix.vocab_size)
    return 4 * int(sum(int(df[t].sum()) for t, _ in queries))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse", "measurements.txt"))
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--draws", type=int, default=165)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_bench.py measures on an MI355X: no GPU found")
    from kirag_amd import _sparse_lib
    R = _sparse_lib.block_rows()
    V, N = args.vocab, args.rows
    lines = [f"tools/sparse_bench.py --rows {N} --vocab {V} --draws {args.draws} --rounds {args.rounds} on {torch.cuda.get_device_name(0)}, R = {R}",
             "per-call milliseconds: median over rounds of the device-event time of one call; kernel and yardstick alternate", ""]
    t0 = time.perf_counter()
    ix, spent, blocks = build_index(V, N, args.draws)
    lines.append(f"corpus: {ix.ntotal} rows, {ix.nnz} postings ({ix.nnz / ix.ntotal:.1f} terms a row), built in {time.perf_counter() - t0:.1f} s; host inversion + upload "
                 f"{1e3 * spent / max(blocks, 1):.0f} ms per block of {R} rows ({blocks} blocks)")
    print(lines[-1], flush=True)

    csr = None
    if not args.no_yardstick:
        try:
            crow = torch.from_numpy(ix.row_off.copy()).cuda()
            col = torch.from_numpy(ix.terms.astype(np.int64)).cuda()
            val = torch.from_numpy(ix.weights.astype(np.float32)).cuda()
            csr = torch.sparse_csr_tensor(crow, col, val, size=(N, V), device="cuda")
            _ = (csr @ torch.zeros((V, 1), device="cuda")).sum().item()
        except Exception as e:      # noqa: BLE001  (reported, not hidden: the section says the yardstick did not run)
            csr = None
            lines.append(f"yardstick: torch.sparse_csr_tensor @ dense does not run on this device here: {type(e).__name__}: {str(e)[:200]}")
            print(lines[-1], flush=True)

    for nq in (1, 32, 1000):
        queries = zipf_queries(V, nq, 30, seed=100 + nq)
        dense_q = None
        if csr is not None:
            dq = np.zeros((V, nq), np.float32)
            for j, (t, w) in enumerate(queries):
                dq[t, j] = w
            dense_q = torch.from_numpy(dq).cuda()
        vb = visited_bytes(ix, queries)
        for k in (10, 100):
            res = {}
            tk, tt = [], []
            for r in range(1 + args.rounds):
                a = event_ms(lambda: res.__setitem__("k", ix.search_arrays(queries, k)))
                if csr is not None:
                    b = event_ms(lambda: res.__setitem__("t", torch.topk((csr @ dense_q).t(), k, dim=1)))
                if r >= 1:
                    tk.append(a)
                    if csr is not None:
                        tt.append(b)
            mk = statistics.median(tk)
            lines.append(f"nq = {nq:4d}, k = {k:3d}: search_arrays (query CSR, ks_search, copy back) median {mk:9.3f} ms (min {min(tk):.3f}, max {max(tk):.3f}); "
                         f"postings visited {vb / 1e6:.1f} MB -> {vb / mk / 1e9:.3f} TB/s ({100 * vb / mk / 1e9 / 6.3:.0f} % of the 6.3 TB/s copy rate)")
            if csr is not None:
                mt = statistics.median(tt)
                ts, ti = res["t"]
                same = float((ti.cpu().numpy() == res["k"][1]).mean())
                lines.append(f"{'':19s}torch csr @ dense + topk      median {mt:9.3f} ms (min {min(tt):.3f}, max {max(tt):.3f}); torch / ks_search = {mt / mk:.2f}; "
                             f"rows equal to torch's at {100 * same:.1f} % of the places, worst |score difference| "
                             f"{float(np.abs(ts.cpu().numpy() - res['k'][0]).max()):.2e}")
            print("\n".join(lines[-2:]), flush=True)
    del csr

    # ---- ingest: a [64, V] block through index_block (count, compact, copy of the kept entries, host append) ----
    from kirag_amd.retriever.sparse_index import SparseIndexer
    rng = np.random.default_rng(5)
    block = torch.from_numpy(np.where(rng.random((64, V)) < 150.0 / V, rng.uniform(0.05, 3.0, (64, V)), 0.0).astype(np.float32)).cuda()
    sink = SparseIndexer(V, device="cuda:0")
    times = []
    for r in range(7):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sink.index_block([str(64 * r + i) for i in range(64)], block, skip_terms=(0,))
        times.append(time.perf_counter() - t0)
    lines += ["", f"index_block of a [64, {V}] block with about 150 kept entries a row (host clock): median {1e3 * statistics.median(times[2:]):.3f} ms -> "
                  f"{64 / statistics.median(times[2:]):.0f} passages/s without the forward; the block is {64 * V * 4 / 1e6:.1f} MB, the kept entries "
                  f"{6 * sink.nnz / 7 / 1e3:.1f} KB"]
    print(lines[-1], flush=True)

    # ---- what the index replaces: SpladeModel.rerank over 64 passages next to retrieve over an index holding them (the synthetic model of the tests) ----
    if not args.no_model:
        try:
            sys.path.insert(0, os.path.join(REPO, "tests"))
            import reranker_util as RU
            import splade_util as S
            from kirag_amd.retriever.splade import BertSpladeEncoder, SpladeModel
            tok = RU.bert_pair_tokenizer()
            model = SpladeModel(S.hf_mlm("h64", tok.vocab_size, S.tied_weights(tok.vocab_size), "cuda", cls=BertSpladeEncoder, tie=True), tokenizer=tok)
            query, passages = RU.passages(1, seed=11, lo=8, hi=12)[0], RU.passages(64, seed=12)
            held = SparseIndexer(tok.vocab_size, device="cuda:0")
            t0 = time.perf_counter()
            model.index_passages([str(i) for i in range(64)], passages, held, batch_size=64)
            t_index = time.perf_counter() - t0
            a, b = [], []
            for r in range(7):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                order, _ = model.rerank(query, passages)
                t1 = time.perf_counter()
                got = model.retrieve([query], held, top_k=64)[0]
                t2 = time.perf_counter()
                a.append(1e3 * (t1 - t0)); b.append(1e3 * (t2 - t1))
            lines += ["", f"synthetic SPLADE model (2 layers, H = 128, V = {tok.vocab_size}), 64 passages, one query (host clock):",
                      f"    SpladeModel.rerank (encodes the 64 passages again, dict scoring)   median {statistics.median(a[2:]):8.3f} ms",
                      f"    SpladeModel.retrieve over the index holding them                  median {statistics.median(b[2:]):8.3f} ms",
                      f"    index_passages of the 64 (first call, one forward): {1e3 * t_index:.1f} ms; same first ten: "
                      f"{[str(int(i)) for i in order[:10]] == got[0][:10]}"]
            print("\n".join(lines[-4:]), flush=True)
        except Exception as e:      # noqa: BLE001
            lines += ["", f"SpladeModel.rerank against retrieve: not measured ({type(e).__name__}: {str(e)[:200]})"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
    print("appended to", args.out)


if __name__ == "__main__":
    main()
