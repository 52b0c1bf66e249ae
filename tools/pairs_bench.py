#!/usr/bin/env python3
"""Times SparseIndexer.score_pairs (kp_sparse_dot, libkirag_pairs.so) on one MI355X over the synthetic Zipf corpus of tools/sparse_bench.py against a torch
yardstick on the same GPU and the same float16 data, and appends a section to profiles/pairs/measurements.txt (or --out).

    python tools/pairs_bench.py [--out FILE] [--rows 1000000] [--vocab 30522] [--draws 165] [--rounds 7] [--no-model]

One process; per shape (1 x 100, 100 x 100, 1000 x 100 pairs: queries of 30 terms, 100 random candidate rows each) the calls ALTERNATE for --rounds rounds
after one warm-up round; a call is timed with device events around it; the figure is the median over rounds.  Three things are timed per shape:

  * ``score_rows``: the query CSR, the pair arrays, ``kp_sparse_dot`` (records staged, copied, kernel, wait) and the copy back of the scores — the call with
    its host part, as tools/sparse_bench.py reports ``search_arrays``;
  * ``score_pairs``: the same behind the lookup of 100 id strings per query in the index's id map (a Python loop);
  * the torch yardstick, on the device mirror itself: the query scattered into a dense ``[V]`` fp32 vector, gathered by the candidate rows' terms, multiplied
    by the weights and summed per row segment (``index_add_``).  Its inputs (entry indices, segment ids) are built on the host and uploaded inside the timed
    region, as the kernel's pair records are.

Bytes of row data per call (6 bytes an entry of a candidate row) over the time are reported as a share of the 6.3 TB/s copy rate.  Also timed, with the
synthetic bge-m3 model of the tests unless --no-model: ``compute_lexical_matching_score`` over dicts for 64 passages against ``SparseIndexer.rerank`` over the
same stored rows.  Refuses to run without a GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sparse_bench import build_index, event_ms, zipf_queries  # noqa: E402

COPY_RATE = 6.3e12


def yardstick_batched(ix, queries, rows):
    """fp32 [npairs]: scatter, gather, multiply, segment sum in torch on the index's device mirror, ONE set of launches for all queries of the call (a dense
    [nq, V] query block)"""
    dev = ix.device
    V, nq = ix.vocab_size, len(queries)
    flat = np.concatenate(rows)
    a, b = ix.row_off[flat], ix.row_off[flat + 1]
    n = b - a
    seg = np.repeat(np.arange(len(flat), dtype=np.int64), n)
    ent = np.repeat(a - np.concatenate(([0], np.cumsum(n)[:-1])), n) + np.arange(int(n.sum()), dtype=np.int64)
    qrow = np.repeat(np.repeat(np.arange(nq, dtype=np.int64), [len(r) for r in rows]), n)
    dq = torch.zeros((nq, V), dtype=torch.float32, device=dev)
    qi = np.repeat(np.arange(nq, dtype=np.int64), [len(t) for t, _ in queries])
    dq[torch.from_numpy(qi).to(dev), torch.from_numpy(np.concatenate([t for t, _ in queries]).astype(np.int64)).to(dev)] = \
        torch.from_numpy(np.concatenate([w for _, w in queries])).to(dev)
    ent_d, seg_d, qrow_d = torch.from_numpy(ent).to(dev), torch.from_numpy(seg).to(dev), torch.from_numpy(qrow).to(dev)
    prod = dq[qrow_d, ix._d_terms[ent_d].long()] * ix._d_weights[ent_d].float()
    return torch.zeros(len(flat), dtype=torch.float32, device=dev).index_add_(0, seg_d, prod).cpu().numpy()


def bench_corpus(V, N, draws, rounds, lines):
    t0 = time.perf_counter()
    ix, _, _ = build_index(V, N, draws)
    t1 = time.perf_counter()
    ix._sync_mirror()
    torch.cuda.synchronize()
    lines.append(f"corpus: V = {V}, {ix.ntotal} rows, {ix.nnz} entries ({ix.nnz / ix.ntotal:.1f} terms a row), built in {t1 - t0:.1f} s; the device mirror "
                 f"({6 * ix.nnz / 1e6:.0f} MB) uploaded in {time.perf_counter() - t1:.2f} s")
    print(lines[-1], flush=True)
    for nq in (1, 100, 1000):
        queries = zipf_queries(V, nq, 30, seed=100 + nq)
        rng = np.random.default_rng(nq)
        rows = [rng.integers(0, ix.ntotal, 100).astype(np.int64) for _ in range(nq)]
        ids = [[str(int(i)) for i in ix.ids[r]] for r in rows]
        row_bytes = 6 * int(sum(int((ix.row_off[r + 1] - ix.row_off[r]).sum()) for r in rows))
        res, times = {}, {"rows": [], "pairs": [], "torch": []}
        for r in range(1 + rounds):
            a = event_ms(lambda: res.__setitem__("rows", ix.score_rows(queries, rows)))
            b = event_ms(lambda: res.__setitem__("pairs", ix.score_pairs(queries, ids)))
            c = event_ms(lambda: res.__setitem__("torch", yardstick_batched(ix, queries, rows)))
            if r >= 1:
                times["rows"].append(a); times["pairs"].append(b); times["torch"].append(c)
        med = {k: statistics.median(v) for k, v in times.items()}
        flat = np.concatenate(res["rows"])
        assert np.array_equal(flat.view(np.uint32), np.concatenate(res["pairs"]).view(np.uint32))
        rate = row_bytes / (med["rows"] * 1e-3)
        lines.append(f"{nq:4d} x 100 pairs: score_rows (query CSR, kp_sparse_dot, copy back) median {med['rows']:8.3f} ms (min {min(times['rows']):.3f}, max "
                     f"{max(times['rows']):.3f}); row data {row_bytes / 1e6:.2f} MB -> {rate / 1e9:.2f} GB/s ({100 * rate / COPY_RATE:.2f} % of the 6.3 TB/s copy rate)")
        lines.append(f"{'':17s}score_pairs (the same behind the id lookup)           median {med['pairs']:8.3f} ms (min {min(times['pairs']):.3f}, max "
                     f"{max(times['pairs']):.3f})")
        lines.append(f"{'':17s}torch scatter / gather / index_add_ (one batch)       median {med['torch']:8.3f} ms (min {min(times['torch']):.3f}, max "
                     f"{max(times['torch']):.3f}); torch / score_rows = {med['torch'] / med['rows']:.2f}; worst |score difference| "
                     f"{float(np.abs(res['torch'] - flat).max()):.2e}, {100 * float((res['torch'].view(np.uint32) == flat.view(np.uint32)).mean()):.1f} % of the scores equal bit for bit")
        print("\n".join(lines[-3:]), flush=True)
    # the kernel without the call's host part: device events around kp_sparse_dot alone are not available from outside the library (it waits for its
    # stream), so the host clock around the C call is what can be said
    from kirag_amd import _pairs_lib
    lib = _pairs_lib.load()
    q_off, q_term, q_w = ix._queries_csr(queries)
    pair_q = np.repeat(np.arange(nq, dtype=np.int64), 100)
    pair_row = np.ascontiguousarray(np.concatenate(rows))
    out = torch.empty(len(pair_q), dtype=torch.float32, device=ix.device)
    stream = int(torch.cuda.current_stream(ix.device).cuda_stream)
    calls = []
    for r in range(1 + rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _pairs_lib.check(lib.kp_sparse_dot(ix._d_terms.data_ptr(), ix._d_weights.data_ptr(), ix.nnz, ix._row_off.ctypes.data, ix.ntotal, V, q_off.ctypes.data, nq,
                                           q_term.ctypes.data, q_w.ctypes.data, pair_q.ctypes.data, pair_row.ctypes.data, len(pair_q), out.data_ptr(), 0, stream))
        calls.append(1e3 * (time.perf_counter() - t0))
    m = statistics.median(calls[1:])
    lines.append(f"{'':17s}kp_sparse_dot alone at 1000 x 100 (host clock around the C call: checks, records, copy, kernel, wait) median {m:.3f} ms -> "
                 f"{row_bytes / m / 1e6:.2f} GB/s ({100 * row_bytes / (m * 1e-3) / COPY_RATE:.2f} % of the copy rate)")
    print(lines[-1], flush=True)
    lines.append("")
    del ix
    torch.cuda.empty_cache()


def bench_model(lines):
    """what score_pairs replaces: the dict loop of compute_score / rerank over 64 passages next to SparseIndexer.rerank over the same stored rows"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import m3_util as M
    import xlmr_util as X
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.late import MultiVectorStore
    from kirag_amd.retriever.m3 import BGEM3Model, XLMRobertaM3Encoder, compute_lexical_matching_score
    from kirag_amd.retriever.sparse_index import SparseIndexer
    P = 128
    hw = M.heads_for("xlmr", P)
    enc = M.hf_backbone("xlmr", M.backbone("xlmr"), "cuda", cls=XLMRobertaM3Encoder)
    enc.set_heads({"weight": torch.from_numpy(hw[M.HEADS[0]]), "bias": torch.from_numpy(hw[M.HEADS[1]])},
                  {"weight": torch.from_numpy(hw[M.HEADS[2]]), "bias": torch.from_numpy(hw[M.HEADS[3]])})
    tok = X.toy_tokenizer()
    m3 = BGEM3Model(enc, tokenizer=tok)
    passages, query = M.texts(64, seed=5, lo=3, hi=24), M.texts(1, seed=105, lo=6, hi=16)[0]
    ids = [str(i) for i in range(64)]
    indexer, store, sp = Indexer(128), MultiVectorStore(P, device="cuda:0"), SparseIndexer(len(tok), device="cuda:0")
    m3.index_passages(ids, passages, indexer, store, batch_size=64, sparse_index=sp)
    lex_q = m3.encode([query], return_dense=False, return_sparse=True)["lexical_weights"][0]
    lex_p = m3.encode(passages, batch_size=64, return_dense=False, return_sparse=True)["lexical_weights"]
    a, b, c = [], [], []
    for r in range(9):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loop = [compute_lexical_matching_score(lex_q, p) for p in lex_p]
        t1 = time.perf_counter()
        got_ids, got = sp.rerank(lex_q, ids)
        t2 = time.perf_counter()
        m3.encode(passages, batch_size=64, return_dense=False, return_sparse=True)
        t3 = time.perf_counter()
        a.append(1e3 * (t1 - t0)); b.append(1e3 * (t2 - t1)); c.append(1e3 * (t3 - t2))
    by_id = dict(zip(got_ids, got.tolist()))
    worst = max(abs(by_id[i] - s) for i, s in zip(ids, loop))
    lines += [f"synthetic bge-m3 model (xlmr backbone of the tests, V = {len(tok)}), 64 passages, one query (host clock):",
              f"    compute_lexical_matching_score over 64 dict pairs (the passages' dicts at hand)   median {statistics.median(a[2:]):8.3f} ms",
              f"    encoding the 64 passages' lexical weights again, which compute_score / rerank do   median {statistics.median(c[2:]):8.3f} ms",
              f"    SparseIndexer.rerank over the same 64 stored rows (lookup, kp_sparse_dot, sort)    median {statistics.median(b[2:]):8.3f} ms",
              f"    worst |dict score - stored-row score| {worst:.2e} (the stored weights are rounded to float16)", ""]
    print("\n".join(lines[-6:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pairs", "measurements.txt"))
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--draws", type=int, default=165)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pairs_bench.py measures on an MI355X: no GPU found")
    lines = [f"tools/pairs_bench.py --rows {args.rows} --vocab {args.vocab} --draws {args.draws} --rounds {args.rounds} on {torch.cuda.get_device_name(0)}",
             "per-call milliseconds: median over rounds of the device-event time of one call; score_rows, score_pairs and the yardstick alternate", ""]
    bench_corpus(args.vocab, args.rows, args.draws, args.rounds, lines)
    if not args.no_model:
        try:
            bench_model(lines)
        except Exception as e:      # noqa: BLE001  (reported, not hidden)
            lines += [f"dict loop against SparseIndexer.rerank: not measured ({type(e).__name__}: {str(e)[:200]})", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("appended to", args.out)


if __name__ == "__main__":
    main()
