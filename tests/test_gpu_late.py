"""GPU tests of libkirag_late.so and of what stands on it (kirag_amd.retriever.late.MultiVectorStore, BGEM3Model.index_passages / retrieve).

kl_maxsim against the float64 reference of tests/late_util.py on the same float16 operands: bit for bit on integer-exact operands over every pair of the
row counts {1, 5, 32, 33, 70} x {0, 1, 31, 32, 33, 64, 65, 200} at P = 32 / 96 / 128 / 256 / 1024 and both reduces; within the derived bound
(late_util.kernel_bound) where ONE token decides the score (document rows 0 / 31 / 32 / last / last of a ragged tail, all-negative products, query rows
31 / 32 / last) and on random unit rows; against the UNROUNDED rows within the derived float16 bound, below the project's 1e-3.  A pair's bits do not
depend on its company.  Guard words around every output.  kl_gather_rows_f16 gives torch's float16 bits.  End to end on the synthetic M3 handles of
tests/m3_util.py against HF fp32 + the heads in float64.

Measured on one MI355X (profiles/late/measurements.txt, section 4; the tests print the figures under -s): worst |kernel - float64| / derived bound on random
unit rows 0.006 at P = 128, 0.001 at 256, below 0.0005 at 1024; end to end worst |score - reference| 3.8e-5 against the bar of 1e-3, 3 - 4 of 44
neighbouring reference pairs closer than 2e-3."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import late_util as U  # noqa: E402
import m3_util as M  # noqa: E402
import xlmr_util as X  # noqa: E402

pytestmark = pytest.mark.gpu

KL_ERANGE = -34


@functools.lru_cache(maxsize=None)
def lib():
    from kirag_amd import _late_lib
    return _late_lib.load()


def all_pairs(nq, nd):
    pq, pd = np.meshgrid(np.arange(nq), np.arange(nd), indexing="ij")
    return pq.reshape(-1), pd.reshape(-1)


def f32_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------
# 1. bit-exact on integer-exact operands
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(P):
    queries = [U.exact_rows(n, P, 100 + n) for n in U.Q_ROWS]
    docs = [U.exact_rows(n, P, 200 + n) for n in U.D_ROWS]
    s64 = [[(q.astype(np.float64) @ d.astype(np.float64).T) for d in docs] for q in queries]
    return queries, docs, s64


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("P", U.DIMS)
def test_integer_exact_operands_bit_for_bit(P, reduce):
    queries, docs, s64 = exact_case(P)
    pq, pd = all_pairs(len(queries), len(docs))
    rc, got, intact = U.run_maxsim(lib(), queries, docs, pq, pd, P, reduce)
    assert rc == 0 and intact
    want = np.zeros(len(pq), np.float32)
    for k, (a, b) in enumerate(zip(pq, pd)):
        if docs[b].shape[0]:
            total = np.float32(s64[a][b].max(axis=1).sum())         # exact: an integer times 2^-4 below 2^20
            assert float(total) == s64[a][b].max(axis=1).sum()
            want[k] = total / np.float32(queries[a].shape[0]) if reduce == "mean" else total      # IEEE fp32 division
    bad = np.flatnonzero(f32_bits(got) != f32_bits(want))
    assert bad.size == 0, [(U.Q_ROWS[pq[k]], U.D_ROWS[pd[k]], float(got[k]), float(want[k])) for k in bad[:8]]
    assert np.all(f32_bits(got[np.array([docs[b].shape[0] == 0 for b in pd])]) == 0)           # no rows: +0.0


# ---------------------------------------------------------------------------------------------------------
# 2. decisive tokens
# ---------------------------------------------------------------------------------------------------------
def check_pair(q, d, P, reduce):
    rc, got, intact = U.run_maxsim(lib(), [q], [d], [0], [0], P, reduce)
    assert rc == 0 and intact
    ref, bound = U.ref_maxsim(q, d, reduce), U.kernel_bound(q, d, reduce)
    assert abs(float(got[0]) - ref) <= bound, (float(got[0]), ref, bound)
    return ref


@pytest.mark.parametrize("P", [128, 1024])
@pytest.mark.parametrize("nd,row", [(65, 0), (65, 31), (65, 32), (64, 63), (65, 64), (200, 199), (33, 32), (1, 0)])
def test_the_document_token_that_decides(P, nd, row):
    q, d = U.decisive_doc(P, 33, nd, row, seed=nd * 7 + row)
    ref = check_pair(q, d, P, "mean")
    without = U.ref_maxsim(q, np.delete(d, row, axis=0), "mean")
    assert abs(ref - without) > 10 * U.SCORE_BAR, (ref, without)


@pytest.mark.parametrize("P", [128, 1024])
@pytest.mark.parametrize("nd", [1, 31, 33, 65, 200])
def test_all_negative_products_a_padding_row_must_not_win(P, nd):
    q, d = U.decisive_doc(P, 33, nd, nd - 1, seed=nd, negative=True)
    assert (q.astype(np.float64) @ d.astype(np.float64).T).max() < 0
    ref = check_pair(q, d, P, "mean")
    assert ref < -0.1 and abs(U.ref_maxsim(q, d, "mean", broken="admit_padding_row") - ref) > 10 * U.SCORE_BAR


@pytest.mark.parametrize("P", [128, 1024])
@pytest.mark.parametrize("nq,row", [(70, 31), (70, 32), (70, 69), (33, 32), (32, 31)])
def test_the_query_row_that_decides(P, nq, row):
    q, d = U.decisive_query(P, nq, 65, row, seed=nq + row)
    ref = check_pair(q, d, P, "sum")
    without = U.ref_maxsim(np.delete(q, row, axis=0), d, "sum")
    assert abs(ref - without) > 10 * U.SCORE_BAR, (ref, without)


# ---------------------------------------------------------------------------------------------------------
# 3. random unit rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [128, 256, 1024])
def test_random_unit_rows_within_the_derived_bounds(P):
    raw_q = [U.unit_rows(n, P, 300 + n) for n in U.Q_ROWS]
    raw_d = [U.unit_rows(n, P, 400 + n) for n in (1, 33, 65, 200)]
    queries, docs = [U.f16(a) for a in raw_q], [U.f16(a) for a in raw_d]
    pq, pd = all_pairs(len(queries), len(docs))
    worst = {"sum": 0.0, "mean": 0.0}
    for reduce in ("sum", "mean"):
        rc, got, intact = U.run_maxsim(lib(), queries, docs, pq, pd, P, reduce)
        assert rc == 0 and intact
        for k, (a, b) in enumerate(zip(pq, pd)):
            ref, bound = U.ref_maxsim(queries[a], docs[b], reduce), U.kernel_bound(queries[a], docs[b], reduce)
            worst[reduce] = max(worst[reduce], abs(float(got[k]) - ref) / bound)
            if reduce == "mean":        # against the rows before they were rounded to float16
                total = bound + U.rounding_bound(raw_q[a], raw_d[b])
                assert total < U.SCORE_BAR
                assert abs(float(got[k]) - U.ref_maxsim(raw_q[a], raw_d[b], "mean")) <= total
    print(f"P={P}: worst |kernel - float64| / bound: sum {worst['sum']:.3f}, mean {worst['mean']:.3f}")
    assert worst["sum"] <= 1.0 and worst["mean"] <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------
# 4. a pair's bits do not depend on its company
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowd(P=128):
    """6 queries and 50 documents of mixed sizes (empty ones among them), 300 pairs"""
    rng = np.random.default_rng(9)
    queries = [U.f16(U.unit_rows(n, P, 500 + k)) for k, n in enumerate((1, 5, 32, 33, 70, 32))]
    docs = [U.f16(U.unit_rows(int(n), P, 600 + k)) for k, n in enumerate(rng.choice(U.D_ROWS, size=50))]
    pq, pd = all_pairs(6, 50)
    return queries, docs, pq, pd


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_a_pair_alone_in_a_crowd_and_reversed_through_the_library(reduce):
    P = 128
    queries, docs, pq, pd = crowd(P)
    rc, full, intact = U.run_maxsim(lib(), queries, docs, pq, pd, P, reduce)
    assert rc == 0 and intact and len(full) == 300
    rc, rev, intact = U.run_maxsim(lib(), queries, docs, pq[::-1], pd[::-1], P, reduce)
    assert rc == 0 and intact and np.array_equal(f32_bits(rev[::-1]), f32_bits(full))
    for k in (0, 37, 149, 250, 299):
        rc, one, intact = U.run_maxsim(lib(), [queries[pq[k]]], [docs[pd[k]]], [0], [0], P, reduce)      # alone, and at other offsets of q and d
        assert rc == 0 and intact and f32_bits(one)[0] == f32_bits(full)[k], k
    # the same document under every query, and the same pair many times in one call
    rc, col, _ = U.run_maxsim(lib(), queries, docs, np.arange(6), np.full(6, 17), P, reduce)
    assert rc == 0 and np.array_equal(f32_bits(col), f32_bits(full.reshape(6, 50)[:, 17]))
    rc, rep, _ = U.run_maxsim(lib(), queries, docs, np.full(40, 4), np.full(40, 17), P, reduce)
    assert rc == 0 and np.all(f32_bits(rep) == f32_bits(full.reshape(6, 50)[4, 17]))


def test_a_pair_alone_and_in_a_crowd_through_a_store_that_grew_twice():
    from kirag_amd.retriever.late import MultiVectorStore
    P = 128
    queries, docs, pq, pd = crowd(P)
    rc, full, _ = U.run_maxsim(lib(), queries, docs, pq, pd, P, "mean")
    assert rc == 0
    store = MultiVectorStore(P, device="cuda:0")
    caps = set()
    for k, d in enumerate(docs):                    # one passage per call: 50 adds, capacities 1024 -> 2048 -> 4096
        store.add([str(1000 + k)], [d.astype(np.float32)])
        caps.add(store.vectors.shape[0])
    assert store.ntotal == 50 and store.ntokens == sum(len(d) for d in docs) and len(caps) >= 3, caps
    ids = [str(1000 + k) for k in range(50)]
    got = store.maxsim([q.astype(np.float32) for q in queries], [ids] * 6)
    assert np.array_equal(f32_bits(np.concatenate(got)), f32_bits(full))
    alone = store.maxsim([queries[3]], [["1017"]])[0]
    assert f32_bits(alone)[0] == f32_bits(full.reshape(6, 50))[3, 17]
    rev = store.maxsim([queries[3]], [ids[::-1]])[0]
    assert np.array_equal(f32_bits(rev[::-1]), f32_bits(full.reshape(6, 50)[3]))
    # rerank: score descending, then position; ids come back as strings
    top_ids, top = store.rerank(queries[3], ids, top_k=7)
    order = np.lexsort((np.arange(50), -full.reshape(6, 50)[3].astype(np.float64)))[:7]
    assert top_ids == [ids[i] for i in order] and np.array_equal(f32_bits(top), f32_bits(full.reshape(6, 50)[3][order]))
    assert np.array_equal(store.get("1017"), docs[17].astype(np.float32))
    with pytest.raises(KeyError, match="4242"):
        store.maxsim([queries[0]], [["1000", "4242"]])
    with pytest.raises(ValueError, match="reduce"):
        store.maxsim([queries[0]], [["1000"]], reduce="max")
    sums = store.maxsim([queries[3]], [ids], reduce="sum")[0]
    rc, want, _ = U.run_maxsim(lib(), queries, docs, np.full(50, 3), np.arange(50), P, "sum")
    assert np.array_equal(f32_bits(sums), f32_bits(want))


def test_release_scratch_between_calls_changes_nothing():
    P = 128
    queries, docs, pq, pd = crowd(P)
    rc, before, _ = U.run_maxsim(lib(), queries, docs, pq, pd, P, "mean")
    assert rc == 0
    lib().kl_release_scratch()
    lib().kl_release_scratch()                      # nothing left to free: a no-op
    rc, after, intact = U.run_maxsim(lib(), queries, docs, pq, pd, P, "mean")
    assert rc == 0 and intact and np.array_equal(f32_bits(after), f32_bits(before))
    side = torch.cuda.Stream()                      # another stream than the previous call's: ordered behind it by the library
    with torch.cuda.stream(side):
        rc, other, intact = U.run_maxsim(lib(), queries, docs, pq[::-1], pd[::-1], P, "mean")
    assert rc == 0 and intact and np.array_equal(f32_bits(other[::-1]), f32_bits(before))


# ---------------------------------------------------------------------------------------------------------
# 5. the gather
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [32, 128, 1024])
def test_gather_gives_the_bits_of_torchs_cpu_conversion(P):
    rng = np.random.default_rng(P)
    block = rng.standard_normal((40, P)).astype(np.float32)
    block[3, :8] = [65504.0, -65504.0, 65519.9, 6e-8, -2.9e-8, 3.1e-8, 6.1e-5, -0.0]     # the largest finite values, subnormal results, a tie region, a zero
    block[5] = rng.standard_normal(P).astype(np.float32) * 1e-6                            # a row of subnormal results
    block[7] = 1 + (rng.integers(0, 512, P) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -11)   # odd multiples of half an ulp in [1, 2): every one a tie
    src = np.array([39, 3, 3, 0, 5, 7, 12, 38, 1], np.int64)
    rc, got, intact = U.run_gather(lib(), block, src)
    assert rc == 0 and intact
    want = torch.from_numpy(block[src]).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e6, -65520.0])
def test_gather_refuses_what_is_not_finite_in_float16(bad):
    block = np.random.default_rng(1).standard_normal((9, 64)).astype(np.float32)
    block[4, 33] = bad
    rc, _, intact = U.run_gather(lib(), block, np.array([0, 4, 8], np.int64))
    assert rc == KL_ERANGE and intact and "finite" in lib().kl_last_error().decode()
    rc, _, intact = U.run_gather(lib(), block, np.array([0, 3, 8], np.int64))         # the bad row is not among the gathered ones
    assert rc == 0 and intact


def test_add_block_on_the_device_equals_the_cpu_store():
    from kirag_amd.retriever.late import MultiVectorStore
    B, S, P = 5, 23, 128
    block = torch.from_numpy(np.random.default_rng(2).standard_normal((B, S, P)).astype(np.float32))
    _, mask = M.batch("xlmr", B, S, "holes", seed=3)
    ids = [str(k) for k in range(B)]
    for skip in (True, False):
        cpu, dev = MultiVectorStore(P, device="cpu"), MultiVectorStore(P, device="cuda:0")
        cpu.add_block(ids, block, mask, skip_first=skip)
        dev.add_block(ids, block.cuda(), mask, skip_first=skip)
        assert dev.ntokens == cpu.ntokens and dev.offsets.tolist() == cpu.offsets.tolist()
        assert torch.equal(dev.vectors[:dev.ntokens].cpu().view(torch.int16), cpu.vectors[:cpu.ntokens].view(torch.int16))
    bad = block.clone()
    bad[2, 1, 5] = float("nan")
    dev = MultiVectorStore(P, device="cuda:0")
    with pytest.raises(ValueError, match="finite"):
        dev.add_block(ids, bad.cuda(), np.ones((B, S), np.int64))
    assert (dev.ntotal, dev.ntokens) == (0, 0)


# ---------------------------------------------------------------------------------------------------------
# 6. end to end: index_passages, retrieve
# ---------------------------------------------------------------------------------------------------------
# Twelve short passages (1 .. 8 toy words) and four queries: the synthetic backbones put every score of a query within about 0.1 of the others, so more passages
# would leave most neighbours closer than 2e-3.  With these seeds the reference alone (HF fp32 on the CPU) has 3 .. 4 of its 44 neighbouring pairs per model
# under that gap (at most 9.1 %, against the quarter allowed).
N_PASSAGES, N_QUERIES, SEED_P, SEED_Q = 12, 4, 5, 105
WEIGHTS = (0.4, 0.6)


@functools.lru_cache(maxsize=None)
def m3_model(kind, P):
    from kirag_amd.retriever.m3 import BertM3Encoder, BGEM3Model, XLMRobertaM3Encoder
    hw = M.heads_for(kind, P)
    enc = M.hf_backbone(kind, M.backbone(kind), "cuda", cls=XLMRobertaM3Encoder if kind == "xlmr" else BertM3Encoder)
    enc.set_heads({"weight": torch.from_numpy(hw[M.HEADS[0]]), "bias": torch.from_numpy(hw[M.HEADS[1]])},
                  {"weight": torch.from_numpy(hw[M.HEADS[2]]), "bias": torch.from_numpy(hw[M.HEADS[3]])})
    return BGEM3Model(enc, tokenizer=X.toy_tokenizer()), hw


def reference_scores(kind, hw, tok, queries, passages, device):
    """[n_queries, n_passages] float64: (w_d dense + w_c colbert) / (w_d + w_c) of the HF fp32 model + the heads in float64"""
    hf = M.hf_backbone(kind, M.backbone(kind), device)
    rq, rp = M.ref_encode(hf, hw, tok, queries), M.ref_encode(hf, hw, tok, passages)
    wd, wc = WEIGHTS
    out = np.empty((len(rq), len(rp)))
    for i, q in enumerate(rq):
        for j, p in enumerate(rp):
            s = M.ref_scores(q, p)
            out[i, j] = (wd * s["dense"] + wc * s["colbert"]) / (wd + wc)
    return out


@pytest.mark.parametrize("kind,P", [("xlmr", 128), ("xlmr", 256), ("bert", 128), ("bert", 256)])
def test_index_passages_then_retrieve_follows_the_reference(kind, P):
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.late import MultiVectorStore
    m3, hw = m3_model(kind, P)
    passages, queries = M.texts(N_PASSAGES, seed=SEED_P, lo=1, hi=8), M.texts(N_QUERIES, seed=SEED_Q, lo=4, hi=12)
    ids = [str(500 + 3 * k) for k in range(N_PASSAGES)]
    indexer, store = Indexer(128), MultiVectorStore(P, device="cuda:0")
    m3.index_passages(ids, passages, indexer, store, batch_size=5)
    assert indexer.index.ntotal == store.ntotal == N_PASSAGES
    ref = reference_scores(kind, hw, m3.tokenizer, queries, passages, "cuda")
    got = m3.retrieve(queries, indexer, store, top_k=N_PASSAGES, n_candidates=N_PASSAGES, weights=WEIGHTS)
    skipped = checked = 0
    worst = 0.0
    for i, (got_ids, got_scores) in enumerate(got):
        assert sorted(got_ids) == sorted(ids) and got_scores.dtype == np.float32 and np.all(np.diff(got_scores) <= 0)
        col = np.array([ids.index(x) for x in got_ids])
        worst = max(worst, float(np.abs(got_scores - ref[i, col]).max()))
        rank = np.empty(N_PASSAGES, np.int64); rank[col] = np.arange(N_PASSAGES)
        order = np.argsort(-ref[i], kind="stable")
        for a, b in zip(order[:-1], order[1:]):                # neighbours in the reference's order
            if ref[i, a] - ref[i, b] > 2 * M.SCORE_BAR:
                checked += 1
                assert rank[a] < rank[b], (i, ids[a], ids[b])
            else:
                skipped += 1
    print(f"{kind} P={P}: worst |score - reference| {worst:.2e}; {skipped} of {skipped + checked} neighbouring pairs lie within 2e-3 of each other")
    assert worst <= M.SCORE_BAR
    assert skipped <= (skipped + checked) / 4
    # fewer candidates than passages: the candidates are the dense top-n, and a pair scores as it did in the larger call
    few = m3.retrieve(queries[:1], indexer, store, top_k=3, n_candidates=6, weights=WEIGHTS)[0]
    dense_top = m3.encode(queries[:1])["dense_vecs"]
    cand = indexer.search_knn(dense_top, 6, verbose=False)[0][0]
    assert len(few[0]) == 3 and set(few[0]) <= set(cand)
    full = dict(zip(got[0][0], got[0][1]))
    assert all(f32_bits(np.float32(full[x])) == f32_bits(s) for x, s in zip(*few))
    # the stored rows are the float16 rounding of what encode returns
    vecs = m3.encode(passages, batch_size=5, return_colbert_vecs=True)["colbert_vecs"]
    for k in (0, 4, 5, 11):
        assert np.array_equal(store.get(ids[k]), vecs[k].astype(np.float16).astype(np.float32)), k
