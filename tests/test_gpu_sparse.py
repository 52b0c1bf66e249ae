"""GPU tests of libkirag_sparse.so and of what stands on it (kirag_amd.retriever.sparse_index.SparseIndexer, SpladeModel.index_passages / retrieve,
BGEM3Model.index_passages(sparse_index=) / retrieve_sparse).

The result definition of include/kirag_sparse.h fixes the order of every rounding, so kernel and reference (tests/sparse_util.py, numpy float32) must agree
BIT FOR BIT, rows and score bits, in every case below that calls the library on generated data: no tolerance is involved.  The float64 sum with the a-priori
bound gamma_m sum q d is a second, independent check on the random cases.  R is the library's ``ks_block_rows()``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def lib():
    from kirag_amd import _sparse_lib
    return _sparse_lib.load()


@functools.lru_cache(maxsize=None)
def R():
    return int(lib().ks_block_rows())


def gpu_index(c, n=None):
    """a SparseIndexer on the GPU holding the first ``n`` rows of corpus ``c`` under the ids "0", "1", ..."""
    from kirag_amd.retriever.sparse_index import SparseIndexer
    ix = SparseIndexer(c.V, device="cuda:0")
    n = c.N if n is None else n
    ix.index_data([str(i) for i in range(n)], c.pairs(0, n))
    return ix


def search(ix, queries, k):
    rc, s, r, intact = U.run_search(lib(), ix, queries, k)
    assert rc == 0, lib().ks_last_error().decode()
    assert intact, "guard words around an output were overwritten"
    return s, r


def assert_equal_to_reference(c, ix, queries, k):
    s, r = search(ix, queries, k)
    for i, (t, w) in enumerate(queries):
        ws, wr = U.ref_search(c, t, w, k)
        assert np.array_equal(r[i], wr), (i, k, r[i][:12], wr[:12])
        assert np.array_equal(U.bits(s[i]), U.bits(ws)), (i, k)
    return s, r


# ---------------------------------------------------------------------------------------------------------
# 1. random corpora, bit for bit
# ---------------------------------------------------------------------------------------------------------
def sizes():
    return {"1": 1, "R-1": R() - 1, "R": R(), "R+1": R() + 1, "2R+5": 2 * R() + 5}


@functools.lru_cache(maxsize=None)
def random_case(V, size):
    N = sizes()[size]
    c = U.random_corpus(V, N, seed=V + N % 1000)
    return c, gpu_index(c), [U.random_query(V, m, seed=7 * m + V) for m in U.QUERY_TERMS]         # a 200-term query holds min(200, V) terms


@pytest.mark.parametrize("size", ["1", "R-1", "R", "R+1", "2R+5"])
@pytest.mark.parametrize("V", U.VOCABS)
def test_random_corpus_bit_for_bit(V, size):
    c, ix, queries = random_case(V, size)
    got = {k: assert_equal_to_reference(c, ix, queries, k) for k in U.KS}
    assert np.array_equal(got[100][1][:, :10], got[10][1]) and np.array_equal(U.bits(got[100][0][:, :10]), U.bits(got[10][0]))      # k = 10 is the prefix of k = 100
    # the second, independent check: every returned score lies within gamma_m sum q d of the float64 sum
    s, r = got[1024]
    for i, (t, w) in enumerate(queries):
        s64, bound = U.scores64(c, t, w)
        hit = r[i] >= 0
        assert (np.abs(s[i][hit].astype(np.float64) - s64[r[i][hit]]) <= bound[r[i][hit]]).all()
        assert hit.sum() == min(1024, int((s64 > 0).sum()))
    if c.N > 1:
        assert (got[1024][1] >= 0).sum() > 4                      # the queries do meet rows


def test_a_query_of_more_terms_than_one_chunk_of_segments():
    """the scan fetches the segments of 1024 query terms at a time: 1024 terms are one full chunk, 1025 one term more, 2500 three chunks"""
    c, ix, _ = random_case(30522, "R+1")
    queries = [U.random_query(30522, m, seed=m) for m in (1024, 1025, 2500)]
    assert [len(t) for t, _ in queries] == [1024, 1025, 2500]
    for k in (10, 1024):
        assert_equal_to_reference(c, ix, queries, k)


def test_bge_m3_vocabulary():
    """V = 250002, N = R + 1: a pointer table of a megabyte per block"""
    c = U.random_corpus(250002, R() + 1, seed=9, lo=1, hi=40)
    ix = gpu_index(c)
    queries = [U.random_query(250002, m, seed=m) for m in (33, 200)] + [(np.array([250001], np.int32), np.array([1.0], np.float32))]
    for k in (10, 100):
        _, r = assert_equal_to_reference(c, ix, queries, k)
    assert (r[:2, 0] >= 0).all()


# ---------------------------------------------------------------------------------------------------------
# 2. decisive placements, ties, queries that meet nothing
# ---------------------------------------------------------------------------------------------------------
SPECIAL = 1020                     # the random rows use the terms below; 1020 .. 1030 are placed by hand


@functools.lru_cache(maxsize=None)
def placed_case():
    """V = 1031, N = 2R + 1.  Random rows over the terms < 1020; by hand: term 1020 + i on placement row i alone, with the largest float16 weight;
    term 1026 with weight 1.0 on the 30 rows R - 16 .. R - 2 and R + 1 .. R + 15, which hold nothing else; term 1027 with distinct weights on 9 rows; 1028 .. 1030 nowhere"""
    Rr = R()
    base = U.random_corpus(SPECIAL, 2 * Rr + 1, seed=21)
    rows = [list(base.row(r)) for r in range(base.N)]
    placements = [0, Rr - 1, Rr, 2 * Rr - 1, 2 * Rr]
    for i, p in enumerate(placements):
        rows[p] = [np.append(rows[p][0], SPECIAL + i).astype(np.int32), np.append(rows[p][1], np.float16(60000.0))]
    tied = list(range(Rr - 16, Rr - 1)) + list(range(Rr + 1, Rr + 16))
    for r in tied:
        rows[r] = [np.array([1026], np.int32), np.array([1.0], np.float16)]
    nine = [5, 77, Rr - 100, Rr + 30, Rr + 31, 2 * Rr - 7, 2 * Rr - 6, 1000, 1001]
    for j, r in enumerate(nine):
        rows[r] = [np.append(rows[r][0], 1027).astype(np.int32), np.append(rows[r][1], np.float16(0.5 + 0.125 * j))]
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=off[1:])
    c = U.Corpus(1031, off, np.concatenate([t for t, _ in rows]), np.concatenate([w for _, w in rows]).astype(np.float32))
    full = U.Corpus(1031, off[:2 * Rr + 1], c.terms[:off[2 * Rr]], c.w32[:off[2 * Rr]])       # without the one-row tail block
    ix = gpu_index(c, 2 * Rr)
    return c, full, ix, placements, tied, nine


def test_the_best_row_at_the_edges_of_the_first_and_the_last_block():
    c, full, ix, placements, _, _ = placed_case()
    Rr = R()
    assert ix.ntotal == 2 * Rr                                    # two full blocks: rows 0, R - 1 (first block), R, 2R - 1 (last block)
    qt, qw = U.random_query(SPECIAL, 33, seed=3)
    queries = [(np.append(qt, SPECIAL + i).astype(np.int32), np.append(qw, np.float32(2.0))) for i in range(4)]
    for k in (1, 10):
        _, r = assert_equal_to_reference(full, ix, queries, k)
        assert r[:, 0].tolist() == placements[:4]
    # one more row: the first row of a one-row tail block
    ix.index_data([str(2 * Rr)], [c.row(2 * Rr)])
    queries.append((np.append(qt, SPECIAL + 4).astype(np.int32), np.append(qw, np.float32(2.0))))
    for k in (1, 10):
        _, r = assert_equal_to_reference(c, ix, queries, k)
        assert r[:, 0].tolist() == placements
    assert_equal_to_reference(c, ix, [(np.array([SPECIAL + 4], np.int32), np.array([0.5], np.float32))], 3)       # the tail row alone is a result


def test_bit_equal_scores_across_two_blocks_the_lower_rows_win():
    c, _, _, _, tied, _ = placed_case()
    ix = tie_index()
    k = 10
    assert len(tied) == 3 * k and tied[0] < R() <= tied[-1]
    # the tied rows alone: the first k of them; with k = 100 all 30 and then row -1
    s, r = assert_equal_to_reference(c, ix, [(np.array([1026], np.int32), np.array([1.5], np.float32))], k)
    assert r[0].tolist() == tied[:k] and (s[0] == 1.5).all()
    s, r = assert_equal_to_reference(c, ix, [(np.array([1026], np.int32), np.array([1.5], np.float32))], 100)
    assert r[0][:30].tolist() == tied and (r[0][30:] == -1).all() and (U.bits(s[0][30:]) == 0).all()
    # the cut goes through the tie: term 1026's query weight IS the 8th best score of the other terms, so 7 rows lie above the 31 rows that share that score
    qt, qw = U.random_query(SPECIAL, 33, seed=5)
    v = np.sort(U.ref_scores(c, qt, qw))[::-1][7]
    q = (np.append(qt, 1026).astype(np.int32), np.append(qw, v))
    full = U.ref_scores(c, *q)
    assert (U.bits(full) == U.bits(np.array([v]))[0]).sum() == 31 and (full > v).sum() == 7
    s, r = assert_equal_to_reference(c, ix, [q], k)
    assert (U.bits(s[0][7:]) == U.bits(np.array([v]))[0]).all() and (np.diff(r[0][7:]) > 0).all()


@functools.lru_cache(maxsize=None)
def tie_index():
    c = placed_case()[0]
    return gpu_index(c)


def test_exactly_k_minus_1_positive_rows_leave_the_last_place_empty():
    c, _, _, _, _, nine = placed_case()
    ix = tie_index()
    s, r = assert_equal_to_reference(c, ix, [(np.array([1027], np.int32), np.array([0.75], np.float32))], 10)
    assert sorted(r[0][:9].tolist()) == sorted(nine) and r[0][9] == -1 and U.bits(s[0])[9] == 0
    assert r[0][0] == nine[-1]                                    # the largest weight


def test_queries_that_meet_nothing_among_ordinary_ones():
    c = placed_case()[0]
    ix = tie_index()
    a, b = U.random_query(SPECIAL, 33, seed=8), U.random_query(SPECIAL, 2, seed=9)
    queries = [a,
               (np.append(a[0], 1029).astype(np.int32), np.append(a[1], np.float32(3.0))),        # one term no row holds
               (np.array([1028, 1029, 1030], np.int32), np.ones(3, np.float32)),                  # nothing in common with the corpus
               (np.empty(0, np.int32), np.empty(0, np.float32)),                                  # no terms
               b]
    for k in (1, 100):
        s, r = assert_equal_to_reference(c, ix, queries, k)
        assert np.array_equal(r[0], r[1]) and np.array_equal(U.bits(s[0]), U.bits(s[1]))
        assert (r[2:4] == -1).all() and (U.bits(s[2:4]) == 0).all()
    from kirag_amd.retriever.sparse_index import SparseIndexer
    out = ix.search_knn([queries[0], queries[3], {"1027": 0.75}], 10)
    assert out[1] == ([], []) and len(out[0][0]) == 10 and len(out[2][0]) == 9 and all(isinstance(x, str) for x in out[0][0])
    assert out[0][1] == s[0][:10].tolist()                       # s: the k = 100 call above, whose first ten are the k = 10 result
    empty = SparseIndexer(1031, device="cuda:0")                 # an index without rows: every place is empty
    assert empty.search_knn([queries[0]], 5) == [([], [])]


# ---------------------------------------------------------------------------------------------------------
# 3. invariance, bit for bit
# ---------------------------------------------------------------------------------------------------------
def test_a_query_alone_among_300_and_reversed():
    c, ix, _ = random_case(1031, "R+1")
    queries = [U.random_query(1031, 33 if i % 3 else 2, seed=1000 + i) for i in range(300)]
    s, r = search(ix, queries, 10)
    s2, r2 = search(ix, queries[::-1], 10)
    assert np.array_equal(r2[::-1], r) and np.array_equal(U.bits(s2[::-1]), U.bits(s))
    for i in (0, 17, 299):
        s1, r1 = search(ix, [queries[i]], 10)
        assert np.array_equal(r1[0], r[i]) and np.array_equal(U.bits(s1[0]), U.bits(s[i]))
        ws, wr = U.ref_search(c, *queries[i], 10)
        assert np.array_equal(r[i], wr) and np.array_equal(U.bits(s[i]), U.bits(ws))


def test_a_rows_score_does_not_move_when_its_block_closes():
    """ten rows in the open tail block, then 2R more: the ten now lie in a closed block and two blocks follow"""
    Rr = R()
    c = U.random_corpus(SPECIAL, 2 * Rr + 10, seed=31)
    rows = c.pairs()
    for r in range(10):            # term 1025 lifts the first ten rows to the top, so that they are reported both times
        rows[r] = (np.append(rows[r][0], 1025).astype(np.int32), np.append(rows[r][1], np.float16(200.0 + r)))
    from kirag_amd.retriever.sparse_index import SparseIndexer
    ix = SparseIndexer(1031, device="cuda:0")
    ix.index_data([str(i) for i in range(10)], rows[:10])
    qt, qw = U.random_query(SPECIAL, 33, seed=6)
    q = [(np.append(qt, 1025).astype(np.int32), np.append(qw, np.float32(1.25)))]
    s_a, r_a = search(ix, q, 10)
    assert sorted(r_a[0].tolist()) == list(range(10)) and ix._closed == 0
    ix.index_data([str(i) for i in range(10, len(rows))], rows[10:])
    assert ix._closed == 2 and ix.ntotal == 2 * Rr + 10
    s_b, r_b = search(ix, q, 10)
    assert np.array_equal(r_a, r_b) and np.array_equal(U.bits(s_a), U.bits(s_b))
    s_c, r_c = search(ix, q, 1024)                               # and k takes no part in a score
    assert np.array_equal(r_c[0][:10], r_a[0]) and np.array_equal(U.bits(s_c[0][:10]), U.bits(s_a[0]))


def test_release_scratch_between_calls_changes_nothing():
    _, ix, queries = random_case(1031, "R+1")
    s, r = search(ix, queries, 100)
    lib().ks_release_scratch()
    s2, r2 = search(ix, queries, 100)
    assert np.array_equal(r, r2) and np.array_equal(U.bits(s), U.bits(s2))


def test_sliced_queries_equal_the_same_queries_one_by_one():
    """two blocks and k = 10 make 20 candidates a query; a bound of 50 lets two queries into a slice: seven queries are four slices"""
    from kirag_amd import _sparse_lib
    c, ix, _ = random_case(1031, "R+1")
    queries = [U.random_query(1031, 33, seed=2000 + i) for i in range(7)]
    _sparse_lib.set_candidate_bound(50)
    try:
        s, r = search(ix, queries, 10)
        rc = U.run_search(lib(), ix, queries, 100)[0]            # 200 candidates a query do not fit 50: refused, nothing launched
        assert rc == -22 and "workspace bound" in lib().ks_last_error().decode()
    finally:
        _sparse_lib.set_candidate_bound(None)
    for i, q in enumerate(queries):
        s1, r1 = search(ix, [q], 10)
        assert np.array_equal(r1[0], r[i]) and np.array_equal(U.bits(s1[0]), U.bits(s[i]))
        ws, wr = U.ref_search(c, *q, 10)
        assert np.array_equal(r[i], wr) and np.array_equal(U.bits(s[i]), U.bits(ws))


# ---------------------------------------------------------------------------------------------------------
# 4. ks_count_positive / ks_compact_rows
# ---------------------------------------------------------------------------------------------------------
def splade_like_block(V, B=6, seed=0):
    rng = np.random.default_rng(seed)
    block = np.where(rng.random((B, V)) < 0.2, rng.uniform(1e-3, 4.0, (B, V)), 0.0).astype(np.float32)
    block[1] = 0.0                                               # a row with no entry
    block[2] = rng.uniform(0.5, 1.0, V)                          # a row with every entry
    block[3, :8] = [1e-9, 2.9e-8, 3.1e-8, -0.5, -0.0, 6e-8, 65504.0, 65519.0]     # rounds to zero, the tie below the smallest subnormal, just above it, ...
    return block


@pytest.mark.parametrize("V", U.VOCABS)
def test_compact_rows_against_the_torch_rule_bit_for_bit(V):
    block = splade_like_block(V, seed=V)
    for skip in ((), (0, 5, V - 1)):
        counts, terms, wbits = U.torch_compact(block, skip)
        rc1, got_counts, rc2, got_terms, got_w, intact = U.run_compact(lib(), block, skip)
        assert rc1 == 0 and rc2 == 0 and intact, lib().ks_last_error().decode()
        assert np.array_equal(got_counts, counts) and counts[1] == 0 and counts[2] == V - len(skip)
        assert np.array_equal(got_terms, terms) and np.array_equal(got_w, wbits)
    row3 = got_terms[counts[:3].sum():counts[:4].sum()]
    assert 0 not in row3 and 1 not in row3 and 3 not in row3 and 4 not in row3 and 2 in row3 and 6 in row3      # what rounds to zero is dropped


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e6, 65520.0])
def test_compact_rows_refuses_what_is_not_finite_in_float16(bad):
    block = splade_like_block(1031, seed=3)
    counts = U.torch_compact(block)[0]
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    block[4, 1000] = bad
    assert U.torch_compact(block) is None
    rc1, _, rc2, _, _, intact = U.run_compact(lib(), block, row_off=off)
    assert rc1 == -34 and rc2 == -34 and intact
    assert "finite" in lib().ks_last_error().decode()


@pytest.mark.parametrize("delta", [-1, 1])
def test_a_row_off_that_disagrees_is_refused_and_nothing_leaves_a_rows_slot(delta):
    block = splade_like_block(1031, seed=4)
    counts, terms, wbits = U.torch_compact(block)
    wrong = counts.copy()
    wrong[4] += delta                                            # one slot too few / too many for row 4
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(wrong, out=off[1:])
    rc1, _, rc2, got_terms, _, intact = U.run_compact(lib(), block, row_off=off)
    assert rc1 == 0 and rc2 == -22 and intact
    assert "row_off disagrees" in lib().ks_last_error().decode()
    assert np.array_equal(got_terms[:off[4]], terms[:off[4]])    # the rows before it are whole, in their own slots
    assert np.array_equal(got_terms[off[5]:], terms[counts[:5].sum():])      # and the rows behind it in theirs


def test_index_block_on_the_device_equals_the_cpu_index():
    from kirag_amd.retriever.sparse_index import SparseIndexer
    V = 30522
    block = splade_like_block(V, B=5, seed=6)
    ids = [str(10 + i) for i in range(5)]
    cpu, gpu = SparseIndexer(V, device="cpu"), SparseIndexer(V, device="cuda:0")
    for s in (slice(0, 2), slice(2, 5)):
        cpu.index_block(ids[s], torch.from_numpy(block[s]), skip_terms=(0,))
        gpu.index_block(ids[s], torch.from_numpy(block[s]).cuda(), skip_terms=(0,))
    assert np.array_equal(cpu.row_off, gpu.row_off) and np.array_equal(cpu.terms, gpu.terms) and np.array_equal(U.bits(cpu.weights), U.bits(gpu.weights))
    assert gpu.ntotal == 5 and gpu.nnz > V and 0 not in gpu.terms
    bad = block.copy(); bad[1, 7] = np.inf
    with pytest.raises(ValueError, match="finite"):
        gpu.index_block(["1", "2", "3", "4", "5"], torch.from_numpy(bad).cuda())
    with pytest.raises(ValueError, match="is on"):
        gpu.index_block(["1", "2", "3", "4", "5"], torch.from_numpy(block))
    assert gpu.ntotal == 5


# ---------------------------------------------------------------------------------------------------------
# 5. end to end: index_passages, then retrieve / retrieve_sparse
# ---------------------------------------------------------------------------------------------------------
N_PASSAGES, N_QUERIES = 64, 8
# (b) below orders by the HF reference wherever its neighbouring scores differ by more than a margin, the margin being twice the worst |score - HF score|
# measured on these very cases on one MI355X (profiles/sparse/measurements.txt, section 4):
#     SPLADE (synthetic tied BERT, 64 passages, 8 queries)   worst measured 1.342e-02, on scores up to 63.3
#     M3 (synthetic xlmr / bert, 64 passages, 8 queries)     worst measured 8.142e-06 (xlmr), 3.343e-06 (bert), on scores up to 0.025
# Checked on the CPU before any GPU run: of HF's own neighbouring pairs 42 of 504 (SPLADE), 2 of 95 (xlmr) and 8 of 91 (bert) lie within these margins.
SPLADE_WORST, M3_WORST = 1.35e-2, 8.2e-6
SPLADE_MARGIN, M3_MARGIN = 2 * SPLADE_WORST, 2 * M3_WORST


def check_against_corpus(got, ids, c, queries):
    """(a): what came back is the reference's result over the library's own encode outputs: ids in its order, scores within the float64 bound (here even its
    bits, since the stored weights ARE those outputs rounded to float16)"""
    for (got_ids, got_scores), (t, w) in zip(got, queries):
        ws, wr = U.ref_search(c, t, w, len(ids))
        n = int((wr >= 0).sum())
        assert got_ids == [ids[r] for r in wr[:n]]
        s64, bound = U.scores64(c, t, w)
        assert (np.abs(np.asarray(got_scores, np.float64) - s64[wr[:n]]) <= bound[wr[:n]]).all()
        assert np.array_equal(U.bits(np.asarray(got_scores, np.float32)), U.bits(ws[:n]))


def check_order_against_hf(got, ids, hf, margin, label):
    """(b): hf [nq, N] float64 scores; returns the worst |score - HF score| over what came back"""
    worst, skipped, checked = 0.0, 0, 0
    for i, (got_ids, got_scores) in enumerate(got):
        col = np.array([ids.index(x) for x in got_ids], np.int64)
        worst = max(worst, float(np.abs(np.asarray(got_scores, np.float64) - hf[i, col]).max()))
        rank = np.full(len(ids), len(ids), np.int64); rank[col] = np.arange(len(col))
        order = np.argsort(-hf[i], kind="stable")
        order = order[hf[i, order] > margin]                    # a passage HF scores within the margin of 0 may be no result at all
        for a, b in zip(order[:-1], order[1:]):
            if hf[i, a] - hf[i, b] > margin:
                checked += 1
                assert rank[a] < rank[b], (label, i, ids[a], ids[b])
            else:
                skipped += 1
    print(f"{label}: worst |score - HF score| {worst:.3e}; margin {margin:.3e}; {skipped} of {skipped + checked} neighbouring pairs lie within the margin")
    assert worst <= margin
    assert checked > 0 and skipped <= (skipped + checked) / 4
    return worst


@functools.lru_cache(maxsize=None)
def splade_surface():
    import reranker_util as RU
    import splade_util as S
    from kirag_amd.retriever.splade import BertSpladeEncoder, SpladeModel
    tok = RU.bert_pair_tokenizer()
    V = tok.vocab_size
    w = S.tied_weights(V)
    ref = S.hf_mlm("h64", V, w, "cuda", tie=True)
    twin = S.hf_mlm("h64", V, w, "cuda", cls=BertSpladeEncoder, tie=True)
    return tok, ref, SpladeModel(twin, tokenizer=tok)


def dense_rows_as_queries(vecs, pad):
    out = []
    for v in vecs:
        idx = np.flatnonzero(v > 0)
        idx = idx[idx != pad]
        out.append((idx.astype(np.int32), v[idx].astype(np.float32)))
    return out


def test_splade_index_passages_then_retrieve():
    import reranker_util as RU
    import splade_util as S
    from kirag_amd.retriever.sparse_index import SparseIndexer
    tok, ref, model = splade_surface()
    V, pad = tok.vocab_size, tok.pad_token_id
    passages, queries = RU.passages(N_PASSAGES, seed=12), RU.passages(N_QUERIES, seed=11, lo=8, hi=12)
    ids = [str(700 + 3 * i) for i in range(N_PASSAGES)]
    ix = SparseIndexer(V, device="cuda:0")
    model.index_passages(ids, passages, ix, batch_size=24)
    assert ix.ntotal == N_PASSAGES
    got = model.retrieve(queries, ix, top_k=N_PASSAGES)
    assert len(got) == N_QUERIES and all(len(g[0]) == len(g[1]) > 0 for g in got)
    # (a) the library's own encode outputs: passages rounded to float16, queries in float32
    p = model.encode_dense(passages, batch_size=24).float().cpu().numpy()
    p[:, pad] = 0
    rows = dense_rows_as_queries(np.where(p.astype(np.float16) > 0, p, 0), pad)
    off = np.zeros(N_PASSAGES + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=off[1:])
    c = U.Corpus(V, off, np.concatenate([t for t, _ in rows]), np.concatenate([w for _, w in rows]))
    assert np.array_equal(c.terms, ix.terms) and np.array_equal(U.bits(c.w16), U.bits(ix.weights))      # what is stored is encode's output in float16
    q = dense_rows_as_queries(model.encode_dense(queries).float().cpu().numpy(), pad)
    check_against_corpus(got, ids, c, q)
    # (b) HF fp32 + the formula
    enc = tok(queries + passages, padding=True, truncation=True, max_length=512, return_tensors="np")
    hf = S.reference(ref, enc["input_ids"].astype(np.int64), enc["attention_mask"].astype(np.int64))
    hf[:, pad] = 0
    check_order_against_hf(got, ids, hf[:N_QUERIES] @ hf[N_QUERIES:].T, SPLADE_MARGIN, "SPLADE")
    top = model.retrieve(queries[0], ix, top_k=5)                # one query as a string, a smaller k: the prefix
    assert top[0][0] == got[0][0][:5] and top[0][1] == got[0][1][:5]


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_m3_index_passages_then_retrieve_sparse(kind):
    import m3_util as M
    import xlmr_util as X
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.late import MultiVectorStore
    from kirag_amd.retriever.m3 import BertM3Encoder, BGEM3Model, XLMRobertaM3Encoder
    from kirag_amd.retriever.sparse_index import SparseIndexer
    P = 128
    hw = M.heads_for(kind, P)
    enc = M.hf_backbone(kind, M.backbone(kind), "cuda", cls=XLMRobertaM3Encoder if kind == "xlmr" else BertM3Encoder)
    enc.set_heads({"weight": torch.from_numpy(hw[M.HEADS[0]]), "bias": torch.from_numpy(hw[M.HEADS[1]])},
                  {"weight": torch.from_numpy(hw[M.HEADS[2]]), "bias": torch.from_numpy(hw[M.HEADS[3]])})
    tok = X.toy_tokenizer()
    m3 = BGEM3Model(enc, tokenizer=tok)
    V = len(tok)
    passages, queries = M.texts(N_PASSAGES, seed=5, lo=3, hi=24), M.texts(N_QUERIES, seed=105, lo=6, hi=16)
    ids = [str(500 + 3 * k) for k in range(N_PASSAGES)]
    indexer, store, sp = Indexer(128), MultiVectorStore(P, device="cuda:0"), SparseIndexer(V, device="cuda:0")
    m3.index_passages(ids, passages, indexer, store, batch_size=24, sparse_index=sp)
    assert indexer.index.ntotal == store.ntotal == sp.ntotal == N_PASSAGES
    got = m3.retrieve_sparse(queries, sp, top_k=N_PASSAGES)
    # (a) the library's own lexical weights
    lex_p = m3.encode(passages, batch_size=24, return_dense=False, return_sparse=True)["lexical_weights"]
    lex_q = m3.encode(queries, return_dense=False, return_sparse=True)["lexical_weights"]
    as_pair = lambda d: (np.array(sorted(int(k) for k in d), np.int32), np.array([d[str(k)] for k in sorted(int(k) for k in d)], np.float32))
    rows = [as_pair({k: w for k, w in d.items() if np.float16(w) > 0}) for d in lex_p]
    off = np.zeros(N_PASSAGES + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=off[1:])
    c = U.Corpus(V, off, np.concatenate([t for t, _ in rows]), np.concatenate([w for _, w in rows]))
    assert np.array_equal(c.terms, sp.terms) and np.array_equal(U.bits(c.w16), U.bits(sp.weights))
    check_against_corpus(got, ids, c, [as_pair(d) for d in lex_q])
    # (b) HF fp32 + the heads in float64
    hf_model = M.hf_backbone(kind, M.backbone(kind), "cuda")
    rq, rp = M.ref_encode(hf_model, hw, tok, queries), M.ref_encode(hf_model, hw, tok, passages)
    hf = np.array([[M.ref_scores(a, b)["sparse"] for b in rp] for a in rq])
    check_order_against_hf(got, ids, hf, M3_MARGIN, "M3 " + kind)

    # a batch one container refuses: the three stay in step
    class Refusing:
        def __init__(self, inner, refuse):
            self.inner, self.refuse, self.index = inner, refuse, inner.index
        def index_data(self, batch_ids, emb):
            if self.refuse in batch_ids:
                raise RuntimeError("the index refuses this batch")
            self.inner.index_data(batch_ids, emb)
    more = [str(9000 + k) for k in range(6)]
    with pytest.raises(RuntimeError, match="refuses this batch"):
        m3.index_passages(more, passages[:6], Refusing(indexer, more[4]), store, batch_size=3, sparse_index=sp)
    assert indexer.index.ntotal == store.ntotal == sp.ntotal == N_PASSAGES + 3
    assert sp.ids.tolist() == store.ids.tolist()
    again = m3.retrieve_sparse(queries[:2], sp, top_k=5)          # the index is searched again after the add and the take-back
    assert all(len(g[0]) == 5 for g in again)
