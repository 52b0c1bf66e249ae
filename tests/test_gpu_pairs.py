"""GPU tests of libkirag_pairs.so and of what stands on it (SparseIndexer.score_pairs / rerank, BGEM3Model.retrieve_hybrid / retrieve_rrf, fusion.fuse_hits
over real hit lists).

The result definition of include/kirag_pairs.h fixes the order of every rounding, so kernel and reference (tests/pairs_util.py: sparse_util.ref_scores read
at the pairs' rows, numpy float32) must agree BIT FOR BIT in every case below that calls the library on generated data: no tolerance is involved.  The float64
sum with the a-priori bound gamma_m sum q d is a second, independent check on the random cases.  R is the sparse library's ``ks_block_rows()``."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_util as PU  # noqa: E402
import sparse_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def lib():
    from kirag_amd import _pairs_lib
    return _pairs_lib.load()


@functools.lru_cache(maxsize=None)
def sparse_lib():
    from kirag_amd import _sparse_lib
    return _sparse_lib.load()


def dot(dc, queries, pq, pr):
    rc, s, intact = PU.run_pairs(lib(), dc, queries, pq, pr)
    assert rc == 0, lib().kp_last_error().decode()
    assert intact, "guard words around out were overwritten"
    return s


# ---------------------------------------------------------------------------------------------------------
# 1. random corpora, every (query, row) pair, bit for bit
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(V):
    c = U.random_corpus(V, 300, seed=V + 300)
    return c, PU.DeviceCorpus(c), [U.random_query(V, m, seed=7 * m + V) for m in U.QUERY_TERMS]


@pytest.mark.parametrize("V", U.VOCABS)
def test_random_corpus_every_pair_bit_for_bit(V):
    c, dc, queries = random_case(V)
    pq, pr = PU.all_pairs(len(queries), c.N)
    got = dot(dc, queries, pq, pr)
    want = PU.ref_pairs(c, queries, pq, pr)
    assert np.array_equal(U.bits(got), U.bits(want))
    # pairs that share no term: exactly +0.0, sign bit clear
    shares = np.concatenate([U.scores64(c, t, w)[0] > 0 for t, w in queries])
    assert 0 < (~shares).sum() < len(shares)
    assert (U.bits(got)[~shares] == PU.POS_ZERO).all() and (got[shares] > 0).all()
    # the second, independent check: within gamma_m sum q d of the float64 sum
    for i, (t, w) in enumerate(queries):
        s64, bound = U.scores64(c, t, w)
        assert (np.abs(got[i * c.N:(i + 1) * c.N].astype(np.float64) - s64) <= bound).all()


def test_the_random_cases_notice_float32_weights():
    """teeth: a kernel that read unrounded weights would not pass the random cases"""
    changed = 0
    for V in U.VOCABS:
        c, _, queries = random_case(V)
        pq, pr = PU.all_pairs(len(queries), c.N)
        changed += int((U.bits(PU.ref_pairs(c, queries, pq, pr)) != U.bits(PU.ref_pairs(c, queries, pq, pr, "float32_weights"))).sum())
    assert changed > 100


# ---------------------------------------------------------------------------------------------------------
# 2. chunk edges: the wave walks a row in chunks of 64 entries
# ---------------------------------------------------------------------------------------------------------
EDGE_V = 2048
EDGE_LENGTHS = (1, 63, 64, 65, 128, 129, 700)


def edge_term(pos):
    """the term at position ``pos`` of every edge row: rows hold even terms from 10 up, so no odd term is in any row"""
    return 10 + 2 * pos


@functools.lru_cache(maxsize=None)
def edge_case():
    rng = np.random.default_rng(77)
    rows = [(np.array([edge_term(j) for j in range(L)], np.int32), rng.uniform(0.05, 3.0, L).astype(np.float32)) for L in EDGE_LENGTHS]
    c = PU.corpus_of(EDGE_V, rows)
    queries, placed = [], []              # placed: (query, row, position of the single shared term, where it sits in the query)
    for r, L in enumerate(EDGE_LENGTHS):
        for pos in sorted({0, L - 1, 63, 64, 127, 128, (L - 1) // 64 * 64} & set(range(L))):
            t = edge_term(pos)
            for where, terms in (("alone", [t]), ("first", [t] + [t + 1 + 2 * j for j in range(5)]), ("last", [1, 3, 5, 7, 9, t])):
                placed.append((len(queries), r, pos, where))
                queries.append((np.array(terms, np.int32), rng.uniform(0.1, 2.0, len(terms)).astype(np.float32)))
    full = len(queries)                   # every entry of the 65-term row is shared: the order of the sum decides the bits
    queries.append((rows[EDGE_LENGTHS.index(65)][0].copy(), rng.uniform(0.1, 2.0, 65).astype(np.float32)))
    return c, queries, placed, full


def test_chunk_edges_bit_for_bit():
    c, queries, placed, full = edge_case()
    dc = PU.DeviceCorpus(c)
    pq, pr = PU.all_pairs(len(queries), c.N)
    got = dot(dc, queries, pq, pr).reshape(len(queries), c.N)
    want = PU.ref_pairs(c, queries, pq, pr).reshape(len(queries), c.N)
    assert np.array_equal(U.bits(got), U.bits(want))
    # the placed pairs share exactly their one term, at the place they were built for
    places = set()
    for q, r, pos, where in placed:
        t, w = queries[q]
        rt, rw = c.row(r)
        shared = np.intersect1d(t, rt)
        assert shared.tolist() == [edge_term(pos)] and rt[pos] == edge_term(pos)
        assert got[q, r] == np.float32(w[t == edge_term(pos)][0] * np.float32(rw[pos])) > 0
        places.add((EDGE_LENGTHS[r], pos))
    for L in EDGE_LENGTHS:
        assert (L, 0) in places and (L, L - 1) in places                     # the row's first and last entry
    assert {(65, 63), (65, 64), (129, 127), (129, 128), (700, 63), (700, 64), (700, 128)} <= places      # lane 63 of a chunk, lane 0 of the next
    assert {(65, 64), (129, 128), (700, 640), (700, 699)} <= places          # only in the ragged last chunk
    assert got[full, EDGE_LENGTHS.index(65)] > 0


def test_the_all_shared_row_decides_order_and_fusion():
    """teeth, on the CPU: on the pair where all 65 entries are shared, summing in descending order or fusing multiply and add changes the reference's bits,
    so the bit-for-bit test above does not hold for a kernel that does either"""
    c, queries, _, full = edge_case()
    r = EDGE_LENGTHS.index(65)
    whole = PU.ref_pairs(c, queries, [full], [r])
    for broken in ("descending_terms", "fused_multiply_add"):
        assert U.bits(PU.ref_pairs(c, queries, [full], [r], broken))[0] != U.bits(whole)[0], broken


# ---------------------------------------------------------------------------------------------------------
# 3. agreement with the search, and the mirror across a block boundary
# ---------------------------------------------------------------------------------------------------------
MARK = 1025                        # the random rows use the terms below 1020; this one is placed by hand


def test_the_rows_a_search_returns_get_the_same_bits_from_pairs_as_the_index_grows():
    """ONE index grown to R - 1, R + 1 and 2R + 5 rows.  At each size: for each query the rows ``ks_search`` returns at k = 1024 get the same score bits from
    ``kp_sparse_dot`` over the index's own mirror — among them the rows on either side of a block boundary and the one-row tail block (row R at size R + 1) —
    and ``score_pairs`` equals the reference over the index's current contents."""
    from kirag_amd.retriever.sparse_index import SparseIndexer
    R = int(sparse_lib().ks_block_rows())
    N = 2 * R + 5
    base = U.random_corpus(1020, N, seed=31, lo=1, hi=12)
    marked = [R - 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, N - 1]
    rows = base.pairs()
    for r in marked:
        rows[r] = (np.append(rows[r][0], MARK).astype(np.int32), np.append(rows[r][1], np.float16(3.0)))
    ids = [str(10 * i + 3) for i in range(N)]
    queries = [(np.array([MARK], np.int32), np.array([1.5], np.float32)), U.random_query(1020, 200, seed=5)]
    t, w = U.random_query(1020, 33, seed=6)
    queries.append((np.append(t, MARK).astype(np.int32), np.append(w, np.float32(2.0))))
    ix = SparseIndexer(1031, device="cuda:0")
    have = 0
    for size in (R - 1, R + 1, N):
        ix.index_data(ids[have:size], rows[have:size])
        have = size
        rc, s, r, intact = U.run_search(sparse_lib(), ix, queries, 1024)
        assert rc == 0 and intact
        dc = PU.IndexCorpus(ix)
        assert dc.c.N == size and ix._synced == ix.nnz
        pq = np.concatenate([np.full(int((r[i] >= 0).sum()), i, np.int64) for i in range(len(queries))])
        pr = np.concatenate([r[i][r[i] >= 0] for i in range(len(queries))])
        got = dot(dc, queries, pq, pr)
        assert np.array_equal(U.bits(got), U.bits(np.concatenate([s[i][r[i] >= 0] for i in range(len(queries))])))
        here = [m for m in marked if m < size]
        assert set(here) <= set(r[0].tolist()) and set(here) <= set(r[2].tolist())          # the boundary rows were among them
        # the public call, on ids: the marked rows and a sample, against the reference over the index's contents
        sample = sorted(set(here) | set(np.random.default_rng(size).integers(0, size, 200).tolist()))
        scores = ix.score_pairs(queries, [[ids[x] for x in sample]] * len(queries))
        want = PU.ref_pairs(dc.c, queries, np.repeat(np.arange(len(queries)), len(sample)), np.tile(sample, len(queries)))
        assert np.array_equal(U.bits(np.concatenate(scores)), U.bits(want))


# ---------------------------------------------------------------------------------------------------------
# 4. a pair's result depends on its row and its query alone
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def independence_case():
    c = U.random_corpus(1031, 300, seed=8)
    a, b = c.row_off[119], c.row_off[120]                              # row 119 loses its terms
    off = c.row_off.copy(); off[120:] -= b - a
    c = U.Corpus(1031, off, np.delete(c.terms, slice(a, b)), np.delete(c.w32, slice(a, b)))
    queries = [U.random_query(1031, m, seed=3 * m) for m in (2, 33, 200)] + [(np.empty(0, np.int32), np.empty(0, np.float32))]
    rng = np.random.default_rng(9)
    pq, pr = rng.integers(0, 4, 60), rng.integers(0, 300, 60)
    pq[:4], pr[:4] = [0, 1, 2, 3], [119, 119, 119, 7]                  # the empty row under three queries; the query without terms
    return c, PU.DeviceCorpus(c), queries, pq.astype(np.int64), pr.astype(np.int64)


def test_a_pairs_result_does_not_depend_on_the_rest_of_the_call():
    from kirag_amd import _pairs_lib
    c, dc, queries, pq, pr = independence_case()
    alone = dot(dc, queries, pq, pr)
    want = PU.ref_pairs(c, queries, pq, pr)
    assert np.array_equal(U.bits(alone), U.bits(want))
    assert (U.bits(alone)[:4] == PU.POS_ZERO).all()                     # an empty row, a query without terms: +0.0
    assert (alone > 0).sum() >= 10 and (alone[4:] == 0).sum() >= 10      # pairs that meet and pairs that do not, side by side
    same = lambda s: np.array_equal(U.bits(s), U.bits(alone))
    for i in range(5):                                                  # one pair to a call
        assert U.bits(dot(dc, queries, pq[i:i + 1], pr[i:i + 1]))[0] == U.bits(alone)[i]
    rng = np.random.default_rng(10)                                     # among 100 000 pairs, at scattered places
    big_q, big_r = rng.integers(0, 4, 100000).astype(np.int64), rng.integers(0, 300, 100000).astype(np.int64)
    at = np.sort(rng.choice(100000, len(pq), replace=False))
    big_q[at], big_r[at] = pq, pr
    among = dot(dc, queries, big_q, big_r)
    assert same(among[at])
    assert np.array_equal(U.bits(among), U.bits(PU.ref_pairs(c, queries, big_q, big_r)))
    assert same(dot(dc, queries, pq[::-1], pr[::-1])[::-1])             # reversed
    dup = dot(dc, queries, np.repeat(pq, 2), np.repeat(pr, 2))          # each pair twice
    assert same(dup[0::2]) and same(dup[1::2])
    _pairs_lib.set_staged_bound(7)                                      # slices of 7 records: 60 pairs are 9 launches
    try:
        assert same(dot(dc, queries, pq, pr))
        assert np.array_equal(U.bits(dot(dc, queries, big_q[:1000], big_r[:1000])), U.bits(among[:1000]))
    finally:
        _pairs_lib.set_staged_bound(None)
    assert same(dot(dc, queries, pq, pr))                               # the bound's default again
    lib().kp_release_scratch()
    assert same(dot(dc, queries, pq, pr))                               # a fresh workspace


# ---------------------------------------------------------------------------------------------------------
# 5. the device mirror follows the index
# ---------------------------------------------------------------------------------------------------------
def contents(ix, ids):
    """the index's current contents through its public ``get``, as a corpus in the order of ``ids``"""
    return PU.corpus_of(ix.vocab_size, [(t, w.astype(np.float32)) for t, w in (ix.get(i) for i in ids)])


def check_score_pairs(ix, ids, queries):
    c = contents(ix, ids)
    got = ix.score_pairs(queries, [ids] * len(queries))
    pq, pr = PU.all_pairs(len(queries), len(ids))
    assert all(g.dtype == np.float32 and len(g) == len(ids) for g in got)
    assert np.array_equal(U.bits(np.concatenate(got)), U.bits(PU.ref_pairs(c, queries, pq, pr)))
    return got


def test_the_mirror_follows_adds_drops_and_a_round_trip(tmp_path):
    from kirag_amd.retriever.sparse_index import SparseIndexer
    a, b = U.random_corpus(1031, 250, seed=41), U.random_corpus(1031, 40, seed=42)
    ids = [str(7 * i + 1) for i in range(250)]
    queries = [U.random_query(1031, m, seed=m + 50) for m in (2, 33, 200)]
    ix = SparseIndexer(1031, device="cuda:0")
    ix.index_data(ids[:100], a.pairs(0, 100))
    ix.search_knn(queries, 5)
    assert ix._d_terms is None and ix._synced == 0                     # lazy: a search mirrors nothing
    check_score_pairs(ix, ids[:100], queries)
    assert ix._synced == ix.nnz
    ix.index_data(ids[100:], a.pairs(100, 250))                        # more rows: only the suffix is uploaded
    before = ix._synced
    assert before < ix.nnz
    check_score_pairs(ix, ids, queries)
    assert ix._synced == ix.nnz
    ix._drop_last(40)                                                  # 40 rows leave, 40 OTHER rows take their ids and their place in the arrays
    assert ix._synced == ix.nnz == int(a.row_off[210])
    check_score_pairs(ix, ids[:210], queries)
    ix.index_data(ids[210:], b.pairs())
    got = check_score_pairs(ix, ids, queries)
    assert np.array_equal(ix.get(ids[210])[0], b.row(0)[0])
    # rerank: (score descending, position ascending), ids as strings
    order = np.lexsort((np.arange(250), -got[1].astype(np.float64)))
    top_ids, top_scores = ix.rerank(queries[1], ids, top_k=7)
    assert top_ids == [ids[i] for i in order[:7]] and np.array_equal(U.bits(top_scores), U.bits(got[1][order[:7]]))
    assert ix.rerank(queries[1], ids)[0] == [ids[i] for i in order]
    assert [len(g) for g in ix.score_pairs(queries, [[], ids[:3], []])] == [0, 3, 0]
    assert ix.score_pairs([], []) == []
    with pytest.raises(KeyError, match="id 5 is not in the index"):
        ix.score_pairs(queries[:1], [[ids[0], "5"]])
    # a round trip through the file: the new index mirrors from nothing, the old one is reset and loads again
    ix.serialize(str(tmp_path))
    other = SparseIndexer(1031, device="cuda:0")
    other.deserialize_from(str(tmp_path))
    assert other._synced == 0
    again = check_score_pairs(other, ids, queries)
    assert all(np.array_equal(U.bits(x), U.bits(y)) for x, y in zip(again, got))
    ix.deserialize_from(str(tmp_path))
    assert ix._synced == 0 and ix._d_terms is None
    check_score_pairs(ix, ids, queries)


# ---------------------------------------------------------------------------------------------------------
# 6. end to end: the three stored forms of bge-m3 together; rank fusion over real hit lists
# ---------------------------------------------------------------------------------------------------------
N_PASSAGES, N_QUERIES, P = 64, 8, 128
# Test (2) below orders by the HF fp32 reference wherever its neighbouring combined scores differ by more than a margin, the margin being twice the worst
# |combined - reference combined| measured on these very cases on one MI355X (profiles/pairs/measurements.txt, section 3):
#     xlmr (synthetic, 64 passages, 8 queries, all 512 pairs)   worst measured 1.739e-05, on scores up to 0.591
#     bert                                                       worst measured 1.943e-05, on scores up to 0.580
# Checked on the CPU before the GPU run that set the order rule's margin (twice the bar, 4 x worst): of the reference's own neighbouring pairs 71 of 504 (xlmr)
# and 79 of 504 (bert) lie within it, under the cap of a quarter.
HYBRID_WORST = {"xlmr": 1.8e-5, "bert": 2.0e-5}


@functools.lru_cache(maxsize=None)
def m3_case(kind):
    import m3_util as M
    import xlmr_util as X
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.late import MultiVectorStore
    from kirag_amd.retriever.m3 import BertM3Encoder, BGEM3Model, XLMRobertaM3Encoder
    from kirag_amd.retriever.sparse_index import SparseIndexer
    hw = M.heads_for(kind, P)
    enc = M.hf_backbone(kind, M.backbone(kind), "cuda", cls=XLMRobertaM3Encoder if kind == "xlmr" else BertM3Encoder)
    enc.set_heads({"weight": torch.from_numpy(hw[M.HEADS[0]]), "bias": torch.from_numpy(hw[M.HEADS[1]])},
                  {"weight": torch.from_numpy(hw[M.HEADS[2]]), "bias": torch.from_numpy(hw[M.HEADS[3]])})
    tok = X.toy_tokenizer()
    m3 = BGEM3Model(enc, tokenizer=tok)
    passages, queries = M.texts(N_PASSAGES, seed=5, lo=3, hi=24), M.texts(N_QUERIES, seed=105, lo=6, hi=16)
    ids = [str(500 + 3 * k) for k in range(N_PASSAGES)]
    indexer, store, sp = Indexer(128), MultiVectorStore(P, device="cuda:0"), SparseIndexer(len(tok), device="cuda:0")
    m3.index_passages(ids, passages, indexer, store, batch_size=24, sparse_index=sp)
    return m3, hw, tok, passages, queries, ids, indexer, store, sp


def parts(m3, queries, indexer, store, sp, n):
    """the three public parts for the dense top-n of each query: (ids, dense, sparse, colbert)"""
    q = m3.encode(list(queries), return_dense=True, return_sparse=True, return_colbert_vecs=True)
    hits = indexer.search_knn(q["dense_vecs"], n, verbose=False)
    cands = [[str(i) for i in h[0]] for h in hits]
    return cands, [np.asarray(h[1], np.float64) for h in hits], sp.score_pairs(q["lexical_weights"], cands), store.maxsim(q["colbert_vecs"], cands, reduce="mean")


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_retrieve_hybrid_is_the_formula_over_the_three_public_parts(kind):
    m3, _, _, _, queries, ids, indexer, store, sp = m3_case(kind)
    for weights, n, top_k in (((1.0, 1.0, 1.0), N_PASSAGES, N_PASSAGES), ((0.4, 0.2, 0.4), 20, 5)):
        wd, ws, wc = weights
        cands, dense, sparse, colbert = parts(m3, queries, indexer, store, sp, n)
        got = m3.retrieve_hybrid(queries, indexer, store, sp, top_k=top_k, n_candidates=n, weights=weights)
        two = m3.retrieve_hybrid(queries, indexer, None, sp, top_k=top_k, n_candidates=n, weights=weights)
        assert len(got) == len(two) == N_QUERIES
        for i in range(N_QUERIES):
            for res, s in ((got[i], (wd * dense[i] + ws * sparse[i].astype(np.float64) + wc * colbert[i].astype(np.float64)) / (wd + ws + wc)),
                           (two[i], (wd * dense[i] + ws * sparse[i].astype(np.float64)) / (wd + ws))):
                order = sorted(range(n), key=lambda j: (-s[j], j))[:top_k]             # (combined descending, dense rank ascending)
                assert res[0] == [cands[i][j] for j in order]
                assert res[1].dtype == np.float32 and np.array_equal(U.bits(res[1]), U.bits(s[order].astype(np.float32)))
        assert any((sp_i > 0).any() for sp_i in sparse)                                # the sparse head does take part
    one = m3.retrieve_hybrid(queries[0], indexer, store, sp, top_k=3)                  # one query as a string
    assert len(one) == 1 and one[0][0] == m3.retrieve_hybrid(queries, indexer, store, sp, top_k=3)[0][0]
    empty = m3.retrieve_hybrid(queries[:2], indexer, store, sp, n_candidates=0)
    assert [len(e[0]) for e in empty] == [0, 0] and all(e[1].dtype == np.float32 and len(e[1]) == 0 for e in empty)


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_retrieve_hybrid_refuses_a_candidate_one_container_lacks(kind):
    from kirag_amd.retriever.late import MultiVectorStore
    from kirag_amd.retriever.sparse_index import SparseIndexer
    m3, _, tok, _, queries, ids, indexer, store, sp = m3_case(kind)
    with pytest.raises(KeyError, match="not in the index"):
        m3.retrieve_hybrid(queries[:2], indexer, store, SparseIndexer(len(tok), device="cuda:0"), n_candidates=5)
    with pytest.raises(KeyError):
        m3.retrieve_hybrid(queries[:2], indexer, MultiVectorStore(P, device="cuda:0"), sp, n_candidates=5)


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_retrieve_hybrid_against_the_hf_reference(kind):
    """(2): |combined - reference combined| stays within the bar — twice the worst measured on these cases, 3.6e-5 (xlmr) and 4.0e-5 (bert), see
    HYBRID_WORST — and the ids follow the reference's order wherever its neighbours differ by more than twice the bar; at most a quarter of the
    neighbouring pairs may lie closer."""
    import m3_util as M
    m3, hw, tok, passages, queries, ids, indexer, store, sp = m3_case(kind)
    got = m3.retrieve_hybrid(queries, indexer, store, sp, top_k=N_PASSAGES, n_candidates=N_PASSAGES)
    hf_model = M.hf_backbone(kind, M.backbone(kind), "cuda")
    rq, rp = M.ref_encode(hf_model, hw, tok, queries), M.ref_encode(hf_model, hw, tok, passages)
    hf = np.array([[M.ref_scores(a, b)["colbert+sparse+dense"] for b in rp] for a in rq])
    worst, skipped, checked = 0.0, 0, 0
    for i, (got_ids, got_scores) in enumerate(got):
        assert sorted(got_ids) == sorted(ids)
        col = np.array([ids.index(x) for x in got_ids], np.int64)
        worst = max(worst, float(np.abs(got_scores.astype(np.float64) - hf[i, col]).max()))
    print(f"hybrid {kind}: worst |combined - reference| {worst:.3e} on scores up to {np.abs(hf).max():.3f}")
    bar = 2 * HYBRID_WORST[kind]
    assert worst <= bar
    for i, (got_ids, _) in enumerate(got):
        rank = {x: j for j, x in enumerate(got_ids)}
        order = np.argsort(-hf[i], kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            if hf[i, a] - hf[i, b] > 2 * bar:
                checked += 1
                assert rank[ids[a]] < rank[ids[b]], (kind, i, ids[a], ids[b])
            else:
                skipped += 1
    print(f"hybrid {kind}: {skipped} of {skipped + checked} neighbouring pairs of the reference lie within {2 * bar:.3e}")
    assert checked > 0 and skipped <= (skipped + checked) / 4


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_retrieve_rrf_is_rrf_over_the_two_searches_and_maxsim_over_their_union(kind):
    from kirag_amd.retriever.fusion import rrf
    m3, _, _, _, queries, ids, indexer, store, sp = m3_case(kind)
    n = 12
    q = m3.encode(list(queries), return_dense=True, return_sparse=True, return_colbert_vecs=True)
    dense = [[str(i) for i in h[0]] for h in indexer.search_knn(q["dense_vecs"], n, verbose=False)]
    sparse = [h[0] for h in m3.retrieve_sparse(queries, sp, top_k=n)]
    got = m3.retrieve_rrf(queries, indexer, sp, top_k=10, n_candidates=n, k=20.0)
    with_store = m3.retrieve_rrf(queries, indexer, sp, top_k=10, n_candidates=n, k=20.0, store=store)
    differ = 0
    for i in range(N_QUERIES):
        want_ids, want = rrf([dense[i], sparse[i]], k=20.0, top_k=10)
        assert got[i][0] == want_ids and np.array_equal(got[i][1], want)
        union = dense[i] + [x for x in sparse[i] if x not in dense[i]]
        col = store.maxsim([q["colbert_vecs"][i]], [union], reduce="mean")[0]
        third = [union[j] for j in sorted(range(len(union)), key=lambda j: (-float(col[j]), j))]
        want_ids, want = rrf([dense[i], sparse[i], third], k=20.0, top_k=10)
        assert with_store[i][0] == want_ids and np.array_equal(with_store[i][1], want)
        differ += len(union) > n
    assert differ > 0                                                    # the sparse search did bring candidates the dense one had not


def test_fuse_hits_over_splade_retrieve_and_a_dense_index():
    """how a dense retriever meets SpladeModel: the two per-query hit lists, fused by rank"""
    import reranker_util as RU
    import splade_util as S
    from kirag_amd.retriever.fusion import fuse_hits, rrf
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.sparse_index import SparseIndexer
    from kirag_amd.retriever.splade import BertSpladeEncoder, SpladeModel
    tok = RU.bert_pair_tokenizer()
    V = tok.vocab_size
    model = SpladeModel(S.hf_mlm("h64", V, S.tied_weights(V), "cuda", cls=BertSpladeEncoder, tie=True), tokenizer=tok)
    passages, queries = RU.passages(N_PASSAGES, seed=12), RU.passages(N_QUERIES, seed=11, lo=8, hi=12)
    ids = [str(700 + 3 * i) for i in range(N_PASSAGES)]
    ix = SparseIndexer(V, device="cuda:0")
    model.index_passages(ids, passages, ix, batch_size=24)
    rng = np.random.default_rng(3)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    dense_index = Indexer(128)
    dense_index.index_data(ids, unit(rng.standard_normal((N_PASSAGES, 128))))
    dense_hits = dense_index.search_knn(unit(rng.standard_normal((N_QUERIES, 128))), 15, verbose=False)
    splade_hits = model.retrieve(queries, ix, top_k=15)
    fused = fuse_hits(dense_hits, splade_hits, top_k=10)
    assert len(fused) == N_QUERIES
    for i, (got_ids, got_scores) in enumerate(fused):
        want_ids, want = rrf([[str(x) for x in dense_hits[i][0]], list(splade_hits[i][0])], top_k=10)
        assert [str(x) for x in got_ids] == want_ids and got_scores.dtype == np.float32
        assert np.array_equal(got_scores, want.astype(np.float32))
        assert len(got_ids) == 10 and set(got_ids) <= set(ids)
