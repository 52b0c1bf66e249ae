"""libkirag_pairs.so, kirag_amd.retriever.fusion and SparseIndexer.score_pairs without a GPU: the header, the binding and the built library name the same four
functions; kp_sparse_dot refuses every malformed argument by field before a device is asked for, and a well-formed call finds no device; reciprocal rank fusion
against a literal restatement in Python floats, every tie level of its order rule built on purpose; the refusals of score_pairs that need no launch; and the
pair reference of tests/pairs_util.py notices the mutations the GPU tests rely on it to notice."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_util as PU  # noqa: E402
import sparse_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kirag_pairs.h")


@pytest.fixture(scope="module")
def lib():
    from kirag_amd import _pairs_lib
    if not os.path.exists(_pairs_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _pairs_lib.load()


def last_error(lib):
    return lib.kp_last_error().decode()


def no_gpu():
    import torch
    return not torch.cuda.is_available()


# ---- header and ABI ----
def test_header_binding_and_library_agree_on_the_four_functions(lib):
    from kirag_amd import _pairs_lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert set(re.findall(r"\b(k[pslr]_[a-z0-9_]+)\s*\(", text)) == PU.EXPORTS
    assert set(_pairs_lib.SIGNATURES) == PU.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", _pairs_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()}
    assert {s for s in exported if s.startswith(("kp_", "ks_", "kl_", "kr_"))} == PU.EXPORTS
    assert re.search(r"#define\s+KP_ABI_VERSION\s+1\b", text) and lib.kp_abi_version() == 1 == _pairs_lib.ABI_VERSION
    assert (_pairs_lib.MAX_QUERIES, _pairs_lib.MAX_PAIRS, _pairs_lib.MAX_STAGED_PAIRS) == (65535, 1 << 24, 1 << 20)
    assert re.search(r"#define\s+KP_MAX_QUERIES\s+65535\b", text) and re.search(r"#define\s+KP_MAX_PAIRS\s+\(1 << 24\)", text)
    assert re.search(r"#define\s+KP_MAX_STAGED_PAIRS\s+\(1 << 20\)", text)


def test_error_codes_carry_the_values_of_the_codes_they_mirror():
    from kirag_amd import _pairs_lib
    mine, main = open(HEADER).read(), open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    for name in ("EINVAL", "ENOMEM", "ENODEV", "EHIP"):
        a = re.search(r"#define\s+KP_%s\s+\((-?\d+)\)" % name, mine).group(1)
        b = re.search(r"#define\s+KR_%s\s+\((-?\d+)\)" % name, main).group(1)
        assert a == b and int(a) == getattr(_pairs_lib, name)


def test_library_links_the_hip_runtime_and_no_project_library():
    from kirag_amd import _pairs_lib
    out = subprocess.run(["readelf", "-d", _pairs_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.+?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed)
    assert not [n for n in needed if "kirag" in n]


def test_release_scratch_without_a_workspace_is_a_no_op(lib):
    lib.kp_release_scratch()
    assert lib.kp_abi_version() == 1


# ---- refusals that need no device ----
_BUFFERS = {}


def buffers():
    """(terms, weights, out) device addresses.  Without a GPU they are fake: every call ends at the argument checks or at the search for a device, nothing
    behind them is read.  With one, the calls that pass the checks RUN, so the addresses are those of real, zero-filled tensors of 64 elements."""
    if not _BUFFERS:
        if no_gpu():
            _BUFFERS["addr"] = (0x1000, 0x2000, 0x3000)
        else:
            import torch
            _BUFFERS["keep"] = [torch.zeros(64, dtype=dt, device="cuda:0") for dt in (torch.int32, torch.float16, torch.float32)]
            _BUFFERS["addr"] = tuple(t.data_ptr() for t in _BUFFERS["keep"])
    return _BUFFERS["addr"]


DEFAULT = object()


def call(lib, row_off=(0, 3, 3, 7), nnz=7, N=None, V=100, q_off=(0, 2, 2), q_term=(3, 5), q_w=(1.0, 2.0), nq=None, pair_q=(0, 1, 0), pair_row=(0, 2, 1),
         npairs=None, terms=DEFAULT, weights=DEFAULT, out=DEFAULT, device=0):
    """``None`` for an array passes a null pointer; ``terms`` / ``weights`` / ``out``: ``buffers()`` unless given"""
    terms, weights, out = (b if a is DEFAULT else a for a, b in zip((terms, weights, out), buffers()))
    arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    ptr = lambda a: None if a is None else a.ctypes.data
    row_off, q_off, pair_q, pair_row = arr(row_off, np.int64), arr(q_off, np.int64), arr(pair_q, np.int64), arr(pair_row, np.int64)
    q_term, q_w = arr(q_term, np.int32), arr(q_w, np.float32)
    if N is None:
        N = len(row_off) - 1
    if nq is None:
        nq = len(q_off) - 1
    if npairs is None:
        npairs = len(pair_q)
    return lib.kp_sparse_dot(terms, weights, nnz, ptr(row_off), N, V, ptr(q_off), nq, ptr(q_term), ptr(q_w), ptr(pair_q), ptr(pair_row), npairs, out, device,
                             None)


def PAST_THE_CHECKS():
    """what a well-formed call returns: KP_ENODEV where there is no device, KP_OK where there is one (the call then runs on ``buffers()``)"""
    return -19 if no_gpu() else 0


def refused(lib, field, **kw):
    assert call(lib, **kw) == -22, (kw, last_error(lib))
    assert field in last_error(lib), (field, last_error(lib))


def test_sizes_outside_their_ranges_are_refused_by_name(lib):
    refused(lib, "V=0", V=0)
    refused(lib, "V=16777217", V=(1 << 24) + 1)
    refused(lib, "N=-1", N=-1)
    refused(lib, "N=2147483649", N=(1 << 31) + 1)
    refused(lib, "nnz=-1", nnz=-1)
    refused(lib, "npairs=-1", npairs=-1)
    refused(lib, "npairs=16777217", npairs=(1 << 24) + 1)
    refused(lib, "nq=-1", nq=-1)
    refused(lib, "nq=65536", q_off=np.zeros(65537, np.int64), q_term=(), q_w=(), pair_q=(), pair_row=())


def test_query_offsets_must_start_at_zero_and_not_decrease(lib):
    refused(lib, "q_off[0]=1", q_off=(1, 2, 2))
    refused(lib, "q_off[2]=1", q_off=(0, 2, 1))
    refused(lib, "q_off is null", q_off=None, nq=2)


def test_query_terms_must_ascend_strictly_and_lie_in_the_vocabulary(lib):
    refused(lib, "q_term[1]=3", q_term=(5, 3))
    refused(lib, "q_term[1]=5", q_term=(5, 5))
    refused(lib, "q_term[1]=100", q_term=(3, 100))
    refused(lib, "q_term[0]=-1", q_term=(-1, 4))
    refused(lib, "q_term[0]=5", q_off=(0, 1, 2), q_term=(5, 3), V=2)          # ascending is a rule within a query: the next query starts anew
    assert call(lib, q_off=(0, 1, 2), q_term=(5, 3)) == PAST_THE_CHECKS(), last_error(lib)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_a_query_weight_that_is_not_finite_and_positive_is_refused_by_name(lib, bad):
    refused(lib, "q_w[1]=", q_w=(1.0, bad))


def test_pairs_must_name_a_query_and_a_row(lib):
    refused(lib, "pair_q[1]=2", pair_q=(0, 2, 0))
    refused(lib, "pair_q[0]=-1", pair_q=(-1, 1, 0))
    refused(lib, "pair_q[0]=0", q_off=(0,), q_term=(), q_w=(), pair_q=(0,), pair_row=(0,))       # nq = 0: no query to name
    refused(lib, "pair_row[2]=3", pair_row=(0, 2, 3))
    refused(lib, "pair_row[1]=-1", pair_row=(0, -1, 1))
    refused(lib, "pair_row[0]=0", row_off=(0,), nnz=0, pair_q=(0,), pair_row=(0,))               # N = 0: no row to name


def test_the_offsets_of_a_referenced_row_are_checked_and_no_others(lib):
    refused(lib, "row_off[0]=-1", row_off=(-1, 3, 3, 7))
    refused(lib, "row_off[2]=2", row_off=(0, 3, 2, 7), pair_row=(1, 1, 1))
    refused(lib, "row_off[3]=8", row_off=(0, 3, 3, 8))
    refused(lib, "row_off[3]", row_off=(0, 3, 3, 7), V=3, q_term=(1, 2))                          # a row of 4 entries over 3 terms
    assert "more than V=3" in last_error(lib)
    # rows no pair names are not read: the garbage around row 1 is not met, the call gets as far as the device
    assert call(lib, row_off=(-5, 3, 3, 99), pair_row=(1, 1, 1)) == PAST_THE_CHECKS(), last_error(lib)


def test_a_null_pointer_that_is_needed_is_refused_by_name(lib):
    refused(lib, "q_term / q_w is null", q_term=None)
    refused(lib, "q_term / q_w is null", q_w=None)
    refused(lib, "pair_q / pair_row is null", pair_q=None, npairs=3)
    refused(lib, "pair_q / pair_row is null", pair_row=None, npairs=3)
    refused(lib, "row_off is null", row_off=None, N=3)
    refused(lib, "terms / weights is null", terms=None)
    refused(lib, "terms / weights is null", weights=None)
    refused(lib, "out is null", out=None)
    # not needed: pairs that name only an empty row read no entry
    assert call(lib, terms=None, weights=None, pair_row=(1, 1, 1)) == PAST_THE_CHECKS(), last_error(lib)


def test_a_misaligned_pointer_is_refused_by_name(lib):
    t, w, o = buffers()
    for kw, name in (({"terms": t + 2}, "terms="), ({"weights": w + 1}, "weights="), ({"out": o + 2}, "out=")):
        refused(lib, name, **kw)
        assert "aligned" in last_error(lib)


def test_no_pairs_is_ok_without_a_device(lib):
    assert call(lib, pair_q=(), pair_row=()) == 0
    assert call(lib, pair_q=None, pair_row=None, npairs=0, row_off=None, N=0, terms=None, weights=None, out=None) == 0
    refused(lib, "q_term[1]=3", q_term=(5, 3), pair_q=(), pair_row=())          # the argument checks still come first


def test_a_well_formed_call_without_a_device_is_enodev(lib):
    rc = call(lib)
    assert rc == PAST_THE_CHECKS(), last_error(lib)
    if no_gpu():
        assert rc == -19 and "no HIP device" in last_error(lib)
    refused(lib, "pair_q[1]=2", pair_q=(0, 2, 0))                               # and a malformed one is EINVAL first


def test_a_device_out_of_range(lib):
    """the ordinal can only be checked where devices are counted: without one the call ends at KP_ENODEV as every well-formed call does"""
    for device in (1000, -1):
        if no_gpu():
            assert call(lib, device=device) == -19
        else:
            refused(lib, "device %d" % device, device=device)


# ---- reciprocal rank fusion against a literal restatement ----
def literal_rrf(rankings, k=60.0, weights=None, top_k=None):
    """the definition in Python floats: per id the sum over the systems in order, then a sort by (-score, best rank, first system giving it)"""
    weights = [1.0] * len(rankings) if weights is None else list(weights)
    ids = []
    for r in rankings:
        for i in r:
            if i not in ids:
                ids.append(i)
    rows = []
    for i in ids:
        score, ranks = 0.0, []
        for s, r in enumerate(rankings):
            if i in r:
                rank = r.index(i) + 1
                score = score + weights[s] / (k + rank)
                ranks.append((rank, s))
        rows.append((-score, min(ranks)[0], min(ranks)[1], i))
    rows.sort(key=lambda t: t[:3])
    rows = rows if top_k is None else rows[:top_k]
    return [t[3] for t in rows], [-t[0] for t in rows]


RANKINGS = {
    "two": [["a", "b", "c", "d"], ["c", "a", "e"]],
    "three": [["a", "b", "c", "d"], ["c", "a", "e"], ["e", "d", "f", "a", "g"]],
    "disjoint": [["a", "b"], ["c", "d", "e"]],
    "nested": [["a", "b", "c", "d", "e"], ["b", "c"]],
    "identical": [["x", "y", "z"], ["x", "y", "z"], ["x", "y", "z"]],
    "one empty": [[], ["p", "q"]],
    "integers": [[5, 3, 9], [9, 5, 11, 3]],
}


@pytest.mark.parametrize("name", sorted(RANKINGS))
def test_rrf_equals_the_literal_restatement(name):
    from kirag_amd.retriever.fusion import rrf
    r = RANKINGS[name]
    for kw in ({}, {"k": 1.0}, {"k": 0.5, "weights": [2.0, 0.25, 1.0][:len(r)]}, {"weights": [0.0] + [1.0] * (len(r) - 1)}, {"top_k": 2}, {"top_k": 0}):
        ids, scores = rrf(r, **kw)
        want_ids, want_scores = literal_rrf(r, **kw)
        assert ids == want_ids, (name, kw)
        assert scores.dtype == np.float64 and scores.tolist() == want_scores, (name, kw)      # the same float64 sums, bit for bit


def test_rrf_tie_levels_of_the_order_rule():
    from kirag_amd.retriever.fusion import rrf
    # level 1, the score decides: b is second twice (2 / 62), a is first once (1 / 61)
    ids, s = rrf([["a", "b"], ["c", "b"]])
    assert ids[0] == "b" and s[0] == 1 / 62 + 1 / 62 > s[1]
    # level 2, equal scores, different best ranks.  With k = 1: x at ranks 1 and 5 scores 1/2 + 1/6 = 2/3; y at ranks 2 and 2 scores 1/3 + 1/3 = 2/3
    sys1, sys2 = ["x", "y", "f1", "f2", "f3"], ["g1", "y", "g2", "g3", "x"]
    ids, s = rrf([sys1, sys2], k=1.0)
    assert s[ids.index("x")] == s[ids.index("y")], "the case must tie in float64 to test the rule"
    assert ids.index("x") < ids.index("y")                          # best rank 1 before best rank 2
    ids, s = rrf([sys2, sys1], k=1.0)                               # the systems exchanged: the same scores and best ranks, the same order
    assert s[ids.index("x")] == s[ids.index("y")] and ids.index("x") < ids.index("y")
    # level 3, equal scores and equal best ranks from different systems: the system listed first wins
    ids, s = rrf([["u", "m"], ["v", "n"]])
    assert s[0] == s[1] and ids[:2] == ["u", "v"] and ids[2:] == ["m", "n"]
    ids, _ = rrf([["v", "n"], ["u", "m"]])
    assert ids == ["v", "u", "n", "m"]
    # all three levels in one call agree with the literal restatement
    r = [sys1, sys2, ["u", "x"], ["v", "y"]]
    assert rrf(r, k=1.0)[0] == literal_rrf(r, k=1.0)[0]


def test_rrf_refusals():
    from kirag_amd.retriever.fusion import rrf
    with pytest.raises(ValueError, match="occurs twice"):
        rrf([["a", "b", "a"]])
    for k in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="k="):
            rrf([["a"]], k=k)
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"weights\[1\]"):
            rrf([["a"], ["b"]], weights=[1.0, w])
    with pytest.raises(ValueError, match="1 weights for 2 rankings"):
        rrf([["a"], ["b"]], weights=[1.0])
    assert rrf([]) [0] == [] and rrf([[], []])[0] == []


def test_fuse_hits_is_rrf_per_query_over_the_id_lists():
    from kirag_amd.retriever.fusion import fuse_hits
    dense = [(["1", "2", "3"], [0.9, 0.8, 0.7]), (["7"], [0.5]), ([], [])]
    sparse = [(["3", "1", "4"], np.array([12.0, 3.0, 1.0], np.float32)), (["8", "7"], [2.0, 1.0]), (["5"], [1.0])]
    got = fuse_hits(dense, sparse, top_k=2, k=10.0, weights=(1.0, 0.5))
    assert len(got) == 3
    for q, (ids, scores) in enumerate(got):
        want_ids, want = literal_rrf([list(dense[q][0]), list(sparse[q][0])], k=10.0, weights=(1.0, 0.5), top_k=2)
        assert ids == want_ids and scores.dtype == np.float32
        assert np.array_equal(scores, np.asarray(want, np.float64).astype(np.float32))
    assert len(fuse_hits(dense, sparse)[0][0]) == 4                  # top_k = 10 by default
    three = fuse_hits(dense, sparse, dense, top_k=None)
    assert three[0][0] == literal_rrf([["1", "2", "3"], ["3", "1", "4"], ["1", "2", "3"]])[0]
    with pytest.raises(ValueError, match="results\\[1\\] holds 2 queries"):
        fuse_hits(dense, sparse[:2])
    with pytest.raises(ValueError):
        fuse_hits()


# ---- SparseIndexer.score_pairs: what is refused before any launch ----
def cpu_index():
    from kirag_amd.retriever.sparse_index import SparseIndexer
    ix = SparseIndexer(97, device="cpu")
    c = U.random_corpus(97, 20, seed=4)
    ix.index_data([str(100 + i) for i in range(20)], c.pairs())
    return ix


def test_score_pairs_refusals_on_a_cpu_index():
    ix = cpu_index()
    q = [(np.array([3, 5], np.int32), np.array([1.0, 2.0], np.float32))]
    with pytest.raises(ValueError, match="1 queries, 2 candidate lists"):
        ix.score_pairs(q, [["100"], ["101"]])
    with pytest.raises(KeyError, match="id 999 is not in the index"):
        ix.score_pairs(q, [["100", "999"]])
    with pytest.raises(KeyError, match="not in the index"):
        ix.rerank(q[0], ["100", "nope"])
    with pytest.raises(RuntimeError, match="no torch scoring path"):
        ix.score_pairs(q, [["100", "101"]])
    with pytest.raises(RuntimeError, match="no torch scoring path"):
        ix.rerank(q[0], ["100", "101"], top_k=1)
    assert ix._d_terms is None and ix._synced == 0                   # nothing was mirrored


def test_the_mirror_mark_follows_drop_last_and_reset():
    ix = cpu_index()
    ix._synced = ix.nnz                                              # as if a score_pairs call had mirrored everything
    before = int(ix.row_off[15])
    ix._drop_last(5)
    assert ix._synced == before == ix.nnz
    ix._drop_last(0)
    assert ix._synced == before
    ix._reset()
    assert ix._synced == 0 and ix._d_terms is None and ix._d_weights is None


# ---- the pair reference has teeth ----
def test_the_pair_reference_reads_ref_scores_at_the_pairs_rows():
    c = U.random_corpus(97, 30, seed=6)
    queries = [U.random_query(97, m, seed=m) for m in (2, 33)] + [(np.empty(0, np.int32), np.empty(0, np.float32))]
    pq, pr = PU.all_pairs(3, c.N)
    got = PU.ref_pairs(c, queries, pq, pr)
    for q in range(2):
        assert np.array_equal(U.bits(got[q * c.N:(q + 1) * c.N]), U.bits(U.ref_scores(c, *queries[q])))
    assert (U.bits(got[2 * c.N:]) == PU.POS_ZERO).all()
    back = PU.ref_pairs(c, queries, pq[::-1], pr[::-1])
    assert np.array_equal(U.bits(back), U.bits(got[::-1]))
