"""libkirag_sparse.so and kirag_amd.retriever.sparse_index without a GPU: the header, the binding and the built library name the same functions; the
argument checks of ks_search / ks_count_positive / ks_compact_rows refuse by field before a device is asked for; the numpy inversion against a brute-force
per-term scan; SparseIndexer on the CPU (the three passage forms, max-merge, drop rule, refusals, the file format, the refusal to search); the model surface on
stubs; and the reference of tests/sparse_util.py notices every way the kernel could go wrong that the GPU tests rely on it to notice."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kirag_sparse.h")
EXPORTS = {"ks_abi_version", "ks_last_error", "ks_release_scratch", "ks_block_rows", "ks_search", "ks_count_positive", "ks_compact_rows"}


@pytest.fixture(scope="module")
def lib():
    from kirag_amd import _sparse_lib
    if not os.path.exists(_sparse_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _sparse_lib.load()


def last_error(lib):
    return lib.ks_last_error().decode()


def R_():
    from kirag_amd import _sparse_lib
    return _sparse_lib.block_rows()


# ---- header and ABI ----
def test_header_binding_and_library_agree_on_the_exported_functions(lib):
    from kirag_amd import _sparse_lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(k[slr]_[a-z0-9_]+)\s*\(", text))
    assert declared == EXPORTS
    assert set(_sparse_lib.SIGNATURES) == EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", _sparse_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()}
    assert {s for s in exported if s.startswith(("ks_", "kl_", "kr_"))} == EXPORTS
    assert re.search(r"#define\s+KS_ABI_VERSION\s+1\b", text) and lib.ks_abi_version() == 1 == _sparse_lib.ABI_VERSION
    assert lib.ks_block_rows() in (16384, 32768)
    assert (_sparse_lib.MAX_K, _sparse_lib.MAX_QUERIES, _sparse_lib.MAX_SKIP) == tuple(
        int(re.search(r"#define\s+KS_%s\s+(\d+)" % n, text).group(1)) for n in ("MAX_K", "MAX_QUERIES", "MAX_SKIP"))


def test_error_codes_carry_the_values_of_the_codes_they_mirror():
    from kirag_amd import _sparse_lib
    mine, main = open(HEADER).read(), open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    for name in ("EINVAL", "ENOMEM", "ENODEV", "EHIP", "ERANGE"):
        a = re.search(r"#define\s+KS_%s\s+\((-?\d+)\)" % name, mine).group(1)
        b = re.search(r"#define\s+KR_%s\s+\((-?\d+)\)" % name, main).group(1)
        assert a == b and int(a) == getattr(_sparse_lib, name)


def test_library_links_the_hip_runtime_and_no_project_library():
    from kirag_amd import _sparse_lib
    out = subprocess.run(["readelf", "-d", _sparse_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.+?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed)
    assert not [n for n in needed if "kirag" in n]


def test_release_scratch_without_a_workspace_is_a_no_op(lib):
    lib.ks_release_scratch()
    assert lib.ks_abi_version() == 1


# ---- refusals that need no device ----
def call_search(lib, q_off=(0, 2), q_term=(3, 5), q_w=(1.0, 2.0), k=10, N=10, V=100, post_off=None, nq=None, post=0x1000, ptr=0x2000, out_score=0x3000,
                out_row=0x4000):
    """fake device addresses: every case is refused by the checks that run before a device is selected, nothing behind them is read"""
    q_off, q_term, q_w = np.asarray(q_off, np.int64), np.asarray(q_term, np.int32), np.asarray(q_w, np.float32)
    blocks = -(-N // R_()) if N > 0 else 0
    post_off = np.asarray(post_off if post_off is not None else [0] + [7] * blocks, np.int64)
    return lib.ks_search(post, ptr, post_off.ctypes.data, N, V, q_off.ctypes.data, len(q_off) - 1 if nq is None else nq, q_term.ctypes.data, q_w.ctypes.data,
                         k, out_score, out_row, 0, None)


def test_query_terms_must_ascend_strictly_and_lie_in_the_vocabulary(lib):
    assert call_search(lib, q_term=(5, 3)) == -22 and "q_term[1]=3" in last_error(lib)
    assert call_search(lib, q_term=(5, 5)) == -22 and "q_term[1]=5" in last_error(lib)
    assert call_search(lib, q_term=(3, 100)) == -22 and "q_term[1]=100" in last_error(lib)
    assert call_search(lib, q_term=(-1, 4)) == -22 and "q_term[0]=-1" in last_error(lib)
    # ascending is a rule within a query: the next query starts anew
    assert call_search(lib, q_off=(0, 1, 2), q_term=(5, 3), q_w=(1.0, 1.0), V=2) == -22 and "q_term[0]=5" in last_error(lib)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_a_query_weight_that_is_not_finite_and_positive_is_refused_by_name(lib, bad):
    assert call_search(lib, q_w=(1.0, bad)) == -22
    assert "q_w[1]=" in last_error(lib)


@pytest.mark.parametrize("k", [0, 1025, -3])
def test_k_outside_1_to_1024_is_refused_by_name(lib, k):
    assert call_search(lib, k=k) == -22
    assert "k=%d" % k in last_error(lib)


def test_nq_of_65536_is_refused_by_name(lib):
    off = np.zeros(65537, np.int64)
    assert call_search(lib, q_off=off, q_term=(), q_w=()) == -22
    assert "nq=65536" in last_error(lib)
    assert call_search(lib, nq=-1) == -22 and "nq=-1" in last_error(lib)


def test_offsets_must_start_at_zero_and_not_decrease(lib):
    assert call_search(lib, q_off=(1, 2)) == -22 and "q_off[0]=1" in last_error(lib)
    assert call_search(lib, q_off=(0, 2, 1), q_term=(3, 5), q_w=(1.0, 1.0)) == -22 and "q_off[2]=1" in last_error(lib)
    assert call_search(lib, post_off=(3, 7)) == -22 and "post_off[0]=3" in last_error(lib)
    assert call_search(lib, N=R_() + 1, post_off=(0, 9, 8)) == -22 and "post_off[2]=8" in last_error(lib)
    assert call_search(lib, N=-1, post_off=(0,)) == -22 and "N=-1" in last_error(lib)
    assert call_search(lib, V=0) == -22 and "V=0" in last_error(lib)


def test_a_misaligned_pointer_is_refused_by_name(lib):
    for kw, name in (({"post": 0x1002}, "post="), ({"ptr": 0x2001}, "ptr="), ({"out_score": 0x3002}, "out_score="), ({"out_row": 0x4004}, "out_row=")):
        assert call_search(lib, **kw) == -22
        assert name in last_error(lib) and "aligned" in last_error(lib)
    off = np.array([0, 1], np.int64)
    sk = np.zeros(1, np.int32)
    assert lib.ks_count_positive(0x1002, 1, 8, sk.ctypes.data, 0, off.ctypes.data, 0, None) == -22 and "block=" in last_error(lib)
    for args, name in (((0x1002, 0x2000, 0x3000), "block="), ((0x1000, 0x2002, 0x3000), "terms="), ((0x1000, 0x2000, 0x3001), "weights=")):
        assert lib.ks_compact_rows(args[0], 1, 8, sk.ctypes.data, 0, off.ctypes.data, args[1], args[2], 0, None) == -22
        assert name in last_error(lib) and "aligned" in last_error(lib)


def test_one_querys_candidates_must_fit_the_workspace_bound(lib):
    from kirag_amd import _sparse_lib
    _sparse_lib.set_candidate_bound(5)
    try:
        assert call_search(lib, k=10) == -22 and "workspace bound of 5" in last_error(lib)
    finally:
        _sparse_lib.set_candidate_bound(None)


def test_the_ingest_calls_refuse_by_name(lib):
    sk = np.array([3, 9], np.int32)
    cnt = np.zeros(2, np.int64)
    assert lib.ks_count_positive(0x1000, -1, 8, sk.ctypes.data, 0, cnt.ctypes.data, 0, None) == -22 and "B=-1" in last_error(lib)
    assert lib.ks_count_positive(0x1000, 2, 0, sk.ctypes.data, 0, cnt.ctypes.data, 0, None) == -22 and "V=0" in last_error(lib)
    assert lib.ks_count_positive(0x1000, 2, 8, sk.ctypes.data, 2, cnt.ctypes.data, 0, None) == -22 and "skip_terms[1]=9" in last_error(lib)
    assert lib.ks_count_positive(0x1000, 2, 8, sk.ctypes.data, 65, cnt.ctypes.data, 0, None) == -22 and "ns=65" in last_error(lib)
    for off, what in (((1, 2, 3), "row_off[0]=1"), ((0, 4, 3), "row_off[2]=3"), ((0, 9, 9), "row_off[1]")):
        off = np.asarray(off, np.int64)
        assert lib.ks_compact_rows(0x1000, 2, 8, sk.ctypes.data, 0, off.ctypes.data, 0x2000, 0x3000, 0, None) == -22 and what in last_error(lib)


# ---- the numpy inversion against a brute-force per-term scan ----
def brute_postings(c, r0, r1, t):
    """a scan of every entry of the corpus for term t: the postings of the rows r0 .. r1 - 1, in row order"""
    rows = np.repeat(np.arange(c.N, dtype=np.int64), np.diff(c.row_off))
    hit = (c.terms == t) & (rows >= r0) & (rows < r1)
    return (((rows[hit] - r0) << 16) | U.bits(c.w16)[hit].astype(np.int64)).tolist()


def check_block(c, r0, r1, ptr, post, terms):
    assert ptr.dtype == np.uint32 and post.dtype == np.uint32 and len(ptr) == c.V + 1
    assert ptr[0] == 0 and ptr[-1] == len(post) == c.row_off[r1] - c.row_off[r0] and (np.diff(ptr.astype(np.int64)) >= 0).all()
    for t in terms:
        assert post[ptr[t]:ptr[t + 1]].tolist() == brute_postings(c, r0, r1, t), t


def test_inversion_of_a_small_corpus_against_the_scan_term_by_term():
    from kirag_amd.retriever.sparse_index import invert_block
    c = U.random_corpus(97, 300, seed=1)
    a, b = c.row_off[119], c.row_off[120]                              # row 119 loses its terms: a passage without terms inside a block
    off = c.row_off.copy(); off[120:] -= b - a
    c = U.Corpus(97, off, np.delete(c.terms, slice(a, b)), np.delete(c.w32, slice(a, b)))
    assert c.row(119)[0].size == 0
    ptr, post = invert_block(c.row_off, c.terms, U.bits(c.w16), 0, 300, 97)
    check_block(c, 0, 300, ptr, post, range(97))
    ptr, post = invert_block(c.row_off, c.terms, U.bits(c.w16), 100, 164, 97)            # a block that starts inside the corpus: local rows start at 0
    check_block(c, 100, 164, ptr, post, range(97))


def cpu_index(V, token_to_id=None):
    from kirag_amd.retriever.sparse_index import SparseIndexer
    return SparseIndexer(V, device="cpu", token_to_id=token_to_id)


@pytest.fixture(scope="module")
def grown():
    """ONE CPU index fed in three steps to R - 1, R and R + 1 rows; term 5 is held by every row of block 0, row 7 holds nothing else, row 9 holds nothing"""
    R = R_()
    base = U.random_corpus(1031, R + 1, seed=2, lo=1, hi=6)
    rng = np.random.default_rng(3)
    terms = [np.union1d(base.row(r)[0], [5]) for r in range(R)] + [np.union1d(base.row(R)[0][base.row(R)[0] != 5], [6])]
    terms[7], terms[9] = np.array([5]), np.empty(0, np.int64)
    rows = [(t.astype(np.int32), rng.uniform(0.05, 3.0, len(t)).astype(np.float32)) for t in terms]
    off = np.zeros(R + 2, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=off[1:])
    c = U.Corpus(1031, off, np.concatenate([t for t, _ in rows]), np.concatenate([w for _, w in rows]))
    ix = cpu_index(1031)
    states = {}
    for n0, n1 in ((0, R - 1), (R - 1, R), (R, R + 1)):
        ix.index_data([str(i) for i in range(n0, n1)], rows[n0:n1])
        post_off = ix._sync_tail()
        states[n1] = (post_off.copy(), ix._closed, ix._ptr[:len(post_off) - 1].numpy().view(np.uint32).copy(), ix._post[:post_off[-1]].numpy().view(np.uint32).copy())
    return c, ix, states


def test_incremental_inversion_at_r_minus_1_r_and_r_plus_1(grown):
    c, ix, states = grown
    R = R_()
    probe = [0, 5, 6, 97, 1030] + np.random.default_rng(4).integers(0, 1031, 12).tolist()
    # R - 1 rows: one open tail block; R rows: one closed block and NO tail (post_off has two entries); R + 1: a one-row tail block behind the closed one
    post_off, closed, ptr, post = states[R - 1]
    assert closed == 0 and len(post_off) == 2
    check_block(c, 0, R - 1, ptr[0], post, probe)
    post_off, closed, ptr, post = states[R]
    assert closed == 1 and len(post_off) == 2
    check_block(c, 0, R, ptr[0], post, probe)
    assert ptr[0][6] - ptr[0][5] == R - 1                          # term 5: every row of block 0 but the empty row 9
    assert (post[ptr[0][5]:ptr[0][6]] >> 16).tolist() == [r for r in range(R) if r != 9]
    post_off, closed, ptr, post = states[R + 1]
    assert closed == 1 and len(post_off) == 3 and post_off[2] - post_off[1] == c.row_off[R + 1] - c.row_off[R]
    check_block(c, 0, R, ptr[0], post[:post_off[1]], probe[:4])
    check_block(c, R, R + 1, ptr[1], post[post_off[1]:], range(1031))
    assert ptr[1][6] == ptr[1][5]                                  # the tail row does not hold term 5
    assert ix.ntotal == R + 1 and ix.nnz == c.row_off[-1] and ix.get("9")[0].size == 0 and ix.get("7")[0].tolist() == [5]
    assert np.array_equal(ix.terms, c.terms) and np.array_equal(U.bits(ix.weights), U.bits(c.w16)) and np.array_equal(ix.row_off, c.row_off)


def test_drop_last_reopens_a_closed_block(grown):
    c, ix, _ = grown
    R = R_()
    other = cpu_index(1031)
    other.index_data([str(i) for i in range(R + 1)], c.pairs())
    other._drop_last(3)                                            # R - 2 rows: block 0 is the open tail again
    assert other.ntotal == R - 2 and other._closed == 0
    post_off = other._sync_tail()
    assert len(post_off) == 2 and post_off[1] == c.row_off[R - 2]
    check_block(c, 0, R - 2, other._ptr[0].numpy().view(np.uint32), other._post[:post_off[1]].numpy().view(np.uint32), [5, 0, 700])
    with pytest.raises(KeyError):
        other.get(str(R - 1))
    other.index_data([str(R - 2)], [c.row(R - 2)])                 # the dropped ids are free again
    assert other.ntotal == R - 1


# ---- SparseIndexer on the CPU: forms, merge, drop, refusals ----
def test_the_three_passage_forms_the_max_merge_and_the_drop_rule():
    tok = {"aa": 4, "bb": 9, "cc": 2}
    ix = cpu_index(16, token_to_id=tok.get)
    ix.index_data(["10"], [{"bb": 0.5, "aa": 1.25, "cc": 3.0}])
    assert ix.get("10")[0].tolist() == [2, 4, 9] and ix.get(10)[1].tolist() == [3.0, 1.25, 0.5]
    with pytest.raises(ValueError, match="unknown"):
        ix.index_data(["11"], [{"zz": 1.0}])
    ix = cpu_index(16)
    third = np.float32(1) / np.float32(3)
    ix.index_data(["1", "2", "3"], [{"7": 0.25, "3": 1.0}, (np.array([9, 2, 9, 2, 5]), np.array([0.5, 1.0, 0.75, third, 2.0])), ([], [])])
    assert ix.get("1")[0].tolist() == [3, 7] and ix.get("1")[1].dtype == np.float16 and ix.get("1")[0].dtype == np.int32
    t, w = ix.get("2")                       # duplicates keep the max, whatever their order
    assert t.tolist() == [2, 5, 9] and w.tolist() == [1.0, 2.0, 0.75]
    assert ix.get("3")[0].size == 0 and (ix.ntotal, ix.nnz) == (3, 5)
    # dropped: zero, negative, and what rounds to zero in float16 (below 2^-25); kept: the smallest subnormal's neighbourhood
    ix.index_data(["4"], [([1, 2, 3, 4, 5], [0.0, -2.0, 1e-9, 6e-8, np.float32(third)])])
    t, w = ix.get("4")
    assert t.tolist() == [4, 5] and U.bits(w).tolist() == [1, int(U.bits(np.array([third], np.float16))[0])]
    # a duplicate whose max is not positive is dropped as a whole; a positive one beats a negative one
    ix.index_data(["5"], [([6, 6, 8, 8], [-1.0, 0.0, -3.0, 0.5])])
    assert ix.get("5")[0].tolist() == [8]
    with pytest.raises(ValueError, match="not a term id"):
        ix.index_data(["6"], [{"aa": 1.0}])
    assert ix.ntotal == 5


def test_refused_calls_keep_nothing():
    ix = cpu_index(16)
    ix.index_data(["1"], [([1], [1.0])])
    good = ([2, 3], [1.0, 2.0])
    for bad, what in ((([16], [1.0]), "term 16"), (([-1], [1.0]), "term -1"), (([2], [np.nan]), "NaN or Inf"), (([2], [np.inf]), "NaN or Inf"),
                      (([2], [1e6]), "overflows float16"), (([2], [65520.0]), "overflows float16"), (([2, 3], [1.0]), "2 terms, 1 weights"),
                      (([2.5], [1.0]), "integers")):
        with pytest.raises(ValueError, match=what):
            ix.index_data(["2", "3"], [good, bad])
    for ids in (["1", "2"], ["2", "2"], ["x", "2"]):
        with pytest.raises(ValueError):
            ix.index_data(ids, [good, good])
    with pytest.raises(ValueError, match="1 ids for 2 passages"):
        ix.index_data(["2"], [good, good])
    assert (ix.ntotal, ix.nnz) == (1, 1)
    ix.index_data(["2"], [([2], [65504.0])])                      # the largest finite float16 is a weight like any other
    assert ix.get("2")[1].tolist() == [65504.0]
    for V in (0, (1 << 24) + 1):
        with pytest.raises(ValueError, match="vocab_size"):
            cpu_index(V)


def test_cpu_index_block_follows_the_rule_and_refuses_what_is_not_finite():
    V = 97
    rng = np.random.default_rng(5)
    block = np.where(rng.random((6, V)) < 0.3, rng.uniform(0.01, 4.0, (6, V)), 0.0).astype(np.float32)
    block[1] = 0.0
    block[2] = rng.uniform(0.5, 1.0, V)
    block[3, 10], block[3, 11], block[3, 12] = 1e-9, -0.5, 3.0
    ix = cpu_index(V)
    ix.index_block([str(i) for i in range(6)], torch.from_numpy(block), skip_terms=(0, 12, None))
    counts, terms, wbits = U.torch_compact(block, skip=(0, 12))
    assert np.array_equal(np.diff(ix.row_off), counts) and np.array_equal(ix.terms, terms) and np.array_equal(U.bits(ix.weights), wbits)
    assert ix.get("1")[0].size == 0 and ix.get("2")[0].tolist() == [t for t in range(V) if t not in (0, 12)]
    assert 10 not in ix.get("3")[0] and 11 not in ix.get("3")[0] and 12 not in ix.get("3")[0]
    for bad in (np.nan, np.inf, -np.inf, 1e6):
        b = block.copy(); b[4, 50] = bad
        with pytest.raises(ValueError, match="finite"):
            cpu_index(V).index_block([str(i) for i in range(6)], torch.from_numpy(b))
    with pytest.raises(ValueError, match=r"\[B, 97\]"):
        cpu_index(V).index_block(["1"], torch.zeros(1, 96))
    with pytest.raises(ValueError, match="already stored"):
        ix.index_block([str(i) for i in range(6)], torch.from_numpy(block))
    assert ix.ntotal == 6


# ---- files ----
def test_serialize_round_trip_keeps_every_bit_and_each_corruption_is_named(tmp_path):
    from kirag_amd.retriever.sparse_index import INDEX_FILE, MAGIC
    ix = cpu_index(1031)
    ix.index_data(["5", "-9", "123456789012", "7"], [([3, 900, 1030], [6e-8, 65504.0, 0.333]), ([], []), {"0": 1.0, "17": 2.5}, ([17], [0.1])])
    ix.serialize(str(tmp_path))
    path = os.path.join(str(tmp_path), INDEX_FILE)
    raw = open(path, "rb").read()
    N, nnz = 4, 6
    assert raw[:8] == MAGIC and len(raw) == 64 + 8 * N + 8 * (N + 1) + 4 * nnz + 2 * nnz
    assert np.frombuffer(raw[8:40], "<i8").tolist() == [1031, R_(), N, nnz] and raw[40:64] == bytes(24)
    t = cpu_index(1031)
    t.deserialize_from(str(tmp_path))
    assert (t.ntotal, t.nnz) == (N, nnz) and t.ids.tolist() == ix.ids.tolist() and t.row_off.tolist() == ix.row_off.tolist()
    assert np.array_equal(t.terms, ix.terms) and np.array_equal(U.bits(t.weights), U.bits(ix.weights))
    assert t.get("-9")[0].size == 0 and U.bits(t.get("5")[1]).tolist() == U.bits(ix.get("5")[1]).tolist()
    po_a, po_b = t._sync_tail(), ix._sync_tail()                  # loading inverts again: the same postings
    assert po_a.tolist() == po_b.tolist() and torch.equal(t._post[:po_a[-1]], ix._post[:po_b[-1]]) and torch.equal(t._ptr[:1], ix._ptr[:1])
    t.index_data(["77"], [([1], [1.0])])                          # a loaded index goes on growing
    assert t.ntotal == 5
    t.serialize(str(tmp_path)); t.deserialize_from(str(tmp_path))
    assert t.ntotal == 5 and t.get("77")[0].tolist() == [1]

    def load(data, V=1031):
        open(path, "wb").write(data)
        cpu_index(V).deserialize_from(str(tmp_path))

    def patched(offset, value, fmt="<q"):
        import struct
        b = bytearray(raw)
        struct.pack_into(fmt, b, offset, value)
        return bytes(b)

    ids_at, off_at = 64, 64 + 8 * N
    terms_at = off_at + 8 * (N + 1)
    w_at = terms_at + 4 * nnz
    for data, what, kw in ((raw[:40], "shorter than its header", {}), (b"KSPARSE9" + raw[8:], "magic", {}), (raw, "V=1031", {"V": 97}),
                           (patched(16, 1000), "R=1000", {}), (patched(24, -1), "N=-1", {}), (raw[:-2], "truncated", {}),
                           (patched(24, 5), "truncated", {}), (patched(off_at, 1), "row_off", {}), (patched(off_at + 8, 9), "row_off", {}),
                           (patched(off_at + 32, 5), "row_off", {}), (patched(ids_at + 8, 5), "an id occurs twice", {}),
                           (patched(terms_at, 1031, "<i"), "outside", {}), (patched(terms_at + 4, 3, "<i"), "do not ascend", {}),
                           (patched(w_at, 0, "<H"), "not finite and > 0", {}), (patched(w_at + 2, 0x7C00, "<H"), "not finite and > 0", {}),
                           (patched(w_at + 2, 0x8400, "<H"), "not finite and > 0", {})):
        with pytest.raises(ValueError, match=what):
            load(data, **kw)
    load(raw)                                                      # and the untouched bytes still load


# ---- no torch scoring path ----
def test_cpu_index_refuses_to_search():
    ix = cpu_index(16)
    ix.index_data(["1"], [([1], [1.0])])
    with pytest.raises(RuntimeError, match="GPU"):
        ix.search_knn([([1], [1.0])], 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ix.search_arrays([{"1": 1.0}], 1)


# ---- the model surface on stubs ----
class _StubM3:
    """forward_m3 with a sparse weight per token that depends on the token id alone"""
    def forward_m3(self, ids, mask, return_sparse=True, return_colbert=True):
        self.calls = getattr(self, "calls", 0) + 1
        self.asked_sparse = return_sparse
        B, S = ids.shape
        dense = torch.zeros(B, 4); dense[:, 0] = 1.0
        ang = ids.float()[..., None] * 0.1 + torch.arange(32) * 0.01
        sparse = (0.25 + (ids % 7).float() * 0.125) * mask if return_sparse else None
        return dense, sparse, (torch.cos(ang) * mask[..., None]).float()


class _StubIndexer:
    def __init__(self, refuse=None):
        from types import SimpleNamespace
        self.refuse, self.ids, self.index = refuse, [], SimpleNamespace(ntotal=0)

    def index_data(self, ids, embeddings):
        if self.refuse in ids:
            raise RuntimeError("the index refuses this batch")
        self.ids += [int(i) for i in ids]
        self.index.ntotal = len(self.ids)


def test_m3_index_passages_keeps_three_containers_in_step():
    import xlmr_util as X
    from kirag_amd.retriever.late import MultiVectorStore
    from kirag_amd.retriever.m3 import BGEM3Model
    words = X.toy_words()
    tok = X.toy_tokenizer()
    passages = [" ".join(words[k:k + 1 + k % 3]) for k in range(7)]
    ids = [str(40 + k) for k in range(7)]
    m3 = BGEM3Model(_StubM3(), tokenizer=tok, device="cpu")
    V = len(tok)
    # an id the sparse index holds already: refused before the first forward, nothing indexed anywhere
    ix, st, sp = _StubIndexer(), MultiVectorStore(32, device="cpu"), cpu_index(V)
    sp.index_data([ids[5]], [([1], [1.0])])
    with pytest.raises(ValueError, match="already stored"):
        m3.index_passages(ids, passages, ix, st, batch_size=3, sparse_index=sp)
    assert getattr(m3.model, "calls", 0) == 0 and st.ntotal == 0 and sp.ntotal == 1 and ix.ids == []
    # the index refuses the second batch after store and sparse index took it: both give it back, the first batch stays in all three
    ix, st, sp = _StubIndexer(refuse=ids[4]), MultiVectorStore(32, device="cpu"), cpu_index(V)
    with pytest.raises(RuntimeError, match="refuses this batch"):
        m3.index_passages(ids, passages, ix, st, batch_size=3, sparse_index=sp)
    assert ix.ids == [40, 41, 42] == st.ids.tolist() == sp.ids.tolist() and sp.ntotal == st.ntotal == ix.index.ntotal == 3
    assert m3.model.asked_sparse is True
    ix.refuse = None
    m3.index_passages(ids[3:], passages[3:], ix, st, batch_size=3, sparse_index=sp)
    assert ix.ids == st.ids.tolist() == sp.ids.tolist() == [40 + k for k in range(7)]
    # what is stored is encode's lexical_weights, rounded to float16
    lex = m3.encode(passages, return_dense=False, return_sparse=True)["lexical_weights"]
    for i, d in zip(ids, lex):
        t, w = sp.get(i)
        assert t.tolist() == sorted(int(k) for k in d) and w.tolist() == [float(np.float16(d[str(k)])) for k in t.tolist()] and len(t) > 0
    # the sparse index refuses a batch (a weight that overflows float16): the store gives it back, the index never sees it
    class _Big(_StubM3):
        def forward_m3(self, ids, mask, return_sparse=True, return_colbert=True):
            d, s, c = super().forward_m3(ids, mask, return_sparse, return_colbert)
            return d, (s * 1e6 if self.calls == 2 else s), c
    big = BGEM3Model(_Big(), tokenizer=tok, device="cpu")
    ix, st, sp = _StubIndexer(), MultiVectorStore(32, device="cpu"), cpu_index(V)
    with pytest.raises(ValueError, match="overflows float16"):
        big.index_passages(ids, passages, ix, st, batch_size=3, sparse_index=sp)
    assert ix.ids == [40, 41, 42] == st.ids.tolist() == sp.ids.tolist()
    # without a sparse index the forward is not asked for the sparse block: today's behaviour
    m = BGEM3Model(_StubM3(), tokenizer=tok, device="cpu")
    m.index_passages(ids, passages, _StubIndexer(), MultiVectorStore(32, device="cpu"), batch_size=7)
    assert m.model.asked_sparse is False


def test_splade_index_passages_checks_ids_first_and_skips_the_pad_id():
    import reranker_util as RU
    from kirag_amd.retriever.splade import SpladeModel
    tok = RU.bert_pair_tokenizer()
    V = tok.vocab_size

    class _StubSplade:
        calls = 0
        def forward_splade(self, ids, mask, token_type_ids=None):
            self.calls += 1
            out = torch.zeros(ids.shape[0], V)
            out.scatter_(1, ids, 1.0 + (ids % 5).float() * 0.25)          # a weight under every token id of the row, the pad id's included
            return out

    texts = RU.passages(5, seed=1)
    model = SpladeModel(_StubSplade(), tokenizer=tok, device="cpu")
    sp = cpu_index(V)
    with pytest.raises(ValueError):
        model.index_passages(["1", "2", "3", "4", "1"], texts, sp, batch_size=2)
    with pytest.raises(ValueError, match="4 ids for 5 passages"):
        model.index_passages(["1", "2", "3", "4"], texts, sp, batch_size=2)
    assert model.model.calls == 0 and sp.ntotal == 0
    model.index_passages([str(i) for i in range(5)], texts, sp, batch_size=2)
    assert model.model.calls == 3 and sp.ntotal == 5
    enc = tok(texts, padding=True, truncation=True, return_tensors="np")
    assert (enc["attention_mask"] == 0).any()                             # padding exists, so the pad id had a weight to skip
    for i in range(5):
        real = enc["input_ids"][i][enc["attention_mask"][i] == 1]          # the other rows of a batch of two never pad more than this
        assert tok.pad_token_id not in sp.get(i)[0] and set(sp.get(i)[0].tolist()) == set(int(t) for t in real if t != tok.pad_token_id)
    with pytest.raises(RuntimeError, match="GPU"):
        model.retrieve(texts[:1], sp, top_k=3)


# ---- the reference has teeth ----
@pytest.fixture(scope="module")
def random_case():
    c = U.random_corpus(1031, 3000, seed=11)
    return c, [U.random_query(1031, m, seed=20 + m) for m in (33, 200)]


@pytest.mark.parametrize("broken", U.MUTATIONS)
def test_every_mutation_changes_some_scores_bits(random_case, broken):
    c, queries = random_case
    changed = 0
    for t, w in queries:
        changed += int((U.bits(U.ref_scores(c, t, w)) != U.bits(U.ref_scores(c, t, w, broken))).sum())
    assert changed > 0, broken


def test_the_float32_reference_lies_within_the_a_priori_bound_of_the_float64_sum(random_case):
    c, queries = random_case
    for t, w in queries:
        s64, bound = U.scores64(c, t, w)
        s32 = U.ref_scores(c, t, w)
        assert (s64 > 0).sum() > 100 and (np.abs(s32.astype(np.float64) - s64) <= bound).all()
        assert np.array_equal(s32 > 0, s64 > 0)
        assert s32[s32 > 0].min() >= 2.0 ** -126                    # nothing subnormal: float16 weights >= 2^-10 times query weights >= 0.1


def test_ref_search_orders_ties_by_row_and_pads_with_minus_one():
    c = U.Corpus(8, [0, 1, 2, 3, 3, 4], [2, 2, 2, 2], np.array([1.0, 2.0, 1.0, 2.0], np.float32))
    s, r = U.ref_search(c, [2], [0.5], 6)
    assert r.tolist() == [1, 4, 0, 2, -1, -1] and s.tolist() == [1.0, 1.0, 0.5, 0.5, 0.0, 0.0] and not np.signbit(s[4:]).any()
