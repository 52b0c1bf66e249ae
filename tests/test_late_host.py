"""libkirag_late.so and kirag_amd.retriever.late without a GPU: the header, the binding and the built library name the same five functions; the argument
checks of kl_maxsim / kl_gather_rows_f16 refuse by field before a device is asked for; MultiVectorStore on the CPU (ids, counts, masks with holes, refusals,
the file format); and the reference of tests/late_util.py notices every way the kernel could go wrong that the GPU tests rely on it to notice."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import late_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kirag_late.h")
FIVE = {"kl_abi_version", "kl_last_error", "kl_release_scratch", "kl_gather_rows_f16", "kl_maxsim"}


@pytest.fixture(scope="module")
def lib():
    from kirag_amd import _late_lib
    if not os.path.exists(_late_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _late_lib.load()


def last_error(lib):
    return lib.kl_last_error().decode()


# ---- header and ABI ----
def test_header_binding_and_library_agree_on_five_functions(lib):
    from kirag_amd import _late_lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(k[lr]_[a-z0-9_]+)\s*\(", text))
    assert declared == FIVE
    assert set(_late_lib.SIGNATURES) == FIVE
    nm = subprocess.run(["nm", "-D", "--defined-only", _late_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()}
    assert {s for s in exported if s.startswith(("kl_", "kr_"))} == FIVE
    assert re.search(r"#define\s+KL_ABI_VERSION\s+1\b", text) and lib.kl_abi_version() == 1 == _late_lib.ABI_VERSION


def test_error_codes_carry_the_values_of_the_codes_they_mirror():
    from kirag_amd import _late_lib
    late, main = open(HEADER).read(), open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    for name in ("EINVAL", "ENOMEM", "ENODEV", "EHIP", "ERANGE"):
        a = re.search(r"#define\s+KL_%s\s+\((-?\d+)\)" % name, late).group(1)
        b = re.search(r"#define\s+KR_%s\s+\((-?\d+)\)" % name, main).group(1)
        assert a == b and int(a) == getattr(_late_lib, name)


def test_library_links_the_hip_runtime_and_no_project_library():
    from kirag_amd import _late_lib
    out = subprocess.run(["readelf", "-d", _late_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.+?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed)
    assert not [n for n in needed if "kirag" in n]


def test_release_scratch_without_a_workspace_is_a_no_op(lib):
    lib.kl_release_scratch()
    assert lib.kl_abi_version() == 1


# ---- refusals that need no device ----
def call_maxsim(lib, q_off, d_off, pair_q, pair_d, P=128, reduce=1):
    q_off, d_off = np.asarray(q_off, np.int64), np.asarray(d_off, np.int64)
    pq, pd = np.asarray(pair_q, np.int64), np.asarray(pair_d, np.int64)
    # the data pointers are never read: every case below is refused by the checks that run before a device is selected
    return lib.kl_maxsim(None, q_off.ctypes.data, len(q_off) - 1, None, d_off.ctypes.data, len(d_off) - 1, pq.ctypes.data, pd.ctypes.data, len(pq), P, reduce,
                         None, 0, None)


@pytest.mark.parametrize("P", [0, 16, 48, 100, 2080, 4096, -32])
def test_bad_width_is_refused_by_name(lib, P):
    assert call_maxsim(lib, [0, 3], [0, 4], [0], [0], P=P) == -22
    assert "P=%d" % P in last_error(lib)
    src = np.zeros(1, np.int64)
    assert lib.kl_gather_rows_f16(None, src.ctypes.data, 1, P, None, 0, None) == -22
    assert "P=%d" % P in last_error(lib)


@pytest.mark.parametrize("reduce", [-1, 2, 7])
def test_bad_reduce_is_refused_by_name(lib, reduce):
    assert call_maxsim(lib, [0, 3], [0, 4], [0], [0], reduce=reduce) == -22
    assert "reduce=%d" % reduce in last_error(lib)


def test_offsets_must_start_at_zero_and_not_decrease(lib):
    assert call_maxsim(lib, [0, 5, 3], [0, 4], [0], [0]) == -22
    assert "q_off[2]=3" in last_error(lib)
    assert call_maxsim(lib, [0, 5], [0, 4, 9, 8], [0], [0]) == -22
    assert "d_off[3]=8" in last_error(lib)
    assert call_maxsim(lib, [1, 5], [0, 4], [0], [0]) == -22
    assert "q_off[0]=1" in last_error(lib)
    assert call_maxsim(lib, [0, 5], [-2, 4], [0], [0]) == -22
    assert "d_off[0]=-2" in last_error(lib)


def test_a_pair_out_of_range_is_refused_by_name(lib):
    assert call_maxsim(lib, [0, 3, 6], [0, 4], [0, 2], [0, 0]) == -22
    assert "pair_q[1]=2" in last_error(lib)
    assert call_maxsim(lib, [0, 3, 6], [0, 4], [0, 1], [0, 1]) == -22
    assert "pair_d[1]=1" in last_error(lib)
    assert call_maxsim(lib, [0, 3, 6], [0, 4], [-1], [0]) == -22
    assert "pair_q[0]=-1" in last_error(lib)
    assert call_maxsim(lib, [0, 3, 6], [0, 4], [0], [-5]) == -22
    assert "pair_d[0]=-5" in last_error(lib)


def test_a_negative_source_row_is_refused_by_name(lib):
    src = np.array([0, 3, -1], np.int64)
    assert lib.kl_gather_rows_f16(None, src.ctypes.data, 3, 128, None, 0, None) == -22
    assert "src_row[2]=-1" in last_error(lib)


def test_a_misaligned_data_pointer_is_refused_by_name(lib):
    """fake addresses: every case is refused by the checks that run before a device is selected, nothing is read"""
    q_off, d_off, pair = np.array([0, 3], np.int64), np.array([0, 4], np.int64), np.zeros(1, np.int64)
    def call(q, d, out):
        return lib.kl_maxsim(q, q_off.ctypes.data, 1, d, d_off.ctypes.data, 1, pair.ctypes.data, pair.ctypes.data, 1, 128, 1, out, 0, None)
    for args, name in (((0x1002, 0x2000, 0x3000), "q="), ((0x1000, 0x2008, 0x3000), "d="), ((0x1000, 0x2000, 0x3002), "out=")):
        assert call(*args) == -22
        assert name in last_error(lib) and "aligned" in last_error(lib)
    src = np.zeros(1, np.int64)
    for args, name in (((0x1004, 0x2000), "block="), ((0x1000, 0x2008), "out=")):
        assert lib.kl_gather_rows_f16(args[0], src.ctypes.data, 1, 128, args[1], 0, None) == -22
        assert name in last_error(lib) and "aligned" in last_error(lib)


# ---- MultiVectorStore on the CPU ----
def store(dim=32):
    from kirag_amd.retriever.late import MultiVectorStore
    return MultiVectorStore(dim, device="cpu")


def rows(n, P=32, seed=0):
    return np.random.default_rng(seed).standard_normal((n, P)).astype(np.float32)


def test_cpu_store_add_get_counts_and_id_rules():
    s = store()
    assert (s.ntotal, s.ntokens) == (0, 0)
    a, b, c = rows(5, seed=1), rows(0, seed=2), rows(3, seed=3).astype(np.float64)
    s.add(["7", "11"], [a, b])
    s.add([3], [torch.from_numpy(c)])
    assert (s.ntotal, s.ntokens) == (3, 8)
    assert s.vectors.dtype == torch.float16 and s.offsets.tolist() == [0, 5, 5, 8] and s.ids.tolist() == [7, 11, 3]
    got = s.get("7")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float16).astype(np.float32))
    assert s.get(11).shape == (0, 32)
    assert np.array_equal(s.get("3"), torch.from_numpy(c).to(torch.float16).float().numpy())
    with pytest.raises(KeyError, match="12"):
        s.get("12")
    with pytest.raises(ValueError, match="id 7 is already stored"):
        s.add(["7"], [a])
    with pytest.raises(ValueError, match="already stored"):
        s.add(["20", "20"], [a, a])
    with pytest.raises(ValueError):
        s.add(["not a number"], [a])
    with pytest.raises(ValueError, match="2 ids for 1 passages"):
        s.add(["1", "2"], [a])
    with pytest.raises(ValueError, match=r"\[n, 32\]"):
        s.add(["1"], [rows(2, P=64)])
    assert (s.ntotal, s.ntokens) == (3, 8)         # refused calls keep nothing


@pytest.mark.parametrize("dim", [0, 16, 100, 4096])
def test_store_refuses_a_width_the_kernel_does_not_take(dim):
    with pytest.raises(ValueError, match="dim=%d" % dim):
        store(dim)


def test_cpu_store_grows_by_doubling_and_keeps_rows():
    s = store()
    parts = [rows(700, seed=k) for k in range(4)]
    caps = []
    for k, p in enumerate(parts):
        s.add([k], [p])
        caps.append(s.vectors.shape[0])
    assert caps == [1024, 2048, 4096, 4096]
    for k, p in enumerate(parts):
        assert np.array_equal(s.get(k), p.astype(np.float16).astype(np.float32))


def test_cpu_add_block_skip_first_and_masks_with_holes():
    B, S, P = 4, 9, 32
    block = torch.from_numpy(np.random.default_rng(5).standard_normal((B, S, P)).astype(np.float32))
    mask = np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1],        # full
                     [1, 1, 1, 0, 0, 0, 0, 0, 0],        # right padded
                     [0, 1, 0, 1, 1, 0, 1, 0, 0],        # column 0 masked and holes: the first ATTENDED column (1) goes
                     [0, 0, 0, 0, 0, 0, 0, 0, 0]])       # nothing attended
    keep = {True: [[1, 2, 3, 4, 5, 6, 7, 8], [1, 2], [3, 4, 6], []], False: [[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2], [1, 3, 4, 6], []]}
    for skip in (True, False):
        s = store()
        s.add_block(["10", "11", "12", "13"], block, mask, skip_first=skip)
        assert s.ntotal == 4 and s.ntokens == sum(len(k) for k in keep[skip])
        for b in range(B):
            want = block[b, keep[skip][b]].to(torch.float16).float().numpy().reshape(-1, P)
            assert np.array_equal(s.get(10 + b), want), (skip, b)
    with pytest.raises(ValueError, match="attention_mask"):
        store().add_block(["1", "2", "3", "4"], block, mask[:, :5])
    with pytest.raises(ValueError, match="3 ids for 4 passages"):
        store().add_block(["1", "2", "3"], block, mask)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e6, 65520.0])
def test_cpu_store_refuses_rows_that_are_not_finite_in_float16(bad):
    s = store()
    a = rows(4)
    a[2, 7] = bad
    with pytest.raises(ValueError, match="finite"):
        s.add(["1"], [a])
    block = torch.from_numpy(rows(6).reshape(2, 3, 32).copy())
    block[1, 2, 5] = float(bad)
    with pytest.raises(ValueError, match="finite"):
        s.add_block(["1", "2"], block, np.ones((2, 3), np.int64))
    assert (s.ntotal, s.ntokens) == (0, 0)
    block[1, 2, 5] = 65504.0                      # the largest finite float16 is a value like any other
    s.add_block(["1", "2"], block, np.ones((2, 3), np.int64))
    assert s.get("2")[1, 5] == 65504.0


def test_serialize_round_trip_keeps_every_bit(tmp_path):
    from kirag_amd.retriever.late import MAGIC, STORE_FILE
    s = store(64)
    a = rows(6, P=64, seed=8)
    a[0, :4] = [6e-8, -6.1e-5, 65504.0, -0.0]        # a subnormal, the smallest normal's neighbourhood, the largest finite value, a signed zero
    s.add(["5", "-9", "123456789012"], [a, rows(0, P=64), rows(9, P=64, seed=9)])
    s.serialize(str(tmp_path))
    raw = open(os.path.join(str(tmp_path), STORE_FILE), "rb").read()
    assert raw[:8] == MAGIC and len(raw) == 64 + 8 * 3 + 8 * 4 + 2 * 15 * 64
    assert np.frombuffer(raw[8:32], "<i8").tolist() == [64, 3, 15]
    t = store(64)
    t.deserialize_from(str(tmp_path))
    assert (t.ntotal, t.ntokens) == (3, 15) and t.ids.tolist() == s.ids.tolist() and t.offsets.tolist() == s.offsets.tolist()
    assert torch.equal(t.vectors.view(torch.int16), s.vectors[:15].view(torch.int16))
    assert np.array_equal(U.bits(t.get("-9")), U.bits(s.get("-9"))) and np.array_equal(U.bits(t.get("5")), U.bits(s.get("5")))
    t.add(["77"], [rows(2, P=64)])                     # a loaded store goes on growing
    assert t.ntokens == 17
    with pytest.raises(ValueError, match="dim=64"):
        store(32).deserialize_from(str(tmp_path))
    open(os.path.join(str(tmp_path), STORE_FILE), "wb").write(raw[:-2])
    with pytest.raises(ValueError, match="truncated"):
        store(64).deserialize_from(str(tmp_path))


def test_cpu_store_refuses_to_score():
    s = store()
    s.add(["1"], [rows(3)])
    with pytest.raises(RuntimeError, match="GPU"):
        s.maxsim([rows(2)], [["1"]])
    with pytest.raises(RuntimeError, match="GPU"):
        s.rerank(rows(2), ["1"])


# ---- BGEM3Model.index_passages / retrieve on stubs: the two containers stay in step ----
class _StubModel:
    """what BGEM3Model needs of a model: forward_m3 with a fixed vector per token id (P = 32)"""
    def forward_m3(self, ids, mask, return_sparse=True, return_colbert=True):
        self.calls = getattr(self, "calls", 0) + 1
        B, S = ids.shape
        dense = torch.zeros(B, 4); dense[:, 0] = 1.0
        ang = ids.float()[..., None] * 0.1 + torch.arange(32) * 0.01
        return dense, None, (torch.cos(ang) * mask[..., None]).float()


class _StubIndexer:
    """index_data as Indexer's: ids to int64, then the rows; refuses the batch that holds `refuse`"""
    def __init__(self, refuse=None):
        from types import SimpleNamespace
        self.refuse, self.ids, self.index = refuse, [], SimpleNamespace(ntotal=0)

    def index_data(self, ids, embeddings):
        if self.refuse in ids:
            raise RuntimeError("the index refuses this batch")
        self.ids += [int(i) for i in ids]
        self.index.ntotal = len(self.ids)

    def search_knn(self, *a, **k):
        raise AssertionError("an empty index is not searched")


def test_index_passages_keeps_store_and_index_in_step():
    import xlmr_util as X
    from kirag_amd.retriever.m3 import BGEM3Model
    words = X.toy_words()
    passages = [" ".join(words[k:k + 1 + k % 3]) for k in range(7)]
    ids = [str(40 + k) for k in range(7)]
    m3 = BGEM3Model(_StubModel(), tokenizer=X.toy_tokenizer(), device="cpu")
    # an id twice in the call, an id that is no number, an id the store holds: refused before the first forward, nothing indexed
    for bad_ids in (ids[:6] + [ids[0]], ids[:6] + ["x7"]):
        ix, st = _StubIndexer(), store()
        with pytest.raises(ValueError):
            m3.index_passages(bad_ids, passages, ix, st, batch_size=3)
        assert getattr(m3.model, "calls", 0) == 0 and st.ntotal == 0 and ix.ids == []
    ix, st = _StubIndexer(), store()
    st.add([ids[5]], [rows(2)])
    with pytest.raises(ValueError, match="already stored"):
        m3.index_passages(ids, passages, ix, st, batch_size=3)
    assert getattr(m3.model, "calls", 0) == 0 and st.ntotal == 1 and ix.ids == []
    # the index refuses the second batch after the store took it: the store gives it back, the first batch stays in both
    ix, st = _StubIndexer(refuse=ids[4]), store()
    with pytest.raises(RuntimeError, match="refuses this batch"):
        m3.index_passages(ids, passages, ix, st, batch_size=3)
    assert ix.ids == [40, 41, 42] and st.ids.tolist() == [40, 41, 42] and st.ntotal == 3 and len(st.offsets) == 4
    assert st.ntokens == sum(1 + k % 3 + 1 for k in range(3))          # the words and </s>, without <s>
    with pytest.raises(KeyError):
        st.get(ids[3])
    ix.refuse = None
    m3.index_passages(ids[3:], passages[3:], ix, st, batch_size=3)     # the refused ids are free again
    assert ix.ids == st.ids.tolist() == [40 + k for k in range(7)]
    whole = store()
    m3.index_passages(ids, passages, _StubIndexer(), whole, batch_size=7)
    for i in ids:
        assert np.array_equal(st.get(i), whole.get(i))


def test_retrieve_on_an_empty_index_gives_empty_results_without_a_forward():
    import xlmr_util as X
    from kirag_amd.retriever.m3 import BGEM3Model
    m3 = BGEM3Model(_StubModel(), tokenizer=X.toy_tokenizer(), device="cpu")
    for kw in ({}, {"n_candidates": 0}):
        out = m3.retrieve(["aa0 bb1", "cc2"], _StubIndexer(), store(), top_k=5, **kw)
        assert len(out) == 2 and all(ids == [] and s.dtype == np.float32 and s.shape == (0,) for ids, s in out)
    assert m3.retrieve("aa0", _StubIndexer(), store()) == [([], pytest.approx(np.empty(0)))]
    assert getattr(m3.model, "calls", 0) == 0


# ---- the reference has teeth ----
def test_every_mutation_moves_the_reference_by_ten_bars():
    """On the GPU tests' own data (random unit rows; a ragged query so that padded rows exist), each broken reference differs from the whole one by more than
    10 x the score bar on some pair: a kernel that made that mistake could not pass within the bar."""
    P = 128
    q, d = U.f16(U.unit_rows(33, P, 1)), U.f16(U.unit_rows(65, P, 2))
    whole = U.ref_maxsim(q, d, "mean")
    for mut in U.MUTATIONS:
        moved = abs(U.ref_maxsim(q, d, "mean", broken=mut) - whole)
        if mut == "drop_last_doc_token":           # decisive only where the last token decides
            qd, dd = U.decisive_doc(P, 33, 65, 64, 3)
            moved = abs(U.ref_maxsim(qd, dd, "mean", broken=mut) - U.ref_maxsim(qd, dd, "mean"))
        if mut == "admit_padding_row":             # decisive only where every real score is negative
            qd, dd = U.decisive_doc(P, 33, 65, 64, 3, negative=True)
            assert (qd.astype(np.float64) @ dd.astype(np.float64).T).max() < 0
            moved = abs(U.ref_maxsim(qd, dd, "mean", broken=mut) - U.ref_maxsim(qd, dd, "mean"))
        assert moved > 10 * U.SCORE_BAR, (mut, moved)


def test_bounds_are_below_the_score_bar_on_the_shapes_of_the_gpu_tests():
    for P in (128, 256, 1024):
        q, d = U.unit_rows(33, P, 4), U.unit_rows(65, P, 5)
        kb, rb = U.kernel_bound(U.f16(q), U.f16(d), "mean"), U.rounding_bound(q, d)
        assert 0 < kb < 1e-4 and 0 < rb <= 2 * U.U16 * (1 + U.U16) + 1e-5 and kb + rb < U.SCORE_BAR, (P, kb, rb)
        # and the float16 rounding alone stays inside its bound
        assert abs(U.ref_maxsim(U.f16(q), U.f16(d)) - U.ref_maxsim(q, d)) <= rb


def test_exact_operands_are_exact_in_fp32():
    """the bit-exact GPU test rests on this: every partial sum of the integer-exact operands is representable, in any order"""
    for P in U.DIMS:
        q, d = U.exact_rows(70, P, 1), U.exact_rows(200, P, 2)
        s64 = q.astype(np.float64) @ d.astype(np.float64).T
        assert np.abs(q.astype(np.float64)).max() * np.abs(d.astype(np.float64)).max() * P * 70 * 16 < 2 ** 24      # units of 2^-4
        assert np.array_equal(s64 * 16, np.round(s64 * 16))
        assert np.unique(s64.max(axis=1)).size > 5
