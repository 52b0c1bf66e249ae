"""Host-side pieces of MultiDeviceIndexer (no GPU): the row placement and local -> global maps against a numpy restatement, the mapping of merged lists
with -1 padding, and kr_topk_merge of mapped shard lists against a lexsort by (-score, global row)."""

import numpy as np
import pytest

from kirag_amd.retriever.formats import shard_range
from kirag_amd.retriever.multi_device import RowPlacement, index_devices, parse_index_devices


def restate(world, ops):
    """numpy restatement of the placement rules: -> shard of every global row, in insertion order"""
    owner = []
    plan = None                                       # (start, n)
    for op, n in ops:
        if op == "reserve":
            if n > len(owner):
                plan = (len(owner), n - len(owner))
            continue
        batch = np.empty(n, np.int64)
        i = 0
        while i < n:
            g = len(owner) + i
            if plan is not None and g < plan[0] + plan[1]:
                s = next(s for s in range(world) if g - plan[0] < shard_range(plan[1], s, world)[1])
                batch[i] = s
                i += 1
            else:
                plan = None
                rest = n - i
                sizes = [len(a) for a in np.array_split(np.arange(rest), world)]
                batch[i:] = np.repeat(np.arange(world), sizes)
                i = n
        owner.extend(batch.tolist())
        if plan is not None and len(owner) >= plan[0] + plan[1]:
            plan = None
    return np.array(owner, np.int64)


def apply(world, ops):
    pl = RowPlacement(world)
    for op, n in ops:
        if op == "reserve":
            pl.reserve(n)
        else:
            pl.place(n)
    return pl


def check(world, ops):
    pl = apply(world, ops)
    owner = restate(world, ops)
    assert pl.ntotal == len(owner)
    for s in range(world):
        glob = np.flatnonzero(owner == s)             # shard s's rows in insertion order = its local order
        assert pl.shard_rows[s] == len(glob)
        if len(glob):
            assert np.array_equal(pl.to_global(s, np.arange(len(glob))), glob)
            assert np.all(np.diff(glob) > 0)
    # the runs cover every global row exactly once
    cover = np.zeros(pl.ntotal, np.int64)
    for g0, s, l0, c in pl.global_runs():
        cover[g0:g0 + c] += 1
    assert np.all(cover == 1)
    return pl


SCENARIOS = {
    "reserved": [("reserve", 1000), ("add", 300), ("add", 450), ("add", 250)],
    "unreserved": [("add", 100), ("add", 37), ("add", 1), ("add", 64)],
    "mixed": [("add", 50), ("reserve", 400), ("add", 120), ("add", 300), ("add", 33), ("reserve", 600), ("add", 17), ("add", 5)],
    "small_batches": [("add", 1), ("add", 2), ("add", 5), ("add", 3), ("reserve", 20), ("add", 1), ("add", 2)],
    "reserve_below_ntotal": [("add", 40), ("reserve", 10), ("add", 9)],
}


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_placement_matches_restatement(world, name):
    check(world, SCENARIOS[name])


@pytest.mark.parametrize("world", [1, 3, 8])
def test_placement_random(world):
    rng = np.random.default_rng(world)
    ops = []
    total = 0
    for _ in range(60):
        if rng.random() < 0.2:
            ops.append(("reserve", total + int(rng.integers(0, 300))))
        else:
            m = int(rng.integers(1, 2 * world + 40))
            ops.append(("add", m)); total += m
    check(world, ops)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_reserve_then_fill_is_shard_range(world):
    """a reservation filled in any batch sizes gives every shard its shard_range piece (what deserialize_from loads)"""
    n = 1001
    pl = apply(world, [("reserve", n), ("add", 7), ("add", 500), ("add", n - 507)])
    ld = RowPlacement(world); ld.load(n)
    for s in range(world):
        a, b = shard_range(n, s, world)
        assert pl.runs[s] == ld.runs[s] == ([(a, 0, b - a)] if b > a else [])
    # reserve reports the rows every shard will hold once the plan is filled
    pl2 = RowPlacement(world)
    assert pl2.reserve(n) == [shard_range(n, s, world)[1] - shard_range(n, s, world)[0] for s in range(world)]


def test_batch_smaller_than_world():
    pl = apply(8, [("add", 3), ("add", 2)])
    assert pl.shard_rows == [2, 2, 1, 0, 0, 0, 0, 0]
    assert np.array_equal(pl.to_global(0, np.array([0, 1])), [0, 3])
    assert np.array_equal(pl.to_global(1, np.array([0, 1])), [1, 4])
    assert np.array_equal(pl.to_global(2, np.array([0])), [2])


def test_map_keeps_padding():
    pl = apply(3, [("add", 10), ("add", 7), ("add", 2)])           # several runs per shard
    assert len(pl.runs[0]) == 3
    loc = np.array([[0, 3, 4, -1], [5, 1, -1, -1]], np.int64)
    glob = np.flatnonzero(restate(3, [("add", 10), ("add", 7), ("add", 2)]) == 0)
    want = np.where(loc >= 0, glob[np.maximum(loc, 0)], -1)
    got = pl.to_global(0, loc.copy())
    assert np.array_equal(got, want)
    inplace = loc.copy()
    pl.to_global(0, inplace, out=inplace)
    assert np.array_equal(inplace, want)
    empty = RowPlacement(2)
    assert np.array_equal(empty.to_global(1, np.array([-1, -1])), [-1, -1])


@pytest.mark.parametrize("world", [2, 3, 8])
def test_merge_of_mapped_lists_is_global_lexsort(world):
    """per-shard lists sorted by (score desc, local row asc), mapped to global rows, merged by kr_topk_merge == lexsort over all rows by
    (-score, global row): the bit-equality argument of MultiDeviceIndexer, with many exact ties across shard boundaries"""
    from kirag_amd.parallel import merge_topk
    rng = np.random.default_rng(7 + world)
    ops = [("add", 37), ("reserve", 200), ("add", 90), ("add", 80), ("add", 41)]
    pl = apply(world, ops)
    owner = restate(world, ops)
    n, nq, k = pl.ntotal, 5, 16
    scores = rng.integers(0, 12, size=(nq, n)).astype(np.float32) / 4     # few distinct values: ties everywhere
    want_i = np.stack([np.lexsort((np.arange(n), -scores[q]))[:k] for q in range(nq)])
    want_s = np.take_along_axis(scores, want_i, 1)
    ls = np.full((world, nq, k), -np.inf, np.float32); li = np.full((world, nq, k), -1, np.int64)
    for s in range(world):
        glob = np.flatnonzero(owner == s)
        if not len(glob):
            continue
        for q in range(nq):
            sc = scores[q, glob]
            order = np.lexsort((np.arange(len(glob)), -sc))[:k]        # the shard's own list: local rows
            ls[s, q, :len(order)] = sc[order]; li[s, q, :len(order)] = order
        pl.to_global(s, li[s], out=li[s])
    ms, mi = merge_topk(ls, li, k)
    assert np.array_equal(mi, want_i) and np.array_equal(ms.view(np.uint32), want_s.view(np.uint32))


def test_index_devices_switch(monkeypatch):
    class A:
        pass
    assert parse_index_devices("0,1,2,3") == [0, 1, 2, 3]
    assert parse_index_devices([0, 0]) == [0, 0]
    assert parse_index_devices(" 2 , 3 ") == [2, 3]
    assert parse_index_devices("") is None and parse_index_devices(None) is None
    monkeypatch.delenv("KIRAG_AMD_INDEX_DEVICES", raising=False)
    assert index_devices(A()) is None
    monkeypatch.setenv("KIRAG_AMD_INDEX_DEVICES", "1,0")
    assert index_devices(A()) == [1, 0]
    a = A(); a.index_devices = [0, 0, 0]
    assert index_devices(a) == [0, 0, 0]


def test_cli_flag():
    from kirag_amd.faiss_index_corpus import setup_parser
    assert setup_parser(["--index_devices", "0,1"]).index_devices == "0,1"
    assert setup_parser([]).index_devices is None


def test_exported_next_to_indexer():
    from kirag_amd.retriever import index
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    assert index.MultiDeviceIndexer is MultiDeviceIndexer and issubclass(MultiDeviceIndexer, index.Indexer)
    assert MultiDeviceIndexer.accepts_device_queries is True
