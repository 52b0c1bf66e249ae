"""The inputs of the attention probe have teeth (tests/attn_probe_util.py) — checked on the float64 reference alone, no GPU:
every 64-key step a 32-query tile visits is decisive for a row of that tile, at every length of every list the GPU test launches; admitting a decoy flips rows;
reading another KV head flips every sequence; attn_kv_mul divides; every input value is exact in f16 and in bf16."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probe_util as U  # noqa: E402

MOVE = 0.3


def _cases():
    out = []
    for shape in U.ALL_SHAPES:
        for name, (_, lens) in U.edge_lists(shape).items():
            if name == "gqa-long-dma":      # the same sequences as gqa-long-lds
                continue
            out.append((name, tuple(lens), shape, U.MODES))
    for lens, shape, modes in U.LONG_CASES:
        out.append(pytest.param("long", tuple(lens), shape, modes, marks=pytest.mark.slow))      # 10 - 30 s each: float64 scores of up to 8192 x 8192 per head
    return out


@pytest.mark.parametrize("name,lens,shape,modes", _cases(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_needle_coverage(name, lens, shape, modes):
    """Hiding any visited step from any tile moves a row of the tile by >= 0.3: the share of (tile, step) pairs without a decisive query is 0 (pairs in
    which no query of the tile admits a key of the step are no pairs: hiding such a step changes nothing)"""
    heads, kv, dh = shape
    for mode in modes:
        for n, kind in U.list_kinds(lens, mode):
            s = U.make_seq(n, kind, heads, kv, dh, mode, "needles")
            ref, moved = U.reference(s, sens=True)
            np.testing.assert_allclose(ref, U.seq_reference(n, kind, heads, kv, dh, mode, "needles"), rtol=0, atol=1e-12)      # tile by tile == in blocks of tiles
            assert not [k for k in moved if k[0] == "unvisited"], (mode, n, kind)      # the restated visit rule loses no admitted key
            pairs = {k: v for k, v in moved.items() if v >= 0}
            weak = {k: v for k, v in pairs.items() if v < MOVE}
            assert pairs and not weak, (mode, n, kind, len(weak), len(pairs), sorted(weak.items())[:5])


@pytest.mark.parametrize("mode", U.MODES)
def test_step_sensitivity_equals_hiding_the_step(mode):
    """test_needle_coverage reads "the step hidden from the tile" off the reference's own partial sums ((num - num_step) / (den - den_step)); here the step IS
    hidden (reference(hide=)), on single-target and on several-target tiles, and the two agree"""
    for n, kind, shape in ((193, "right", (4, 2, 32)), (289, "holes", (2, 1, 64)), (513, "left", (2, 1, 64)), (1000, "holes", (6, 2, 64)), (2049, "right", (14, 2, 64))):
        if mode == "causal" and kind.startswith("cls"):
            continue
        s = U.make_seq(n, kind, *shape, mode, "needles")
        ref, moved = U.reference(s, sens=True)
        pairs = sorted(k for k, v in moved.items() if v >= 0)
        for tile, kb in [pairs[0], pairs[len(pairs) // 2], pairs[-1]]:      # the last pair: the last tile's last step (2049, 513: a tile of one query with several targets)
            alt = U.reference(s, hide=lambda t: np.arange(kb, min(kb + U.KEY_STEP, s.nk)) if t == tile else np.zeros(0, np.int64))
            rows = slice(U.Q_TILE * tile, U.Q_TILE * tile + U.Q_TILE)
            assert abs(float(np.abs(alt - ref)[rows].max()) - moved[(tile, kb)]) < 1e-9, (mode, n, kind, tile, kb)
            assert not np.abs(alt - ref)[:rows.start].any() and not np.abs(alt - ref)[rows.stop:].any()


@pytest.mark.parametrize("mode", ["window", "causal"])
@pytest.mark.parametrize("shape", [(4, 2, 32), (2, 1, 64)], ids=str)
def test_decoys(mode, shape):
    """Admitting each decoy class — the window one column wider to the right (causal: key i + 1), one wider to the left — moves a row of every sequence
    that carries such a decoy by >= 0.3, and every query with a decoy still has its target"""
    heads, kv, dh = shape
    lens = U.DECODER_LONG + U.SHORT[128]
    seen = {"r": 0, "l": 0}
    for n, kind in U.list_kinds(lens, mode):
        s = U.make_seq(n, kind, heads, kv, dh, mode, "needles")
        ref = U.seq_reference(n, kind, heads, kv, dh, mode, "needles")
        wl, wr = s.win
        for side, pairs, wide in (("r", s.decoy_r, (wl, wr + 1)), ("l", s.decoy_l, (wl + 1, wr))):
            if not pairs:
                continue
            alt = U.reference(s, win=wide)
            rows = np.array([i for i, _ in pairs])
            d = np.abs(alt - ref)[rows].max((1, 2))
            assert (d >= MOVE).all(), (mode, n, kind, side, float(d.min()))
            seen[side] += len(pairs)
    assert seen["r"] > 100 and (mode == "causal" or seen["l"] > 100), seen


@pytest.mark.parametrize("shape", [s for s in U.ALL_SHAPES if s[0] != s[1]], ids=str)
def test_wrong_kv_head(shape):
    """Reading KV head h mod kv_heads, or the neighbouring group's, moves every sequence by >= 0.3"""
    heads, kv, dh = shape
    g = heads // kv
    wrong = [np.arange(heads) % kv, (np.arange(heads) // g + 1) % kv]
    for mode in ("plain", "causal"):
        for n, kind in U.list_kinds(U.SHORT[32] + U.SHORT[128] + U.GQA_LONG, mode):
            s = U.make_seq(n, kind, heads, kv, dh, mode, "needles")
            ref = U.seq_reference(n, kind, heads, kv, dh, mode, "needles")
            for kv_of in wrong:
                if np.array_equal(kv_of, np.arange(heads) // g):
                    continue
                assert np.abs(U.reference(s, kv_of=kv_of) - ref).max() >= MOVE, (mode, n, kind, kv_of)


def test_attn_kv_mul_divides():
    """(h (65536 / g + 1)) >> 16 == h / g for every h < 1024 and g <= 64 (attn_kv_mul / attn_kv_head, encoder_attn.hpp)"""
    h = np.arange(1024, dtype=np.int64)[:, None]
    g = np.arange(1, 65, dtype=np.int64)[None, :]
    assert np.array_equal((h * (65536 // g + 1)) >> 16, h // g)
    assert (h * (65536 // g + 1)).max() < 2 ** 32      # the kernel multiplies in unsigned 32 bits


@pytest.mark.parametrize("data", ["needles", "diffuse"])
def test_inputs_are_exact_in_both_types(data):
    """Every q, k, v value (and the fill) survives the round trip through f16 and through bf16; the bias table is fp32 multiples of 1/8"""
    for heads, kv, dh in ((4, 2, 32), (14, 2, 64)):
        for mode in U.MODES:
            for n, kind in U.list_kinds(U.SHORT[128] + U.GQA_LONG + [1000], mode):
                s = U.make_seq(n, kind, heads, kv, dh, mode, data)
                for dtype in ("f16", "bf16"):
                    for a in (s.q, s.k, s.v):
                        assert np.array_equal(U.from_bits(U.to_bits(a, dtype), dtype), a)
                assert np.abs(s.v).max() <= U.VMAX
    for dtype in ("f16", "bf16"):
        assert np.array_equal(U.from_bits(U.to_bits(np.array(U.FILLS), dtype), dtype), np.array(U.FILLS))
    t = U.bias_table(4)
    assert t.dtype == np.float32 and np.array_equal(t * 8, np.round(t * 8))


def test_diffuse_rows_share_their_mass():
    """The diffuse set: a few dozen keys share a row's mass (the largest weight of a typical row is small), and both kinds of rows exist: the running maximum
    over the 64-key steps keeps rising (past the rescale threshold of 8) and falls after the first step"""
    s = U.make_seq(1000, "right", 4, 2, 32, "plain", "diffuse")
    sc = np.einsum("qd,jd->qj", s.q[:, 0], s.k[:, 0])
    w = np.exp2(sc - sc.max(1, keepdims=True)); w /= w.sum(1, keepdims=True)
    eff = 1.0 / (w ** 2).sum(1)                          # the number of keys that share the mass
    assert np.median(eff) >= 4 and np.median(w.max(1)) < 0.5
    steps = np.pad(sc, ((0, 0), (0, 24)), constant_values=-np.inf).reshape(1000, 16, 64).max(2)
    assert (steps[:, -1] - steps[:, 0] > 8).sum() > 100 and (steps[:, 0] - steps[:, 1:].max(1) > 0).sum() > 100


def test_error_bound_is_what_the_issue_expects():
    """(1) + (2) dominate: about 2^-10 max|v| for f16 and 2^-7 max|v| for bf16; the fp32 terms stay below the 16-bit ones up to 8192 keys"""
    assert 2.0 ** -10 * U.VMAX < U.error_bound("f16", 64) < 1.02 * 2.0 ** -10 * U.VMAX
    assert 2.0 ** -7 * U.VMAX < U.error_bound("bf16", 8192) < 1.15 * 2.0 ** -7 * U.VMAX
    assert U.error_bound("f16", 8192) < 2.1 * 2.0 ** -10 * U.VMAX
