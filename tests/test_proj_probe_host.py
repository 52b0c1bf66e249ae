"""The inputs of the projection probe have teeth (tests/proj_probe_util.py) — checked on the float64 reference alone, no GPU: on the SAME cases
tests/test_gpu_proj_probe.py launches, every listed mutant of the kernels changes the exact set's expected bits and moves the diffuse set's reference by at least
10 x error_bound somewhere in the block it acts on, in every case it applies to; tile_pair_row round-trips; the exact set's partial sums are integers <= 256 at
K = 9728 in every summation order; check_case mirrors the probe's argument checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_probe_util as U  # noqa: E402
from nomic_util import interleave_gate_up, split_gate_up  # noqa: E402

MOVE = 10.0          # x error_bound, of the wider type's bound (bf16) as of the narrower


def _changed_exact(ref, alt):
    """the exact set: some expected bit pattern changes (values that are exact in both types differ as numbers <=> their bits differ, -0 == +0 aside)"""
    return any(not np.array_equal(np.nan_to_num(ref[k], nan=-1.0), np.nan_to_num(alt[k], nan=-1.0)) for k in ref)


def _moved_diffuse(ref, alt, bound):
    best = 0.0
    for k in ref:
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(alt[k] - ref[k])[:bound[k].shape[0]] / bound[k]
        r = r[~np.isnan(r)]      # (0 / 0: an element the mutant leaves alone where the bound is 0, as in the guard row; x / 0 = inf counts)
        best = max(best, float(r.max()) if r.size else 0.0)
    return best


@pytest.mark.parametrize("epi", range(10), ids=U.EPI_NAMES)
def test_every_mutant_is_seen_in_every_case(epi):
    seen = {m: 0 for m in U.MUTANTS}
    for data in ("exact", "diffuse"):
        for name, c in U.cases_of(epi, data):
            assert U.check_case(c, loop=128) is None, (name, U.check_case(c, loop=128))
            # the exact set's linear epilogues are compared as bit patterns; everything else — the diffuse set, and GELU / the gated epilogues on the exact
            # set — within the bound, so there a mutant has to move the reference by 10 bounds to be seen for certain
            bits = data == "exact" and epi in U.EXACT_BITS
            ref, bound = U.reference(c, dtype="bf16")
            for m in U.MUTANTS:
                if not U.applies(m, c):
                    continue
                alt = U.reference(c, mut=m)
                seen[m] += 1
                if bits:
                    assert _changed_exact(ref, alt), (U.EPI_NAMES[epi], name, m)
                else:
                    moved = _moved_diffuse(ref, alt, bound)
                    assert moved >= MOVE, (U.EPI_NAMES[epi], name, m, moved)
    c = U.cases_of(epi, "exact")[0][1]
    for m in U.MUTANTS:      # a mutant that belongs to this epilogue ran at least on the walk shape
        if U.applies(m, c):
            assert seen[m] >= 2, m


def test_every_mutant_applies_somewhere():
    hit = set()
    for epi in range(10):
        for name, c in U.cases_of(epi, "exact"):
            hit |= {m for m in U.MUTANTS if U.applies(m, c)}
    assert hit == set(U.MUTANTS), set(U.MUTANTS) - hit


def test_tile_pair_row_round_trips():
    r = np.arange(4096)
    for mode in (U.ROWS_HEAD64, U.ROWS_GATE, U.ROWS_UP):
        p = U.tile_pair_row(r, mode)
        assert np.array_equal(U.tile_pair_row_inv(p, mode), r) and len(set(p.tolist())) == len(r)
    # gate and up together fill [0, 2 FF) and agree with nomic_util's interleave
    g, u = U.tile_pair_row(r, U.ROWS_GATE), U.tile_pair_row(r, U.ROWS_UP)
    assert sorted(g.tolist() + u.tolist()) == list(range(2 * len(r)))
    gate, up = np.arange(64)[:, None] * np.ones((1, 3)), 100 + np.arange(64)[:, None] * np.ones((1, 3))
    w = interleave_gate_up(gate, up)
    assert np.array_equal(w[U.tile_pair_row(np.arange(64), U.ROWS_GATE)], gate) and np.array_equal(w[U.tile_pair_row(np.arange(64), U.ROWS_UP)], up)
    assert all(np.array_equal(a, b) for a, b in zip(split_gate_up(w), (gate, up)))
    # the 64-wide head: feature j sits 16 columns before its rotary partner j + 32 inside one 32-column tile
    j = np.arange(32)
    a, b = U.tile_pair_row(j, U.ROWS_HEAD64), U.tile_pair_row(j + 32, U.ROWS_HEAD64)
    assert np.array_equal(b, a + 16) and np.array_equal(a >> 5, b >> 5) and np.array_equal(a & 15, j & 15)
    # packed_index is the permutation the probe is fed: every checkpoint row once
    for epi in (U.EPI_QKV_ROT, U.EPI_SWIGLU, U.EPI_DENSE):
        c = U.make_case(epi, "exact", 33, 320, 64, **U.shape_kwargs(epi, 320))
        assert sorted(U.packed_index(c).tolist()) == list(range(320))


@pytest.mark.parametrize("epi", [U.EPI_DENSE, U.EPI_QKV_ROTB, U.EPI_GEGLU, U.EPI_SPLADE], ids=lambda e: U.EPI_NAMES[e])
def test_exact_set_is_exact_at_the_longest_K(epi):
    """K = 9728: one +-1 per (row, K-tile) against +-1 weights: every product is +-1 or 0, any partial sum in any order is an integer of magnitude <= nk = 152,
    with the bias <= 160 <= 256; all inputs and expected outputs survive both 16-bit types"""
    F = 384 if epi == U.EPI_QKV else U.LONG_F
    c = U.make_case(epi, "exact", U.LONG_T, F, 9728, **U.shape_kwargs(epi, F))
    assert c.nk == 152
    assert set(np.unique(c.W)) == {-1.0, 1.0} and set(np.unique(c.X[:c.T])) == {-1.0, 0.0, 1.0}
    assert (np.abs(c.X[:c.T]).reshape(c.T, c.nk, 64).sum(2) == 1).all()          # exactly one per K-tile
    acc, absacc = U.accumulators(c)
    assert (absacc[:c.T] == c.nk).all() and np.array_equal(acc, np.round(acc))    # sum |x w| = nk bounds every partial sum of every order
    assert np.abs(c.bias[np.isfinite(c.bias) & (np.abs(c.bias) < 100)]).max() <= 8
    for dtype in ("f16", "bf16"):
        U.probe_arrays(c, dtype)                                                  # to_bits raises on a value that is not exact
        if epi in U.EXACT_BITS:
            bits = U.expected_bits(c, dtype)
            for k, v in bits.items():
                if k != "smax":
                    assert np.abs(U.from_bits(v, dtype)).max() <= 256
    # every K-tile moves every element by exactly +-1
    for kt in (0, 75, 151):
        part = c.X[:c.T, 64 * kt:64 * kt + 64] @ c.W[:, 64 * kt:64 * kt + 64].T
        assert (np.abs(part) == 1).all()


def test_diffuse_set_is_exact_in_both_types_and_at_scale():
    for K in (64, 192, 9728):
        c = U.make_case(U.EPI_GELU, "diffuse", 300, 256, K)
        for dtype in ("f16", "bf16"):
            U.probe_arrays(c, dtype)
        acc, _ = U.accumulators(c)
        # sigma sqrt(K) = 1.3 on the plain channels; the outlier channel of every K-tile multiplies the output's deviation by sqrt(1 + 1023 / 64) = 4.1
        assert 1.0 < acc[:c.T].std() / np.sqrt(1 + (U.OUTLIER ** 2 - 1) / 64) < 1.6 and 4.0 < acc[:c.T].std() < 6.5
    cos, sin = U.rope_tables(U.MAX_POS, 64, "diffuse")
    assert cos.dtype == np.float32 and np.abs(cos.astype(np.float64) ** 2 + sin.astype(np.float64) ** 2 - 1).max() < 1e-6
    cos, sin = U.rope_tables(U.MAX_POS, 64, "exact")
    assert set(zip(cos.ravel().tolist(), sin.ravel().tolist())) == {(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)}
    assert len({tuple(r) for r in cos[:8].tolist()}) > 1 and len(set(cos[5].tolist())) > 1      # varies with the position and with the pair index


@pytest.mark.parametrize("K", [2560, 9728])
def test_diffuse_accumulators_round_in_fp32(K):
    """the diffuse operands carry floating significands: fp32 sums of their (exact) products round, and the order of the sum shows in the bits — so the GPU
    test's bit identity across loops, grids and knobs holds the loops to ONE accumulation order, and the gamma_K term of the bound is exercised"""
    c = U.make_case(U.EPI_DENSE, "diffuse", U.LONG_T, U.LONG_F, K)
    prod = (c.X[:8, None, :] * c.W[None, :64, :])
    assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)              # every product is exact in fp32
    p32 = prod.astype(np.float32)
    fwd, bwd = np.zeros(p32.shape[:2], np.float32), np.zeros(p32.shape[:2], np.float32)
    for k in range(K):
        fwd += p32[:, :, k]
        bwd += p32[:, :, K - 1 - k]
    exact = prod.sum(2)
    assert (fwd != bwd).mean() > 0.5 and (fwd.astype(np.float64) != exact).mean() > 0.5   # most sums round, and differently in the two orders
    _, absacc = U.accumulators(c)
    g = K * 2.0 ** -24 / (1 - K * 2.0 ** -24)
    assert (np.abs(fwd - exact) <= g * absacc[:8, :64]).all()                               # and gamma_K sum |x w| bounds what they lose


def test_error_bound_terms():
    """the exact set carries no accumulation term: a linear epilogue's bound is half an ulp of the output; the diffuse bound at K = 9728 is dominated by
    gamma_K sum |x w|, which is why the diffuse set carries an outlier channel per K-tile"""
    c = U.make_case(U.EPI_DENSE, "exact", 33, 320, 128)
    ref, b = U.reference(c, dtype="bf16")
    assert np.allclose(b["out0"], 2.0 ** -8 * np.abs(ref["out0"]) + 2.0 ** -125)
    c = U.make_case(U.EPI_DENSE, "diffuse", 300, 256, 9728)
    ref, b = U.reference(c, dtype="f16")
    _, absacc = U.accumulators(c)
    g = 9728 * 2.0 ** -24 / (1 - 9728 * 2.0 ** -24)
    assert (b["out0"] >= g * absacc[:c.T]).all() and (b["out0"] <= g * absacc[:c.T] * 1.001 + 2.0 ** -11 * np.abs(ref["out0"]) * 1.001 + 2.0 ** -25).all()


def test_check_case_mirrors_the_probe():
    c = U.make_case(U.EPI_QKV_ROT, "exact", 33, 320, 64, **U.shape_kwargs(U.EPI_QKV_ROT, 320))
    assert U.check_case(c) is None and U.check_case(c, loop=130, blocks=16) is None
    assert U.check_case(c, blocks=12) and U.check_case(c, loop=32, blocks=8) and U.check_case(c, loop=130, nt=1) and U.check_case(c, ant=1) and U.check_case(c, pw=0)
    for field, bad in (("T", 0), ("T", c.capT + 1), ("K", 96), ("F", 352), ("A", 128), ("ldT", c.capT - 8), ("dh", 48), ("capT", 300)):
        d = U.Case()
        d.__dict__.update(c.__dict__)
        setattr(d, field, bad)
        assert U.check_case(d), field
    b = U.make_case(U.EPI_QKV_ROTB, "exact", 33, 320, 64, **U.shape_kwargs(U.EPI_QKV_ROTB, 320))
    assert U.check_case(b, loop=256) and U.check_case(b, loop=128) is None
    s = U.make_case(U.EPI_SPLADE, "exact", 33, 320, 64, V=283)
    assert U.check_case(s) is None and U.check_case(s, nt=1)
    d = U.Case()
    d.__dict__.update(s.__dict__)
    d.V = 321
    assert U.check_case(d)
