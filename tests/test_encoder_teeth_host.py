"""Preconditions of the token-level GPU tests (tests/test_gpu_encoder_tokens.py), on the CPU and on the fp64 oracle alone: a GPU parity test at bar BAR says
something about a step of the forward only if getting that step wrong moves the compared rows by much more than BAR, and if 16-bit operands, done right, stay
well inside it.  Both are asserted here, on the very inputs the GPU tests use (tests/sharp_util.py builds them for both files):

  * a planted key: masking it moves EVERY attended row of its sequence by >= 10 BAR, for every batch of section A;
  * the whole-model mutants (score scale of the other head width, exp2 without the log2(e) fold, heads swapped, the value bias dropped, position = rank,
    holes ignored, token types ignored, CLS row = first attended row): each moves every sequence it can reach by >= 10 BAR and leaves the others alone;
  * the f16-operand emulation (weights, xb, q, k, v, P, ctx, h rounded, fp64 accumulation) stays within BAR / 3 of fp64 on all of those inputs and on the
    shapes of the width sweep.  The margin of 3 is there because the emulation models neither the fp32 accumulation order nor the residual low half;
  * the bars of the other precision modes, recorded in sharp_util.MODE_BARS, are 3 x their emulation's worst error and at most a third of the weakest
    precondition of the same inputs.

Deliberately NOT claimed.  A tanh approximation in place of the erf GELU moves no row of these models by more than 5e-3, and an unbiased LayerNorm variance
(H - 1 in place of H) moves rows by 2e-2 at H = 128: both are below what 16-bit operands resolve per token (BAR = 3e-2), so no token-level test can tell them
from rounding and none pretends to.  The pooled-embedding tests against HF fp32 (1 - cos <= 5e-5) are what bounds them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharp_util as U  # noqa: E402

BAR = U.BAR
DEFAULT = U.MODES[0]
PLANTED_CASES = [(dh, S, layout) for dh in U.DH for S in U.PLANTED for layout in U.LAYOUTS]


def test_forward64_without_hooks_is_the_oracle():
    """forward64 is oracle.encoder_np.bert_forward in fp64 plus hooks: with none of them used it returns the oracle's numbers (holes, left padding, token types)"""
    from oracle import encoder_np as E
    ids, mask, tt = U.generic_case(129, "H")
    want = E.bert_forward(U.generic_model(), ids, mask, 2, dtype=np.float64, token_type_ids=tt)
    assert np.abs(U.generic_ref(129, "H") - want).max() <= 1e-12
    ids, mask, _, _ = U.planted_case(64, "L")
    assert np.abs(U.planted_ref(32, 64, "L") - E.bert_forward(U.planted_model(32), ids, mask, 4, dtype=np.float64)).max() <= 1e-12


def test_planted_batches_are_what_the_table_says():
    """every (n, j) of section A's table in every layout: n attended tokens (n - 2 under H where the sequence fills its row), the planted token exactly once, at
    attended index j; L ends at the last column; under H the attended index differs from the column, and for j = 0 column 0 is masked"""
    for S, pairs in U.PLANTED.items():
        assert sorted({n for n, _ in pairs})[-1] == S
        for n in {n for n, _ in pairs}:
            assert {0, n - 1} <= {j for m, j in pairs if m == n}
        for layout in U.LAYOUTS:
            ids, mask, js, ns = U.planted_case(S, layout)
            for b, (n, j) in enumerate(pairs):
                cols = np.flatnonzero(mask[b])
                assert len(cols) == ns[b] == (n - 2 if layout == "H" and n == S else n)
                assert (ids[b] == U.TOKEN).sum() == 1 and ids[b, cols[js[b]]] == U.TOKEN and (ids[b, cols] >= U.TOKEN).all() and (ids[b][mask[b] == 0] == 0).all()
                assert js[b] == min(j, ns[b] - 1)
                if layout == "R":
                    assert cols[-1] == n - 1
                if layout == "L":
                    assert cols[-1] == S - 1 and cols[0] == S - n
                if layout == "H":
                    assert cols[js[b]] != js[b] and (mask[b, 0] == 0) == (js[b] == 0)


@pytest.mark.parametrize("dh,S,layout", PLANTED_CASES)
def test_the_planted_key_decides_every_row_and_f16_noise_is_small(dh, S, layout):
    """Measured (weakest row under drop_key / f16 emulation): d_h 64: S 32 0.87-1.07 / 2.8e-3, S 64 0.80-0.93 / 3.3e-3, S 128 0.67-0.77 / 3.4e-3, S 300 0.55-0.68 /
    3.6e-3; d_h 32: 0.93-1.00 / 3.0e-3, 0.78-1.00 / 3.6e-3, 0.70-0.79 / 3.2e-3, 0.56-0.63 / 3.8e-3 (c = 12; with c = 8 the weakest row was 0.11)."""
    weakest = U.planted_teeth(dh, S, layout)
    noise = U.planted_noise(dh, S, layout, DEFAULT)
    print(f"[d_h {dh}] S {S} {layout}: weakest row without the planted key {weakest:.3f}, f16 emulation {noise:.2e}")
    assert weakest >= 10 * BAR, (dh, S, layout, weakest)
    assert noise <= BAR / 3, (dh, S, layout, noise)


def test_whole_model_mutants_move_every_sequence_they_can_reach():
    """Generic sharp weights, the four batches of section B.  Measured smallest distance over the affected sequences: scale_other_dh 0.54, scale_ln2 0.40,
    heads_swapped 3.3, no_bv 0.68, pos_rank 0.76, holes_ignored 0.44, type_ignored 1.0, cls_first_attended 0.75; f16 emulation <= 4.3e-3."""
    smallest, reached = {}, {m: 0 for m in U.MUTANTS[1:]}
    for S, layout in U.GENERIC:
        ids, mask, tt = U.generic_case(S, layout)
        assert (mask.sum(1) >= 8).all() and ((tt != 0) & (mask != 0)).any(1).sum() == 2, (S, layout)
        for m, d in U.generic_teeth(S, layout).items():
            a = U.affected(m, mask, tt)
            assert (d[~a] == 0).all(), ("a mutant changed a sequence it cannot reach", m, S, layout, d, a)
            if a.any():
                reached[m] += int(a.sum())
                smallest[m] = min(smallest.get(m, np.inf), float(d[a].min()))
                assert (d[a] >= 10 * BAR).all(), ("precondition", m, S, layout, d, a)
        noise = U.generic_noise(S, layout, DEFAULT)
        print(f"S {S} {layout}: f16 emulation {noise:.2e}")
        assert noise <= BAR / 3, (S, layout, noise)
    print("smallest distance per mutant:", {m: round(v, 2) for m, v in smallest.items()}, "sequences reached:", reached)
    assert all(n >= 2 for n in reached.values()), reached
    # the GPU test of section B compares column 0 under CLS pooling: it must be masked somewhere, and holes and left padding must both occur
    assert any((U.generic_case(S, lay)[1][:, 0] == 0).any() for S, lay in U.GENERIC)


@pytest.mark.parametrize("shape", U.WIDTHS, ids=lambda s: "x".join(map(str, s)))
def test_shape_sweep_emulation_noise(shape):
    """The widths and intermediate sizes of section C at sigma sqrt(H) = 1.57 (no shape needed a smaller scale: sharp_util.WIDTH_SCALE is empty), one layer.
    Measured: 2.5e-3 .. 2.9e-3 on every shape, both S."""
    H, heads, FF = shape
    assert H % 128 == 0 and FF % 128 == 0 and H // heads in (32, 64)
    w = U.width_model(H, heads, FF)
    for S in U.WIDTH_S:
        ids, mask = U.width_case(S)
        assert mask[0].all() and mask[1, 0] == 1 and mask[1, -1] == 0 and mask[2, 0] == 0 and mask[2, -1] == 1
        ref = U.forward64(w, ids, mask, heads)
        noise = U.emulation_error(w, ids, mask, heads, ref, *DEFAULT)
        print(f"{shape} S {S}: f16 emulation {noise:.2e}")
        assert noise <= BAR / 3, (shape, S, noise)


def test_recorded_bars_of_the_other_modes():
    """sharp_util.MODE_BARS against what it records: per case the weakest precondition distance and 3 x the emulation's worst error of each mode (each rounded
    down to two digits, so the recorded value may be up to 10 % below what is computed here, and above it by no more than the 2 % allowed for a BLAS that
    sums in another order), and the rule that decides whether the GPU test
    asserts a mode: its bar is at most a third of the weakest precondition.  Every mode qualifies on every case (bf16: bars 0.065 .. 0.094 against 0.13 ..
    0.26)."""
    for (section, dh, S, layout), (weakest_rec, *bars) in U.MODE_BARS.items():
        if section == "A":
            weakest = U.planted_teeth(dh, S, layout)
            noise = [U.planted_noise(dh, S, layout, m) for m in U.MODES[1:]]
        else:
            weakest = U.generic_weakest(S, layout)
            noise = [U.generic_noise(S, layout, m) for m in U.MODES[1:]]
        assert 0.9 * weakest <= weakest_rec <= weakest * 1.02, (section, dh, S, layout, weakest_rec, weakest)
        for m, bar, e in zip(U.MODES[1:], bars, noise):
            assert 0.9 * 3 * e <= bar <= 3 * e * 1.02, (section, dh, S, layout, m, bar, 3 * e)
            assert bar <= weakest_rec / 3, ("the GPU test would skip this mode", section, dh, S, layout, m, bar, weakest_rec)
    assert {k[:3] for k in U.MODE_BARS if k[0] == "A"} == {("A", dh, S) for dh in U.DH for S in (128, 300)}
    assert {k[2:] for k in U.MODE_BARS if k[0] == "B"} == set(U.GENERIC)


def test_rounding_emulation_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -65504.0, 2.0 ** -25, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.0e38])
    assert np.array_equal(U._round_f16(x[:5]), [1.0, 1.0, 1.0 + 2.0 ** -9, -65504.0, 0.0])
    assert np.array_equal(U._round_bf16(x)[[0, 5, 6]], [1.0, 1.0, 1.0 + 2.0 ** -6]) and np.isfinite(U._round_bf16(x)).all()
    r = np.random.default_rng(0).standard_normal(4096) * 7
    assert np.abs(U._round_f16(r) - r).max() <= 2.0 ** -11 * 32 and np.abs(U._round_bf16(r) - r).max() <= 2.0 ** -8 * 32
    assert np.array_equal(U._round_bf16(U._round_bf16(r)), U._round_bf16(r))
