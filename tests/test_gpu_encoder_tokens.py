"""Token-level GPU tests of the plain BERT / XLM-R path: kr_encoder_last_hidden against the fp64 oracle (sharp_util.forward64), element-wise on the attended
rows, at BAR = 3e-2 in the default mode, on weights under which attention decides the output.  The preconditions that give each comparison its teeth (a dropped
key, a wrong score scale, swapped heads, a dropped value-bias fold, position by rank, ignored holes / token types, the wrong CLS row each move the compared
rows by >= 10 BAR; 16-bit operands done right cost <= BAR / 3) are asserted on the same inputs by tests/test_encoder_teeth_host.py.

A  a planted key at every tile edge of both attention kernels, three padding layouts, both pools, both head widths;
B  whole-model parity on generic sharp weights with token types;
C  hidden and intermediate sizes no other test runs (LayerNorm and pooling above 1024 wide, K > 1024 in every projection loop, an odd number of 128-blocks);
D  a row depends on its own tokens only, bit for bit.

Handles are created with KIRAG_AMD_CLS_FULL=1 so that CLS-pooled forwards keep every row.  Under CLS pooling the row of column 0 is compared whether attended
or not (a masked column 0 is the extra query row); every other masked row must be zero.

Measured on MI355X: profiles/encoder_tokens/measurements.txt."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharp_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = U.BAR
COS_BAR = 5e-5              # pooled embeddings
TILES = ("256", "130", "128", "64", "32")
_HANDLES = {}


def _cfg(H, L, heads, FF):
    return SimpleNamespace(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=U.VOCAB,
                           max_position_embeddings=U.MAX_POS, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")


def _new_handle(monkeypatch, cfg, w, mode=(None, None)):
    from kirag_amd.retriever.encoders import HipBertForward
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")          # read at handle creation
    h = HipBertForward(cfg, 0, operand_dtype=mode[0], residual_lo=mode[1])
    monkeypatch.delenv("KIRAG_AMD_CLS_FULL")
    h.load_state(w)
    return h


def _handle(monkeypatch, key, cfg, w, mode=(None, None)):
    """one handle per (model, precision mode) for the whole file"""
    if (key, mode) not in _HANDLES:
        _HANDLES[(key, mode)] = _new_handle(monkeypatch, cfg, w, mode)
        if mode != (None, None):
            assert (_HANDLES[(key, mode)].operand_dtype, _HANDLES[(key, mode)].residual_lo) == mode
        else:
            assert (_HANDLES[(key, mode)].operand_dtype, _HANDLES[(key, mode)].residual_lo) == U.MODES[0]
    return _HANDLES[(key, mode)]


def _tiny(monkeypatch, kind, dh, mode=(None, None)):
    heads = U.DH[dh]
    w = U.planted_model(dh) if kind == "planted" else U.generic_model()
    return _handle(monkeypatch, (kind, dh), _cfg(U.TINY["H"], U.TINY["L"], heads, U.TINY["FF"]), w, mode)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _compared(mask, pool):
    keep = np.asarray(mask) != 0
    if pool == 1:
        keep = keep.copy(); keep[:, 0] = True
    return keep


def _run(h, ids, mask, pool, tt=None):
    """-> (pooled [B,H], last_hidden [B,S,H]) of one forward"""
    out = h.forward_np(ids, mask, pool, token_type_ids=tt)
    return out, h.last_hidden(*ids.shape).numpy()


def _token_error(lh, ref, mask, pool, what):
    """worst |last_hidden - fp64| on the compared rows; the other rows must be zero and everything finite"""
    keep = _compared(mask, pool)
    assert lh.shape == ref.shape and np.isfinite(lh).all(), what
    assert (lh[~keep] == 0).all(), ("a masked row is not zero", what)
    return float(np.abs(lh.astype(np.float64) - ref)[keep].max())


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _planted_parity(h, dh, S, layout, bar, monkeypatch, bits):
    """one planted batch through both pools (and at S = 300 through both attention kernels): every compared row within `bar` of fp64.  With `bits` the two
    kernels and, on right-padded batches, forward_packed must also agree bit for bit.  -> the worst error"""
    ids, mask, _, _ = U.planted_case(S, layout)
    ref = U.planted_ref(dh, S, layout)
    worst = 0.0
    for pool in (0, 1):
        out, lh = _run(h, ids, mask, pool)
        err = _token_error(lh, ref, mask, pool, (dh, S, layout, pool))
        worst = max(worst, err)
        assert err <= bar, (dh, S, layout, pool, err, bar)
        if S > 128:
            monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")          # read per forward: the register-staged kernel with its 128-key staging chunks
            out2, lh2 = _run(h, ids, mask, pool)
            monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
            err2 = _token_error(lh2, ref, mask, pool, (dh, S, layout, pool, "lds"))
            worst = max(worst, err2)
            assert err2 <= bar, (dh, S, layout, pool, "lds", err2, bar)
            if bits:
                assert _same(lh, lh2) and _same(out, out2), ("the two attention kernels differ", dh, S, layout, pool)
        if bits and layout == "R":
            rag, lens = _rag(ids, mask)
            packed = h.forward_packed(rag, lens, S, pool).cpu().numpy()
            assert _same(packed, out), ("forward_packed differs", dh, S, pool)
            assert _same(h.last_hidden(*ids.shape).numpy(), lh), ("forward_packed differs", dh, S, pool)
    return worst


@pytest.mark.parametrize("S", sorted(U.PLANTED))
@pytest.mark.parametrize("dh", sorted(U.DH, reverse=True))
def test_a_planted_key_at_every_tile_edge(dh, S, monkeypatch):
    """Section A.  Layer 0's query bias makes every query attend mostly to the key that holds token 4; sequences of n attended tokens with that key at attended
    index j, for (n, j) at every edge of the 32-row q-tiles, the 64-key steps and the 128-key staging chunks (sharp_util.PLANTED), right-padded, left-padded
    and with holes ahead of the planted column, both pools.  Losing that key, at any of those places, moves every row of the sequence by >= 0.55
    (test_encoder_teeth_host.py) against the bar of 3e-2.
    Kernel selected, mean pooling: S 32 k_attn_lds with 4 heads per block, S 64 2 heads, S 128 1 head, S 300 k_attn_dma and again k_attn_lds through
    KIRAG_AMD_ATTN_LDS=1, same bits.  CLS pooling adds the extra query row of a masked column 0, which is one more q-tile at S = 32, 64 and 128: S 32 then runs the
    2-heads-per-block variant, S 64 the 1-head variant and S 128 k_attn_dma.  On right-padded batches forward_packed gives the same bits.
    Measured on MI355X, worst |last_hidden - fp64| over layouts and pools (f16 emulation beside it): d_h 64: S 32 3.3e-3 (2.8e-3), S 64 3.9e-3 (3.3e-3),
    S 128 3.5e-3 (3.4e-3), S 300 3.9e-3 (3.6e-3); d_h 32: 3.2e-3 (3.0e-3), 3.9e-3 (3.6e-3), 4.0e-3 (3.2e-3), 3.9e-3 (3.8e-3)."""
    h = _tiny(monkeypatch, "planted", dh)
    worst = 0.0
    for layout in U.LAYOUTS:
        err = _planted_parity(h, dh, S, layout, BAR, monkeypatch, bits=True)
        print(f"[A d_h {dh} f16 lo=1] S {S} {layout}: worst |last_hidden - fp64| {err:.2e}")
        worst = max(worst, err)
    print(f"[A d_h {dh} f16 lo=1] S {S}: worst over layouts and pools {worst:.2e} (bar {BAR})")


def _generic_parity(h, S, layout, bar):
    ids, mask, tt = U.generic_case(S, layout)
    ref = U.generic_ref(S, layout)
    worst = 0.0
    for pool in (0, 1):
        out, lh = _run(h, ids, mask, pool, tt)
        err = _token_error(lh, ref, mask, pool, (S, layout, pool))
        worst = max(worst, err)
        assert err <= bar, (S, layout, pool, err, bar)
        cos = float((1 - (out * U.pooled64(ref, mask, pool)).sum(1) / np.linalg.norm(out, axis=1)).max())
        assert cos <= COS_BAR, (S, layout, pool, cos)
    return worst


def test_whole_model_parity_on_generic_sharp_weights(monkeypatch):
    """Section B.  H 128, 2 heads, 2 layers, no plant; S 33 right-padded, 65 left-padded, 129 with holes (column 0 masked in one row), 200 right-padded, B = 4,
    token types on half the rows through forward_np(..., token_type_ids=), both pools.  Each of scale_other_dh, scale_ln2, heads_swapped, no_bv, pos_rank,
    holes_ignored, type_ignored and cls_first_attended moves every sequence it can reach by >= 0.40 on these inputs (test_encoder_teeth_host.py).
    Measured on MI355X (f16 emulation beside it): S 33 4.3e-3 (3.1e-3), S 65 4.4e-3 (4.2e-3), S 129 4.4e-3 (2.8e-3), S 200 4.2e-3 (3.0e-3)."""
    h = _tiny(monkeypatch, "generic", 64)
    for S, layout in U.GENERIC:
        err = _generic_parity(h, S, layout, BAR)
        print(f"[B f16 lo=1] S {S} {layout}: worst |last_hidden - fp64| {err:.2e} (bar {BAR})")


def _mode_bar(section, dh, S, layout, mode):
    """the bar of a non-default mode on one case, or a skip where the case cannot tell that mode's rounding from a mistake"""
    weakest, *bars = U.MODE_BARS[(section, dh, S, layout)]
    bar = bars[U.MODES[1:].index(mode)]
    if bar > weakest / 3:
        pytest.skip(f"{mode}: bar {bar} = 3 x the emulation's error exceeds a third of the weakest precondition distance {weakest} on {section} d_h {dh} S {S} {layout}")
    return bar


@pytest.mark.parametrize("dh", sorted(U.DH, reverse=True))
@pytest.mark.parametrize("mode", U.MODES[1:], ids=lambda m: f"{m[0]}-lo{int(m[1])}")
def test_a_planted_key_in_the_other_precision_modes(mode, dh, monkeypatch):
    """Section A at S = 128 and 300 with f16 operands without the residual low half, and bf16 operands with and without it.  Bar per case: 3 x the worst error
    of the matching emulation on the same inputs (sharp_util.MODE_BARS, asserted by the host file: about 0.010 for f16 without the low half, 0.065 .. 0.077
    for bf16), asserted because it is at most a third of the weakest precondition distance (0.55) everywhere.
    Measured on MI355X: f16 without the low half 3.3e-3 .. 4.5e-3, bf16 with it 2.3e-2 .. 3.1e-2, bf16 without it 2.4e-2 .. 3.1e-2."""
    h = _tiny(monkeypatch, "planted", dh, mode)
    for S in (128, 300):
        for layout in U.LAYOUTS:
            bar = _mode_bar("A", dh, S, layout, mode)
            err = _planted_parity(h, dh, S, layout, bar, monkeypatch, bits=False)
            print(f"[A d_h {dh} {mode[0]} lo={int(mode[1])}] S {S} {layout}: worst |last_hidden - fp64| {err:.2e} (bar {bar})")


@pytest.mark.parametrize("mode", U.MODES[1:], ids=lambda m: f"{m[0]}-lo{int(m[1])}")
def test_whole_model_parity_in_the_other_precision_modes(mode, monkeypatch):
    """Section B in the three other modes, bars as above (0.0095 .. 0.011 for f16 without the low half, 0.071 .. 0.094 for bf16; weakest precondition 0.39).
    Measured on MI355X: f16 without the low half 3.5e-3 .. 4.0e-3, bf16 with it 2.5e-2 .. 2.8e-2, bf16 without it 2.8e-2 .. 3.2e-2."""
    h = _tiny(monkeypatch, "generic", 64, mode)
    for S, layout in U.GENERIC:
        bar = _mode_bar("B", 64, S, layout, mode)
        ids, mask, tt = U.generic_case(S, layout)
        ref = U.generic_ref(S, layout)
        for pool in (0, 1):
            _, lh = _run(h, ids, mask, pool, tt)
            err = _token_error(lh, ref, mask, pool, (S, layout, pool))
            print(f"[B {mode[0]} lo={int(mode[1])}] S {S} {layout} pool {pool}: worst |last_hidden - fp64| {err:.2e} (bar {bar})")
            assert err <= bar, (mode, S, layout, pool, err, bar)


@pytest.mark.parametrize("shape", U.WIDTHS, ids=lambda s: "x".join(map(str, s)))
def test_untested_widths_and_intermediate_sizes(shape, monkeypatch):
    """Section C.  (H, heads, FF) that kr_encoder_create admits and no other test runs: 128 with FF 128 (one 128-deep K block in FF2, half a 256-wide feature
    tile in FF1), 640 / 1152 and 896 / 896 (odd multiples of 128), 1280 / 1408, 1280 / 1280 and 2048 / 2176 (k_ln16<4,7>, k_pool<8>, K > 1024 in every
    projection loop).  One layer, B = 3 (full, right-padded, left-padded), S 40 and 200: token parity at 3e-2 with the launcher's own projection path, then
    KIRAG_AMD_PROJ_TILE 256 / 130 / 128 / 64 / 32 each bit-identical to it (last_hidden and both pooled outputs), and the pooled outputs within 1 - cos <= 5e-5.
    Measured on MI355X, worst |last_hidden - fp64| / worst 1 - cos (f16 emulation 2.5e-3 .. 2.9e-3): 128 / 128 3.3e-3 / 2.7e-7, 640 / 1152 3.1e-3 / 2.1e-7,
    896 / 896 3.0e-3 / 2.0e-7, 1280 / 1408 3.0e-3 / 2.1e-7, 1280 / 1280 3.0e-3 / 2.4e-7, 2048 / 2176 3.3e-3 / 2.3e-7."""
    H, heads, FF = shape
    h = _new_handle(monkeypatch, _cfg(H, 1, heads, FF), U.width_model(H, heads, FF))
    worst, worst_cos = 0.0, 0.0
    for S in U.WIDTH_S:
        ids, mask = U.width_case(S)
        ref = U.forward64(U.width_model(H, heads, FF), ids, mask, heads)
        own = {}
        for pool in (0, 1):
            out, lh = _run(h, ids, mask, pool)
            err = _token_error(lh, ref, mask, pool, (shape, S, pool))
            cos = float((1 - (out * U.pooled64(ref, mask, pool)).sum(1) / np.linalg.norm(out, axis=1)).max())
            worst, worst_cos = max(worst, err), max(worst_cos, cos)
            assert err <= BAR, (shape, S, pool, err)
            assert cos <= COS_BAR, (shape, S, pool, cos)
            own[pool] = (out, lh)
        for tile in TILES:
            monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", tile)      # read per forward
            got = {pool: _run(h, ids, mask, pool) for pool in (0, 1)}
            monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
            for pool in (0, 1):
                assert _same(got[pool][1], own[pool][1]) and _same(got[pool][0], own[pool][0]), ("projection path differs", shape, S, tile, pool)
    print(f"[C {shape}] worst |last_hidden - fp64| {worst:.2e} (bar {BAR}), worst 1 - cos {worst_cos:.2e}")


def test_create_still_refuses_what_the_kernels_do_not_cover():
    from kirag_amd.retriever.encoders import HipBertForward
    for H, heads, FF, word in ((2176, 34, 2176, "hidden=2176"), (128, 2, 192, "intermediate=192")):
        with pytest.raises(Exception) as ei:
            HipBertForward(_cfg(H, 1, heads, FF), 0)
        assert word in str(ei.value), str(ei.value)


def _target(n, S, rng):
    """n attended tokens in columns 0 .. n + 1 with two holes, right padding behind them"""
    assert S >= n + 3
    mask = np.zeros(S, np.int64); mask[:n + 2] = 1; mask[[3, 2 + n // 2]] = 0
    ids = rng.integers(5, U.VOCAB, S) * mask
    return ids, mask


def _neighbours(S, lens, left, rng):
    """four sequences of the given attended lengths, the ones flagged in `left` left-padded, pad id 0 under the mask"""
    ids = np.zeros((4, S), np.int64); mask = np.zeros((4, S), np.int64)
    for r, (n, l) in enumerate(zip(lens, left)):
        if l: mask[r, S - n:] = 1
        else: mask[r, :n] = 1
    ids[mask != 0] = rng.integers(5, U.VOCAB, int(mask.sum()))
    return ids, mask


def _batch(target, others, at=2):
    ids = np.insert(others[0], at, target[0], axis=0); mask = np.insert(others[1], at, target[1], axis=0)
    return np.ascontiguousarray(ids), np.ascontiguousarray(mask)


@pytest.mark.parametrize("n", [31, 64, 65, 129, 257])
@pytest.mark.parametrize("dh", sorted(U.DH, reverse=True))
def test_a_row_depends_on_its_own_tokens_only_bit_for_bit(dh, n, monkeypatch):
    """Section D.  One target sequence (n attended tokens, two holes, right padding, S = n + 7) at batch index 2 of 5, generic sharp weights.  Its rows of
    last_hidden and its pooled vector, both pools, must keep their bits when
      (i)   the four other sequences are replaced by other ids and lengths (the target's packed offset moves: the two in front of it hold S + 5 tokens before,
            9 + 17 after);
      (ii)  every id under a masked column, padding and holes, of every sequence is replaced by another valid id;
      (iii) the batch runs on a fresh handle instead of one that first ran a larger, longer batch (stale k / vT slack, a reallocated workspace);
      (iv)  the batch is padded to a wider S: n <= 65 -> S = 200, which selects k_attn_dma in place of k_attn_lds; n >= 129 runs k_attn_dma at either width, so
            there the other kernel is selected by KIRAG_AMD_ATTN_LDS=1 as well.
    Under (ii) with CLS pooling the target's column 0 is attended, so no input of the compared rows changes.
    Measured on MI355X: every one of (i) - (iv) is bit-exact at every n, both head widths, both pools; there is no exception to document."""
    heads = U.DH[dh]
    cfg, w = _cfg(U.TINY["H"], U.TINY["L"], heads, U.TINY["FF"]), U.generic_model()
    rng = np.random.default_rng(1000 * dh + n)
    S = n + 7
    target = _target(n, S, rng)
    base = _batch(target, _neighbours(S, (S, 5, S - 1, 12), (0, 0, 1, 1), rng))
    used = _tiny(monkeypatch, "generic", dh)
    big = _neighbours(min(2 * S + 9, U.MAX_POS), (min(2 * S + 9, U.MAX_POS),) * 4, (0,) * 4, rng)
    for pool in (0, 1):
        _run(used, np.concatenate([big[0]] * 3), np.concatenate([big[1]] * 3), pool)          # 12 x the longest row first
        out, lh = _run(used, *base, pool)
        want = (out[2].copy(), lh[2].copy())

        def check(what, o, l):
            assert _same(o[2], want[0]), (what, "pooled", dh, n, pool, float(np.abs(o[2] - want[0]).max()))
            assert _same(l[2, :S], want[1]) and (l[2, S:] == 0).all(), (what, "last_hidden", dh, n, pool, float(np.abs(l[2, :S] - want[1]).max()))

        check("(i) other neighbours", *_run(used, *_batch(target, _neighbours(S, (9, 17, 3, S), (1, 0, 0, 1), rng)), pool))
        ids2 = np.where(base[1] != 0, base[0], rng.integers(5, U.VOCAB, base[0].shape))
        assert (ids2 != base[0]).sum() >= 7
        check("(ii) ids under the mask", *_run(used, ids2, base[1], pool))
        check("(iii) fresh handle", *_run(_new_handle(monkeypatch, cfg, w), *base, pool))
        wide = max(200, S + 64)
        wide_ids = np.zeros((5, wide), np.int64); wide_mask = np.zeros((5, wide), np.int64)
        wide_ids[:, :S] = base[0]; wide_mask[:, :S] = base[1]
        check("(iv) wider batch", *_run(used, wide_ids, wide_mask, pool))
        if S > 128:
            monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
            got = _run(used, *base, pool)
            monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
            check("(iv) the other attention kernel", *got)
