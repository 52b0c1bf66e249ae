"""GPU tests of ModernBERT checkpoints (gte-modernbert-base, modernbert-embed, granite-embedding-english-r2: ModernBertModel = a pre-LN stack without a position
table, q and k rotated in the QKV projection's epilogue with one frequency vector per layer type, the gated MLP Wo(gelu(input) * gate) from the epilogue of
the one [2 FF, H] projection, sliding-window attention in the layers the config names).  The reference is transformers.ModernBertModel in fp32 with eager
attention on synthetic weights.  The window, the two thetas, the rotation and the gate are tested on last_hidden_state, element-wise, with preconditions
asserted on the reference: each way of breaking them moves the compared rows by at least 10 x the bar.

The CLS row of a MASKED column 0 (left padding under CLS pooling) is compared with the reference only where its window holds an attended column (first
attended column <= half-window): elsewhere the reference's row is an artefact of its finite mask value (a uniform average over every column, padding
included); the library defines that row's local-attention context as zero, and the tests only ask it to be finite."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modernbert_util as M  # noqa: E402
import nomic_util as N  # noqa: E402
import xlmr_util as X  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL = -22
COS_BAR, SCORE_BAR = 5e-5, 1e-3
HIDDEN_BAR = 3e-2                        # test_g1_last_hidden_state, default mode
WIDTHS = {64: (768, 12, 1152), 32: (384, 12, 640)}  # head width -> (H, heads, FF)
TYPES4 = [M.FULL, M.SLIDING, M.SLIDING, M.FULL]


def _hip(cfg, w, **kw):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(cfg, 0, **kw)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


def _tokens(B, S, layout, seed, vocab, lo=None):
    """(ids, mask) [B,S] int64: id 2 first, real ids in [5, vocab), the pad id 0 in every column that is not attended.  R = right-padded ragged lengths
    (lo .. S, one of them S; lo defaults to S / 2), L = left-padded, F = full length."""
    rng = np.random.default_rng(seed)
    real = rng.integers(5, vocab, (B, S)); real[:, 0] = 2
    lens = rng.integers(max(2, S // 2) if lo is None else lo, S + 1, B)
    lens[0] = S
    if layout == "F":
        lens[:] = S
    ids = np.zeros((B, S), np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        n = int(lens[r])
        if layout == "L":
            ids[r, S - n:] = real[r, :n]; mask[r, S - n:] = 1
        else:
            ids[r, :n] = real[r, :n]; mask[r, :n] = 1
    return ids, mask


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _teeth_model(dh, L=4, types=None, local_attention=128, vocab=1000):
    H, heads, FF = WIDTHS[dh]
    cfg = M.cfg(H, L, heads, FF, vocab, 8192, types=TYPES4[:L] if types is None else types, local_attention=local_attention)
    return cfg, M.teeth_weights(H, L, FF, vocab)


def _assert_teeth(m, ids, mask, ref, what, window):
    """the preconditions, per sequence, on the reference: each way of breaking the feature moves the attended rows by >= 10 x the bar (the three breaks of the
    window only where `window`: sequences long enough to hold token pairs at distance 64 / 65)"""
    keep = mask.astype(bool)
    weakest = np.inf
    for how in M.BREAKS:
        if how in M.WINDOW_BREAKS and not window:
            continue
        with M.broken(m, how):
            other = M.hf_last_hidden(m, ids, mask, chunk=2 if ids.shape[1] >= 2048 else 8)
        for r in range(len(ids)):
            d = float(np.abs(ref[r] - other[r])[keep[r]].max())
            weakest = min(weakest, d)
            assert d >= 10 * HIDDEN_BAR, ("precondition", what, how, r, d)
    return weakest


def _cls_rows_with_keys(mask, w):
    """sequences whose column-0 row has an attended column inside its window"""
    first = np.argmax(mask != 0, axis=1)
    return first <= w


@pytest.mark.parametrize("dh", [64, 32])
def test_last_hidden_state_parity_where_the_features_have_teeth(dh, monkeypatch):
    """kr_encoder_last_hidden against HF's last_hidden_state, element-wise on attended rows, bar 3e-2; 4 layers [full, sliding, sliding, full], local_attention
    128, layer matrices N(0, (1.57 / sqrt(fan_in))^2): right-padded, left-padded and full-length batches at S = 32, 96, 128 (k_attn_lds), 200, 512 and one
    right-padded batch at 2048 (k_attn_dma), both pools (CLS with a masked column 0); forward_packed bit-identical on the right-padded batches.  Sequences
    of S >= 96 hold at least 80 tokens, so that every one has token pairs at distance 64 and 65 for the window's preconditions."""
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")          # read at handle creation: every row of the last layer is kept under CLS pooling too
    cfg, w = _teeth_model(dh)
    h, m = _hip(cfg, w), M.hf_model(cfg, w)
    assert h.is_modern and h.position_padding_idx is None
    worst, weakest = 0.0, np.inf
    for S, layout in [(S, lay) for S in (32, 96, 128, 200, 512) for lay in ("R", "L", "F")] + [(2048, "R")]:
        B = 2 if S >= 2048 else 3 if S >= 200 else 5
        ids, mask = _tokens(B, S, layout, 1000 + S + ord(layout), cfg.vocab_size, lo=max(S // 2, 80) if S >= 96 else None)
        keep = mask.astype(bool)
        ref = M.hf_last_hidden(m, ids, mask, chunk=2 if S >= 2048 else 8)
        weakest = min(weakest, _assert_teeth(m, ids, mask, ref, (S, layout), window=S >= 96))
        for pool in (0, 1):
            h.forward_np(ids, mask, pool)
            lh = h.last_hidden(B, S).numpy()
            err = float(np.abs(lh - ref)[keep].max())
            worst = max(worst, err)
            print(f"[d_h {dh}] S {S} {layout} pool {pool}: max |last_hidden - HF| {err:.2e}")
            assert np.isfinite(lh).all() and err <= HIDDEN_BAR, (S, layout, pool, err)
            if pool == 1 and layout == "L":
                ok = _cls_rows_with_keys(mask, cfg.sliding_window)
                e0 = float(np.abs(lh[ok, 0] - ref[ok, 0]).max())
                print(f"[d_h {dh}] S {S} L cls rows (column 0, masked in {int((mask[:, 0] == 0).sum())} of {B}, {int(ok.sum())} compared): {e0:.2e}")
                assert (mask[ok, 0] == 0).any() and e0 <= HIDDEN_BAR, (S, e0)
            if layout == "R":
                rag, lens = _rag(ids, mask)
                h.forward_packed(rag, lens, S, pool)
                assert _same(h.last_hidden(B, S).numpy()[keep], lh[keep]), (S, pool)
    print(f"[d_h {dh}] worst |last_hidden - HF| {worst:.2e} (bar {HIDDEN_BAR}); weakest precondition distance {weakest:.2f}")


@pytest.mark.parametrize("dh", [64, 32])
def test_half_window_sweep(dh):
    """Half-windows 1, 8, 31, 32, 33, 63, 64, 100 (HF local_attention = 2 w) at S = 200 and 512, ragged right-padded: the band edge at every alignment
    against the 32-key tiles and the 64-key chunks, first steps that hold none of a row's keys included.  Element-wise at the bar, all finite."""
    worst = 0.0
    for wd in (1, 8, 31, 32, 33, 63, 64, 100):
        cfg, w = _teeth_model(dh, L=3, types=[M.SLIDING, M.FULL, M.SLIDING], local_attention=2 * wd)
        h, m = _hip(cfg, w), M.hf_model(cfg, w)
        for S, B in ((200, 4), (512, 3)):
            ids, mask = _tokens(B, S, "R", 300 + S + wd, cfg.vocab_size)
            ref = M.hf_last_hidden(m, ids, mask)
            h.forward_np(ids, mask, 0)
            lh = h.last_hidden(B, S).numpy()
            err = float(np.abs(lh - ref)[mask.astype(bool)].max())
            worst = max(worst, err)
            print(f"[d_h {dh}] w {wd} S {S}: max |last_hidden - HF| {err:.2e}")
            assert np.isfinite(lh).all() and err <= HIDDEN_BAR, (wd, S, err)
    print(f"[d_h {dh}] sweep worst {worst:.2e}")


@pytest.mark.parametrize("dh", [64, 32])
def test_holes_in_the_mask(dh, monkeypatch):
    """20 % of the columns dropped at random: the window counts COLUMNS (not attended tokens), the key columns are gathered from the packed rows' columns."""
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
    cfg, w = _teeth_model(dh)
    h, m = _hip(cfg, w), M.hf_model(cfg, w)
    for S, B in ((200, 4), (512, 3)):
        ids, mask = _tokens(B, S, "R", 50 + S, cfg.vocab_size, lo=max(S // 2, 120))
        rng = np.random.default_rng(S)
        drop = rng.random((B, S)) < 0.2
        drop[:, 0] = False
        mask = mask * ~drop
        ids = ids * mask
        keep = mask.astype(bool)
        ref = M.hf_last_hidden(m, ids, mask)
        with M.broken(m, "window_minus_1"):      # the precondition: the window is what decides here too
            other = M.hf_last_hidden(m, ids, mask)
        for r in range(B):
            assert float(np.abs(ref[r] - other[r])[keep[r]].max()) >= 10 * HIDDEN_BAR, ("precondition", S, r)
        for pool in (0, 1):
            h.forward_np(ids, mask, pool)
            lh = h.last_hidden(B, S).numpy()
            err = float(np.abs(lh - ref)[keep].max())
            print(f"[d_h {dh}] holes S {S} pool {pool}: max |last_hidden - HF| {err:.2e}")
            assert np.isfinite(lh[keep]).all() and err <= HIDDEN_BAR, (S, pool, err)


@pytest.mark.parametrize("dh", [64, 32])
def test_one_arithmetic(dh, monkeypatch):
    """(a) every KIRAG_AMD_PROJ_TILE value and KIRAG_AMD_ATTN_LDS=1 give the same bits.  (b) a 100-token sequence alone (k_attn_lds) and next to a 300-token one
    (k_attn_dma): same bits.  (c) forward_packed == padded forward, a row does not depend on its batch, right-padded == left-padded.  (d) consecutive key
    columns == gathered ones (KIRAG_AMD_ATTN_BIAS_GATHER=1 at creation)."""
    cfg, w = _teeth_model(dh, L=3, types=[M.FULL, M.SLIDING, M.SLIDING], local_attention=64)
    h = _hip(cfg, w)
    rng = np.random.default_rng(5)
    for B, S, layout in ((8, 64, "R"), (24, 200, "L"), (2, 32, "F")):
        i2, m2 = _tokens(B, S, layout, 90 + S, 1000)
        for pool in (0, 1):
            monkeypatch.delenv("KIRAG_AMD_PROJ_TILE", raising=False)
            auto = h.forward_np(i2, m2, pool)
            assert np.isfinite(auto).all()
            for tile in (256, 130, 128, 64, 32):
                monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
                assert _same(h.forward_np(i2, m2, pool), auto), (B, S, pool, tile)
            monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
            monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
            assert _same(h.forward_np(i2, m2, pool), auto), (B, S, pool, "attn_lds")
            monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
    monkeypatch.setenv("KIRAG_AMD_ATTN_BIAS_GATHER", "1")
    hg = _hip(cfg, w)
    monkeypatch.delenv("KIRAG_AMD_ATTN_BIAS_GATHER")
    for pool in (0, 1):
        # (b)
        ids = np.zeros((2, 300), np.int64); mask = np.zeros((2, 300), np.int64)
        ids[0, :100] = rng.integers(5, 1000, 100); ids[1] = rng.integers(5, 1000, 300); ids[:, 0] = 2
        mask[0, :100] = 1; mask[1] = 1
        alone = h.forward_np(ids[:1, :100], mask[:1, :100], pool)
        both = h.forward_np(ids, mask, pool)
        assert np.isfinite(both).all() and _same(alone[0], both[0]), pool
        # (c), (d)
        for S in (100, 300):
            i2, m2 = _tokens(6, S, "R", 40 + S, 1000)
            a = h.forward_np(i2, m2, pool)
            rag, lens = _rag(i2, m2)
            assert _same(h.forward_packed(rag, lens, S, pool).cpu().numpy(), a), (S, pool)
            assert _same(h.forward_np(i2[2:5], m2[2:5], pool), a[2:5]), (S, pool)
            assert _same(hg.forward_np(i2, m2, pool), a), (S, pool, "gather")
            il, ml = np.zeros_like(i2), np.zeros_like(m2)
            for r in range(len(i2)):
                n = int(m2[r].sum())
                il[r, S - n:] = i2[r, :n]; ml[r, S - n:] = 1
            if pool == 0 or (ml[:, 0] != 0).all():
                assert _same(h.forward_np(il, ml, pool), a), (S, pool, "left")
            else:      # CLS pooling of a masked column 0 is another quantity: compare the rows of the mean instead
                assert _same(h.forward_np(il, ml, 0), h.forward_np(i2, m2, 0)), (S, "left")


SHAPES = {"modernbert-base": (768, 3, 12, 1152, 50368), "tiny": (128, 3, 4, 256, 3000), "ff-2624": (256, 3, 4, 2624, 3000)}      # (H, L, heads, FF, vocab)
CASES = N_CASES = {"e5": [(16, 128, "R", 1), (8, 32, "R", 2), (2, 512, "R", 3), (4, 256, "L", 4), (4, 200, "F", 5), (2, 2048, "R", 6)],
                   "bge": [(8, 128, "R", 7), (4, 256, "L", 8), (2, 512, "F", 9)]}      # test_gpu_nomic.CASES


@pytest.mark.parametrize("shape", ["modernbert-base", "tiny", "ff-2624"])
@pytest.mark.parametrize("wname", ["benign", "out3"])
def test_parity_with_hf_modernbert_fp32(shape, wname):
    """The default mode against HF ModernBertModel in fp32 with the encoders' pooling.  Bars: 1 - cos <= 5e-5, every e5 query x passage
    score within 1e-3 of the fp32 scores.  ff-2624: the intermediate size that is no multiple of 128 (zero-padded to 2688 by the Python layer).  The bge
    left-padded case pools a masked column 0: such rows are compared where the column-0 row's window holds an attended column (module docstring).  With these
    cases (test_gpu_nomic's) that may leave only the full-length row of the batch: the masked-column-0 row is not what this test is about, it is compared in
    test_last_hidden_state_parity_where_the_features_have_teeth."""
    H, L, heads, FF, vocab = SHAPES[shape]
    cfg = M.cfg(H, L, heads, FF, vocab, 8192)
    w = M.weights(H, L, FF, vocab, wname)
    h, m = _hip(cfg, w), M.hf_model(cfg, w)
    assert h.is_modern and h.ff_pad % 128 == 0 and h.ff_pad - FF < 128
    outs, refs = {}, {}
    worst_cos = 0.0
    for tag, pool in (("e5", 0), ("bge", 1)):
        for B, S, layout, seed in CASES[tag]:
            ids, mask = _tokens(B, S, layout, seed, vocab, lo=4)
            out, ref = h.forward_np(ids, mask, pool), M.hf_encode(m, ids, mask, pool, chunk=2 if S >= 2048 else 8)
            assert out.shape == ref.shape and np.isfinite(out).all()
            ok = _cls_rows_with_keys(mask, cfg.sliding_window) if pool == 1 else np.ones(B, bool)
            assert ok.any()
            cos = _cos_gap(out[ok], ref[ok])
            worst_cos = max(worst_cos, cos)
            assert cos <= COS_BAR, (tag, B, S, layout, cos)
            outs[(tag, B, S, layout)] = out; refs[(tag, B, S, layout)] = ref
    worst = 0.0
    for a in outs:
        for b in outs:
            if a[0] == b[0] == "e5":
                worst = max(worst, float(np.abs(outs[a] @ outs[b].T - refs[a] @ refs[b].T).max()))
    print(f"[{shape} {wname}] worst |q.d - ref| {worst:.2e}, worst 1 - cos {worst_cos:.2e}")
    assert worst <= SCORE_BAR, worst


def test_bf16_operands_and_no_residual_lo():
    """The other modes run, stay finite and inside their modes' bars (test_gpu_nomic.test_bf16_operands: 1e-4 for bf16 operands; f16 operands without the low
    half of the residual stream: the default mode's bar)."""
    H, L, heads, FF, vocab = SHAPES["tiny"]
    cfg = M.cfg(H, L, heads, FF, vocab, 8192)
    w = M.weights(H, L, FF, vocab, "benign")
    m = M.hf_model(cfg, w)
    ids, mask = _tokens(4, 200, "R", 3, vocab)
    ref = M.hf_encode(m, ids, mask, 0)
    hb = _hip(cfg, w, operand_dtype="bf16")
    b = hb.forward_np(ids, mask, 0)
    assert hb.operand_dtype == "bf16" and np.isfinite(b).all() and _cos_gap(b, ref) <= 1e-4
    hn = _hip(cfg, w, residual_lo=False)
    n = hn.forward_np(ids, mask, 0)
    assert not hn.residual_lo and np.isfinite(n).all() and _cos_gap(n, ref) <= COS_BAR
    for pool in (0, 1):      # the CLS shortcut carries the residual stream in both modes
        assert np.isfinite(hb.forward_np(ids, mask, pool)).all() and np.isfinite(hn.forward_np(ids, mask, pool)).all()


def test_cls_shortcut_equals_the_full_last_layer(monkeypatch):
    """CLS pooling runs the last layer's tail on the gathered CLS rows (with their residual rows): the same bits as on every row, one layer included."""
    for L in (1, 3):
        cfg, w = _teeth_model(32, L=L, types=[M.SLIDING, M.FULL, M.SLIDING][:L])
        ids, mask = _tokens(5, 200, "R", 8, 1000)
        short = _hip(cfg, w).forward_np(ids, mask, 1)
        monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
        full = _hip(cfg, w).forward_np(ids, mask, 1)
        monkeypatch.delenv("KIRAG_AMD_CLS_FULL")
        assert np.isfinite(short).all() and _same(short, full), L


def _raw_handle(layers=2, max_pos=512):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(128, layers, 4, 256, 100, max_pos, 1, 1e-5)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _load(lib, h, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)


def test_limits_and_errors():
    """Every refusal of the ModernBert handle kind through the raw C ABI, by error code and message."""
    H, heads, FF, L = 128, 4, 256, 2
    w = M.weights(H, L, FF, 100)
    gf, lf = M.inv_freq(H // heads, M.THETA[M.FULL]), M.inv_freq(H // heads, M.THETA[M.SLIDING])
    zero_types = ("embeddings.token_type_embeddings.weight", np.zeros((1, H)))

    def handle(settings, tensors, layers=L):
        lib, raw = _raw_handle(layers)
        for k, v in settings:
            assert _load(lib, raw, k, v) == 0, (k, lib.kr_last_error())
        for k, v in tensors:
            assert _load(lib, raw, k, v) == 0, (k, lib.kr_last_error())
        return lib, raw

    def refused(settings, tensors, fragment, layers=L):
        lib, raw = handle(settings, tensors, layers)
        try:
            assert lib.kr_encoder_finalize(raw) == KR_EINVAL and fragment in lib.kr_last_error(), (fragment, lib.kr_last_error())
        finally:
            lib.kr_encoder_destroy(raw)

    full = [(M.GLOBAL_FREQ_NAME, gf), (M.LOCAL_FREQ_NAME, lf), (M.HALF_WINDOW_NAME, [64.0]), (M.LAYER_FLAGS_NAME, [0.0, 1.0])]
    tensors = list(w.items()) + [zero_types]
    # the complete handle finalizes and runs
    lib, raw = handle(full, tensors)
    try:
        assert lib.kr_encoder_finalize(raw) == 0, lib.kr_last_error()
        ids = np.full((2, 200), 7, np.int64); mask = np.ones((2, 200), np.int64)
        out = np.empty((2, H), np.float32)
        assert lib.kr_encoder_forward(raw, ids.ctypes.data, mask.ctypes.data, 2, 200, 0, out.ctypes.data, None) == 0 and np.isfinite(out).all()
        # after the first finalize: the same values are a no-op, anything else is refused
        for k, v in full:
            assert _load(lib, raw, k, v) == 0, k
        for k, v in ((M.LOCAL_FREQ_NAME, 2 * lf), (M.HALF_WINDOW_NAME, [63.0]), (M.LAYER_FLAGS_NAME, [1.0, 1.0]), (M.LAYER_FLAGS_NAME, [0.0, 1.0, 0.0])):
            assert _load(lib, raw, k, v) == KR_EINVAL and b"finalize" in lib.kr_last_error(), k
    finally:
        lib.kr_encoder_destroy(raw)
    # wrong counts / values at load time
    lib, raw = _raw_handle()
    try:
        assert _load(lib, raw, M.LOCAL_FREQ_NAME, lf[:3]) == KR_EINVAL and b"16" in lib.kr_last_error()
        assert _load(lib, raw, M.HALF_WINDOW_NAME, [0.0]) == KR_EINVAL and b">= 1" in lib.kr_last_error()
        assert _load(lib, raw, M.HALF_WINDOW_NAME, [1.0, 2.0]) == KR_EINVAL
        assert _load(lib, raw, M.LAYER_FLAGS_NAME, [0.0, 2.0]) == KR_EINVAL and b"0 / 1" in lib.kr_last_error()
        assert _load(lib, raw, "layers.0.attn_norm.weight", np.ones(H)) == KR_EINVAL and b"identity" in lib.kr_last_error()
        assert _load(lib, raw, "layers.0.attn.Wqkv.bias", np.ones(2 * H)) == KR_EINVAL
        assert _load(lib, raw, "layers.0.attn.Wqkv.weight", np.ones(H * H)) == KR_EINVAL
    finally:
        lib.kr_encoder_destroy(raw)
    # a flag list whose length is not the layer count
    refused(full[:3] + [(M.LAYER_FLAGS_NAME, [0.0, 1.0, 0.0])], tensors, b"config.local_attention_layers holds 3 flags")
    # local layers without their frequencies / without the half-window; the flags without the global frequencies
    refused([full[0], full[2], full[3]], tensors, b"config.rotary_inv_freq_local")
    refused([full[0], full[1], full[3]], tensors, b"config.attention_half_window")
    refused(full[1:], tensors, b"without config.rotary_inv_freq")
    # ModernBert's names on a handle of another kind (a NomicBert handle here), and the reverse
    refused([full[0]], tensors, b"ModernBert name")
    nomic = {k: v for k, v in N.weights(H, L, heads, FF, 100).items() if "token_type" not in k}      # (its two type rows: this handle has one)
    refused(full, list(nomic.items()) + [zero_types], b"takes ModernBert's names")
    # the settings next to the other position schemes
    refused(full + [("config.position_padding_idx", [1.0])], tensors, b"one position scheme")
    refused(full, tensors + [("encoder.relative_attention_bias.weight", np.zeros((32, heads)))], b"one position scheme")
    # the local settings without the flags
    refused(full[:3], list(nomic.items()) + [zero_types], b"without config.local_attention_layers")
    # all layers global: the local settings are not needed; optional biases and betas are taken
    lib, raw = handle([full[0], (M.LAYER_FLAGS_NAME, [0.0, 0.0])], tensors + [("layers.1.mlp.Wi.bias", np.zeros(2 * FF)), ("layers.0.mlp_norm.bias", np.zeros(H)),
                                                                               ("final_norm.bias", np.zeros(H)), ("layers.1.attn.Wo.bias", np.zeros(H))])
    try:
        assert lib.kr_encoder_finalize(raw) == 0, lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(raw)
    # a tensor that was never loaded
    lib, raw = handle(full, [kv for kv in tensors if kv[0] != "layers.1.mlp.Wi.weight"])
    try:
        assert lib.kr_encoder_finalize(raw) != 0 and b"never loaded" in lib.kr_last_error()
        assert _load(lib, raw, "layers.1.mlp.Wi.weight", w["layers.1.mlp.Wi.weight"]) == 0 and lib.kr_encoder_finalize(raw) == 0
    finally:
        lib.kr_encoder_destroy(raw)


@pytest.mark.parametrize("dh", [64, 32])
def test_optional_biases_are_computed(dh, monkeypatch):
    """attn.Wqkv / attn.Wo / mlp.Wi / mlp.Wo biases and every LayerNorm beta (attention_bias, mlp_bias, norm_bias) against HF with the same tensors, on weights
    with teeth.  The q / k bias is added before the rotation (EPI_QKV_ROTB): a precondition asserts that dropping the Wqkv bias alone moves the rows by
    >= 10 x the bar.  Every projection path gives the same bits."""
    from transformers import ModernBertModel
    H, heads, FF = WIDTHS[dh]
    L, vocab = 3, 1000
    cfg = M.cfg(H, L, heads, FF, vocab, 8192, types=[M.FULL, M.SLIDING, M.FULL], attention_bias=True, mlp_bias=True, norm_bias=True)
    w = M.teeth_weights(H, L, FF, vocab)
    rng = np.random.default_rng(1)
    m = ModernBertModel(M.hf_config(cfg))
    state = {k: torch.from_numpy(v) for k, v in w.items()}
    for k, v in m.state_dict().items():
        if k.endswith(".bias"):
            state[k] = torch.from_numpy(((1.0 if "Wqkv" in k else 0.1) * rng.standard_normal(tuple(v.shape))).astype(np.float32))
    assert "layers.1.attn.Wqkv.bias" in state and "layers.1.attn.Wo.bias" in state and "layers.0.mlp.Wi.bias" in state and "final_norm.bias" in state
    res = m.load_state_dict(state, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    m = m.float().eval().cuda()
    h = _hip(cfg, {k: v.numpy() for k, v in state.items()})
    ids, mask = _tokens(4, 200, "R", 3, vocab)
    keep = mask.astype(bool)
    ref = M.hf_last_hidden(m, ids, mask)
    for only in ("Wqkv.bias", ".bias"):      # the preconditions: the fused projection's bias alone matters, and so do the others
        saved = {k: v.clone() for k, v in m.state_dict().items() if k.endswith(only) or (only == ".bias" and k.endswith(".bias") and "Wqkv" not in k)}
        if only == ".bias":
            saved = {k: v for k, v in saved.items() if "Wqkv" not in k}
        with torch.no_grad():
            for k in saved:
                m.state_dict()[k].zero_()
        moved = float(np.abs(M.hf_last_hidden(m, ids, mask) - ref)[keep].max())
        with torch.no_grad():
            for k, v in saved.items():
                m.state_dict()[k].copy_(v)
        assert moved >= 10 * HIDDEN_BAR, ("precondition", only, moved)
    h.forward_np(ids, mask, 0)
    lh = h.last_hidden(4, 200).numpy()
    err = float(np.abs(lh - ref)[keep].max())
    print(f"[d_h {dh}] biases: max |last_hidden - HF| {err:.2e}")
    assert np.isfinite(lh).all() and err <= HIDDEN_BAR, err
    for B, S in ((4, 200), (8, 64), (2, 32), (40, 200)):
        i2, m2 = _tokens(B, S, "R", 7 + S, vocab)
        auto = h.forward_np(i2, m2, 0)
        for tile in (256, 130, 128, 64, 32):
            monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
            assert _same(h.forward_np(i2, m2, 0), auto), (B, S, tile)
        monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")


def test_residual_overflow_raises_kr_erange():
    """A pre-LN residual stream that leaves the f16 range while every projection output stays inside it: mlp.Wo.bias = 40000 on one channel in each of three
    layers (the bias is added in fp32 by the LayerNorm launch, the projection's own output stays small), so the residual is 40000 behind layer 0 and 80000 —
    beyond 65504 — behind layer 1.  Nothing but the next LayerNorm launch ever reads the stored residual, so that launch has to keep the overflow alive: the
    default mode (f16 + low half) and f16 without the low half raise KR_ERANGE; bf16 operands give a finite result that matches HF."""
    from transformers import ModernBertModel
    from kirag_amd import _lib
    H, L, heads, FF, vocab = 128, 3, 4, 256, 500
    cfg = M.cfg(H, L, heads, FF, vocab, 8192, mlp_bias=True)
    w = M.weights(H, L, FF, vocab, "benign")
    for l in range(L):
        w[f"layers.{l}.mlp.Wi.bias"] = np.zeros(2 * FF, np.float32)
        b = np.zeros(H, np.float32); b[5] = 40000.0
        w[f"layers.{l}.mlp.Wo.bias"] = b
    m = ModernBertModel(M.hf_config(cfg))
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    m = m.float().eval().cuda()
    ids, mask = _tokens(4, 64, "R", 3, vocab)
    # the preconditions, on the reference: the residual behind each layer, and the largest projection output (what is stored as a 16-bit value by itself)
    resid, proj = [], []
    hooks = [l.register_forward_hook(lambda _m, _i, o: resid.append(float(o.abs().max()))) for l in m.layers]
    for l in m.layers:
        for mod in (l.attn.Wqkv, l.attn.Wo, l.mlp.Wi):
            hooks.append(mod.register_forward_hook(lambda _m, _i, o: proj.append(float(o.abs().max()))))
        hooks.append(l.mlp.Wo.register_forward_hook(lambda mod, _i, o: proj.append(float((o - mod.bias).abs().max()))))
    ref = M.hf_encode(m, ids, mask, 0)
    for hk in hooks:
        hk.remove()
    assert resid[0] < 65504 < resid[1] and max(proj) < 6000 and np.isfinite(ref).all(), (resid, max(proj))
    for kw in ({}, {"residual_lo": False}):
        h = _hip(cfg, w, **kw)
        assert h.operand_dtype == "f16"
        with pytest.raises(_lib.KiragAmdError) as ei:
            h.forward_np(ids, mask, 0)
        assert ei.value.code == -34, ei.value            # KR_ERANGE
    hb = _hip(cfg, w, operand_dtype="bf16")
    out = hb.forward_np(ids, mask, 0)
    assert np.isfinite(out).all() and _cos_gap(out, ref) <= 1e-4, _cos_gap(out, ref)


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_reference_entry_points_on_a_saved_modernbert_checkpoint(tmp_path, name, pool):
    """save_pretrained a tiny ModernBertModel + a toy fast tokenizer; load_retriever(<existing name>, dir) returns the ModernBert twin, whose embeddings of
    tokenized text match HF fp32 within the embedding bars."""
    from kirag_amd.collators import COLLATOR_MAP
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import InBatchRetriever, load_retriever
    words = X.toy_words(400)
    tok = X.toy_tokenizer(words)
    vocab = tok.vocab_size
    H, L, heads, FF = 128, 3, 4, 200      # FF 200: the padding path on a saved checkpoint
    cfg = M.cfg(H, L, heads, FF, vocab, 512, local_attention=16)
    w = M.weights(H, L, FF, vocab, "out3")
    td = str(tmp_path / "model")
    m = M.hf_model(cfg, w, device="cpu")
    m.save_pretrained(td)
    tok.save_pretrained(td)
    twin = {"E5Retriever": ENC.ModernBertE5Encoder, "BGERetriever": ENC.ModernBertBGEEncoder}[name]
    assert type(load_retriever(name, td)) is twin
    ret = InBatchRetriever(name, td, temperature=0.01)
    assert type(ret.encoder) is twin and ret.hidden_size == H
    ret.encoder.eval().cuda()
    rng = np.random.default_rng(9)
    texts = [" ".join(rng.choice(words, int(rng.integers(3, 40)))) for _ in range(64)]
    col = COLLATOR_MAP[name](tokenizer=tok, query_maxlength=24, doc_maxlength=48)
    a = col.encode_doc(texts)
    ids, mask = a["input_ids"].numpy(), a["attention_mask"].numpy()
    assert (mask == 0).any()
    out = ret.encoder(a["input_ids"].cuda(), a["attention_mask"].cuda()).cpu().numpy()
    hip = ret.encoder._hip
    assert hip.is_modern and hip.ff_pad == 256
    ref = M.hf_encode(m.cuda(), ids, mask, pool)
    cos, dscore = _cos_gap(out, ref), float(np.abs(out @ out.T - ref @ ref.T).max())
    print(f"[{name}] vs HF fp32: 1 - cos {cos:.2e}, |q.d - ref| {dscore:.2e}")
    assert np.isfinite(out).all() and cos <= COS_BAR and dscore <= SCORE_BAR

