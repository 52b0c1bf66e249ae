"""Rotary positions beyond 2048 tokens, through the model: the decoder handles (causal attention, grouped-query K / V), EuroBERT, NomicBert, jina-v3 (bidirectional)
and ModernBert (global and local layers, both rotary tables) on one batch of 8192, 4097, 2049, 300 and 1 tokens against HF fp32 eager at the families' bars, right- and left-padded; bit identity of the long rows; and the LAST row of the rotary table on a
handle whose max_position_embeddings equals the batch width.

What makes these comparisons bite is asserted on the reference first: rotary positions clamped at 2047 move rows beyond 2048 by >= 0.3, positions taken
mod 4096 move rows beyond 4096 by >= 0.3, the last position wrapped to 0 moves the last row by >= 0.3, ModernBert's window one narrower or one wider moves every
sequence by >= 0.3.  (That ATTENTION over 8192 keys is right — a step lost deep
in a ring — parity through a model cannot see: tests/test_gpu_attn_probe.py does, on the kernels alone.)

Kinds: qwen2-32 (4 heads of 32 over 2 KV heads), llama-64 (2 heads of 64 over 1), euro-32, jina-32, nomic-32 (12 heads of 32, the teeth weights of
tests/test_gpu_nomic.py) and modern-32 (4 heads of 32, layers global / local / local, half-window 64, modernbert_util.teeth_weights)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as DC  # noqa: E402
import eurobert_util as EB  # noqa: E402
import attention_edges_util as A  # noqa: E402
import jina3_util as J3  # noqa: E402
import modernbert_util as MB  # noqa: E402
import nomic_util as N  # noqa: E402

pytestmark = pytest.mark.gpu

HIDDEN_BAR, COS_BAR, MOVE = 3e-2, 5e-5, 0.3
POOL_MEAN, POOL_LAST = 0, 5


class NM:
    """NomicBert: H 384, 12 heads of 32, 3 layers, matrices N(0, 0.08^2) x 4 (the scale at which the rotation decides rows, tests/test_gpu_nomic.py)"""
    pool_np = staticmethod(N.pool_np)

    @staticmethod
    def hf_config(kind, L, max_pos):
        return N.cfg(384, 3, 12, 1536, 1000, max_pos)

    @staticmethod
    def weights(cfg):
        return N.weights(384, 3, 12, 1536, 1000, "benign", seed=11, matrix_scale=4.0)

    @staticmethod
    def hf_model(cfg, w, device):
        return N.hf_model(cfg, w, device)


class MD:
    """ModernBert: H 128, 4 heads of 32, layers global / local / local (theta 160000 / 10000), local_attention 128, weights under which the window decides rows"""
    pool_np = staticmethod(MB.pool_np)

    @staticmethod
    def hf_config(kind, L, max_pos):
        return MB.cfg(128, 3, 4, 256, 1000, max_pos, types=[MB.FULL, MB.SLIDING, MB.SLIDING], local_attention=2 * A.WINDOW)

    @staticmethod
    def weights(cfg):
        return MB.teeth_weights(128, 3, 256, 1000)

    @staticmethod
    def hf_model(cfg, w, device):
        return MB.hf_model(cfg, w, device)


KINDS = ("qwen2-32", "llama-64", "euro-32", "jina-32", "nomic-32", "modern-32")
# euro-32: 4 heads of 32 over 2 KV heads, no causal mask; jina-32: 4 heads of 32, post-LN, rotary
UTIL = {"qwen2-32": DC, "llama-64": DC, "euro-32": EB, "jina-32": J3, "nomic-32": NM, "modern-32": MD}
S_LONG = 8192
LENS = [8192, 4097, 2049, 300, 1]
S_TABLE = 300          # the width of the last-table-row test: wrapping position 299 to 0 moves the last row by 0.68 (llama-64) / 1.09 (qwen2-32) / 0.72 (euro-32) / 0.60 (jina-32) / 0.92 (nomic-32) / 3.4 (modern-32) on HF fp32


def _note(line):
    print(line)
    path = os.environ.get("KIRAG_AMD_MEASUREMENTS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cos_gap(out, ref):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return float((1.0 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


@functools.lru_cache(maxsize=None)
def _model(kind, max_pos):
    """(config, handle, HF model on the GPU) of a 2-layer decoder with max_pos positions"""
    from kirag_amd.retriever.encoders import HipBertForward
    F = UTIL[kind]
    cfg = F.hf_config(kind, 2, max_pos=max_pos)
    w = F.weights(cfg)
    h = HipBertForward(cfg, 0)
    h.load_state(w)
    assert h.is_decoder == (F in (DC, EB)) and (h.decoder_attention == 1.0) == (F is DC)      # EuroBERT: the decoders' stack under a bidirectional mask
    assert bool(h.is_nomic) == (F is NM) and bool(h.is_modern) == (F is MD)
    return cfg, h, F.hf_model(cfg, w, "cuda")


@torch.no_grad()
def _hf_alone(m, row, pos=None):
    """HF last_hidden_state [n, H] fp32 of ONE unpadded sequence (positions 0 .. n - 1, or `pos`)"""
    a = torch.from_numpy(np.ascontiguousarray(row[None])).cuda()
    p = None if pos is None else torch.from_numpy(np.ascontiguousarray(pos[None])).cuda()
    return m(input_ids=a, position_ids=p).last_hidden_state[0].float().cpu().numpy()


def _tokens(kind, lens, S, side):
    """(ids, mask): the same rows right- or left-padded (the decoders' ids in [3, 200); NomicBert / ModernBert: id 2 first, then ids in [5, 1000))"""
    if UTIL[kind] in (NM, MD):
        return A.ragged(lens, S, side, 53, 5, 1000, first=2)
    return DC.tokens(len(lens), S, "R" if side == "right" else "L", 71, lens=lens)


@functools.lru_cache(maxsize=None)
def _batch(kind):
    """the right-padded batch, the same sequences left-padded, and every sequence's HF reference alone"""
    _, _, m = _model(kind, S_LONG)
    ids, mask = _tokens(kind, LENS, S_LONG, "right")
    lids, lmask = _tokens(kind, LENS, S_LONG, "left")
    refs = [_hf_alone(m, ids[r, :n]) for r, n in enumerate(LENS)]
    for r, n in enumerate(LENS):
        assert np.array_equal(lids[r, S_LONG - n:], ids[r, :n])
    return ids, mask, lids, lmask, refs


@pytest.mark.parametrize("kind", KINDS)
def test_reference_feels_positions_beyond_2048(kind):
    """the preconditions, on HF fp32: clamping the rotary positions at 2047 moves rows beyond column 2048, taking them mod 4096 moves rows beyond column 4096,
    each by >= 0.3 (under the causal mask no row before: a bidirectional row sees the keys behind it)"""
    _, _, m = _model(kind, S_LONG)
    ids, _, _, _, refs = _batch(kind)
    pos = np.arange(S_LONG)
    d = np.abs(_hf_alone(m, ids[0], np.minimum(pos, 2047)) - refs[0]).max(1)
    causal = UTIL[kind] is DC
    assert (d[:2048].max() < 1e-4 or not causal) and (d[2048:] >= MOVE).sum() >= 1000, (float(d[:2048].max()), int((d[2048:] >= MOVE).sum()))
    d2 = np.abs(_hf_alone(m, ids[0], pos % 4096) - refs[0]).max(1)
    assert (d2[:4096].max() < 1e-4 or not causal) and (d2[4096:] >= MOVE).sum() >= 20, (float(d2[:4096].max()), int((d2[4096:] >= MOVE).sum()))
    _note(f"[{kind}] HF fp32, 8192 tokens: positions clamped at 2047 move {int((d >= MOVE).sum())} rows by >= {MOVE} (first {int(np.argmax(d >= MOVE))}, worst {d.max():.2f}); "
          f"mod 4096: {int((d2 >= MOVE).sum())} rows (first {int(np.argmax(d2 >= MOVE))}, worst {d2.max():.2f})")


def test_reference_feels_the_window_at_every_length():
    """ModernBert's precondition, on HF fp32: the window one narrower or one wider moves every sequence of the batch by >= 0.3 (the one-token sequence has no
    window to move)"""
    _, _, m = _model("modern-32", S_LONG)
    ids, _, _, _, refs = _batch("modern-32")
    for how in ("window_minus_1", "window_plus_1"):
        with MB.broken(m, how):
            moved = [float(np.abs(_hf_alone(m, ids[r, :n]) - refs[r]).max()) for r, n in enumerate(LENS) if n > 1]
        _note(f"[modern-32] HF fp32, {how}: every sequence of {LENS[:-1]} moves by {['%.2f' % d for d in moved]}")
        assert min(moved) >= MOVE, (how, moved)


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_up_to_8192_tokens(kind, side):
    """last_hidden_state of every attended row within 3e-2 of HF fp32 eager, mean- and last-token-pooled embeddings within 1 - cos <= 5e-5.  A left-padded row is
    compared with the reference of its sequence ALONE (positions 0 .. n - 1): rotary scores depend on column differences only, so in exact arithmetic the
    padding moves nothing; the handle rotates by the column inside the sequence either way"""
    _, h, _ = _model(kind, S_LONG)
    ids, mask, lids, lmask, refs = _batch(kind)
    if side == "left":
        ids, mask = lids, lmask
    out = h.forward_np(ids, mask, POOL_MEAN)
    lh = h.last_hidden(*ids.shape).numpy()
    last = h.forward_np(ids, mask, POOL_LAST) if h.decoder_attention == 1.0 else None
    keep = mask.astype(bool)
    assert np.isfinite(lh).all() and not lh[~keep].any()
    ref = np.zeros_like(lh)
    for r, n in enumerate(LENS):
        ref[r][keep[r]] = refs[r]
    per_row = [float(np.abs(lh[r] - ref[r])[keep[r]].max()) for r in range(len(LENS))]
    cos_mean = _cos_gap(out, UTIL[kind].pool_np(ref, mask, POOL_MEAN))
    cos_last = _cos_gap(last, DC.pool_np(ref, mask, POOL_LAST)) if last is not None else 0.0
    beyond = float(np.abs(lh[0] - ref[0])[keep[0]][4096:].max())
    _note(f"[{kind}] {side}-padded {LENS}: max |last_hidden - HF| per sequence {['%.2e' % e for e in per_row]} (bar {HIDDEN_BAR}; rows beyond 4096: {beyond:.2e}), "
          f"1 - cos mean {cos_mean:.2e} last {cos_last:.2e} (bar {COS_BAR})")
    assert max(per_row) <= HIDDEN_BAR, per_row
    assert cos_mean <= COS_BAR and cos_last <= COS_BAR, (cos_mean, cos_last)
    h.check()


@pytest.mark.parametrize("kind", KINDS)
def test_long_rows_are_one_arithmetic(kind, monkeypatch):
    """bit for bit at 4097 and 8192 tokens: alone == in the batch == kr_encoder_forward_packed == KIRAG_AMD_ATTN_LDS=1 (k_attn_lds instead of k_attn_dma)"""
    monkeypatch.delenv("KIRAG_AMD_ATTN_LDS", raising=False)
    _, h, _ = _model(kind, S_LONG)
    ids, mask, _, _, _ = _batch(kind)
    out = h.forward_np(ids, mask, POOL_MEAN)
    lh = h.last_hidden(*ids.shape).numpy()
    for r, n in ((0, 8192), (1, 4097)):
        o1 = h.forward_np(ids[r:r + 1, :n].copy(), mask[r:r + 1, :n].copy(), POOL_MEAN)
        l1 = h.last_hidden(1, n).numpy()
        assert _same(o1[0], out[r]) and _same(l1[0], lh[r, :n]), ("alone", n)
    rag = torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32)))
    rl = torch.from_numpy(mask.sum(1).astype(np.int32))
    assert _same(h.forward_packed(rag, rl, S_LONG, POOL_MEAN).cpu().numpy(), out), "packed"
    assert _same(h.last_hidden(len(ids), S_LONG).numpy(), lh), "packed rows"
    monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
    o4 = h.forward_np(ids, mask, POOL_MEAN)
    l4 = h.last_hidden(*ids.shape).numpy()
    bad = [n for r, n in enumerate(LENS) if not _same(l4[r], lh[r])]
    assert not bad and _same(o4, out), ("k_attn_lds vs k_attn_dma", bad)
    monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
    h.check()


@pytest.mark.parametrize("kind", KINDS)
def test_last_row_of_the_rotary_table(kind):
    """At 8192 tokens the table's last row has no teeth (wrapping position 8191 moves the worst row by 0.08), so it is tested where it has: a handle with
    max_position_embeddings = 300 on a batch 300 wide.  Precondition on HF fp32: position 299 wrapped to 0 moves the last row by >= 0.3"""
    _, h, m = _model(kind, S_TABLE)
    lens = [S_TABLE, 257, 1]
    ids, mask = _tokens(kind, lens, S_TABLE, "right")
    refs = [_hf_alone(m, ids[r, :n]) for r, n in enumerate(lens)]
    pos = np.arange(S_TABLE); pos[-1] = 0
    moved = float(np.abs(_hf_alone(m, ids[0], pos) - refs[0])[-1].max())
    assert moved >= MOVE, moved
    h.forward_np(ids, mask, POOL_MEAN)
    lh = h.last_hidden(*ids.shape).numpy()
    errs = [float(np.abs(lh[r, :n] - refs[r]).max()) for r, n in enumerate(lens)]
    last_row = float(np.abs(lh[0, S_TABLE - 1] - refs[0][-1]).max())
    _note(f"[{kind}] max_pos = width = {S_TABLE}: last row |last_hidden - HF| {last_row:.2e} (wrapping its position moves the reference by {moved:.2f}); per sequence {['%.2e' % e for e in errs]}")
    assert max(errs) <= HIDDEN_BAR, errs
    h.check()
