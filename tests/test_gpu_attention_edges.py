"""GPU tests of the four non-plain attention modes at the lengths where their kernels change path (tests/attention_edges_util.py names the boundary every
length sits on; tests/test_attention_edges_host.py asserts that the lists cover them and that the keys at those boundaries decide rows of the references).

  causal (decoder handles, AM_CAUSAL in k_attn_lds and k_attn_dma): parity with HF fp32 eager attention on a 17 x 1024 batch whose lengths put a q-group of
      one query, the first two-tile wave of a second q-group, a third and a fourth q-group, clipped rings that wrap and every kind of last chunk into ONE
      forward, right-padded, left-padded and with holes; the short batches for each HPB; last-token pooling; causality at the q-group edges of 1024 tokens
  disentangled (DeBERTa handles, AM_DISENT in k_attn_lds + k_pos_scores): parity on a 12 x 512 batch on the kchunk remainders, the short batches, W = 32 and
      96, T = 127 / 128 / 129; shift invariance; reuse of the position-score buffer across widths
  all four (also ModernBert's window and T5's bias): one arithmetic — every edge length alone == in the batch == reversed == packed == the other kernel ==
      gathered key columns, bit for bit

Tiny models (H 128 as 2 x 64 and 4 x 32 heads, 2 or 3 layers).  Bars: last_hidden_state 3e-2 element-wise on attended rows, embeddings
1 - cos <= 5e-5.  The worst measured values are printed, and appended to the file KIRAG_AMD_MEASUREMENTS_FILE names (profiles/attention_edges/measurements.txt
is such a run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_edges_util as A  # noqa: E402
import deberta_util as DB  # noqa: E402
import decoder_util as DC  # noqa: E402
import modernbert_util as MB  # noqa: E402
import t5_util as T5  # noqa: E402

pytestmark = pytest.mark.gpu

HIDDEN_BAR, COS_BAR = 3e-2, 5e-5
POOL_MEAN, POOL_CLS, POOL_LAST = 0, 1, 5


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


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _handle(cfg, w, gather=False):
    """a handle on (cfg, w); `gather`: created under KIRAG_AMD_ATTN_BIAS_GATHER=1 (read at creation)"""
    from kirag_amd.retriever.encoders import HipBertForward
    old = os.environ.get("KIRAG_AMD_ATTN_BIAS_GATHER")
    if gather:
        os.environ["KIRAG_AMD_ATTN_BIAS_GATHER"] = "1"
    else:
        os.environ.pop("KIRAG_AMD_ATTN_BIAS_GATHER", None)
    try:
        h = HipBertForward(cfg, 0)
    finally:
        os.environ.pop("KIRAG_AMD_ATTN_BIAS_GATHER", None)
        if old is not None:
            os.environ["KIRAG_AMD_ATTN_BIAS_GATHER"] = old
    h.load_state(w)
    return h


def _run(h, ids, mask, pool=POOL_MEAN):
    """(pooled rows, last_hidden) of one forward"""
    out = h.forward_np(ids, mask, pool)
    return out, h.last_hidden(*ids.shape).numpy()


# ---------------------------------------------------------------------------------------------------------
# models: built once per module, never changed
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder(kind):
    """(config, weights, handle, HF model on the GPU) of a 2-layer decoder with 1024 positions"""
    cfg = DC.hf_config(kind, 2, max_pos=A.DECODER_LONG_S)
    w = DC.weights(cfg)
    h = _handle(cfg, w)
    assert h.is_decoder
    return cfg, w, h, DC.hf_model(cfg, w, "cuda")


@functools.lru_cache(maxsize=None)
def _deberta(bm, heads):
    """(config, weights, handle, HF model on the CPU: its attention is eager only)"""
    c = DB.cfg(heads=heads, Bk=bm[0], M=bm[1])
    w = DB.weights(c)
    h = _handle(c, w)
    assert h.is_deberta
    return c, w, h, DB.hf_model(c, w)


def _t5(heads):
    return T5.cfg(128, 2, heads, 256, 1000, T5.RELU), T5.weights(128, 2, heads, 256, 1000, T5.RELU)


# ---------------------------------------------------------------------------------------------------------
# 3. decoder
# ---------------------------------------------------------------------------------------------------------
def _decoder_batches():
    """(name, ids, mask): the long batch right-padded, left-padded and with 5 holes per row, and the three short batches"""
    out = [("long right", *A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "R", 31)),
           ("long left", *A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "L", 32)),
           ("long holes", *A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "R", 33, holes=5))]
    for S, lens in A.SHORT.items():
        out.append((f"short {S}", *A.decoder_batch(lens, S, "R", 40 + S)))
    return out


@pytest.mark.parametrize("kind", A.DECODER_KINDS)
def test_decoder_parity_at_the_edges(kind):
    """last_hidden_state on attended rows within 3e-2 of HF fp32 (its own causal mask), masked rows zero, mean-pooled and last-token-pooled embeddings within
    1 - cos <= 5e-5, on the long batch (17 lengths up to 1024: k_attn_dma with up to four q-groups) in three layouts and on the short batches (k_attn_lds, HPB
    4 / 2 / 1)"""
    cfg, w, h, m = _decoder(kind)
    worst = 0.0
    for name, ids, mask in _decoder_batches():
        keep = mask.astype(bool)
        ref = DC.hf_last_hidden(m, ids, mask, chunk=6)
        out, lh = _run(h, ids, mask, POOL_MEAN)
        last = h.forward_np(ids, mask, POOL_LAST)
        err = float(np.abs(lh - ref)[keep].max())
        per_row = [float(np.abs(lh[r] - ref[r])[keep[r]].max()) for r in range(len(ids))]
        cos_mean, cos_last = _cos_gap(out, DC.pool_np(ref, mask, POOL_MEAN)), _cos_gap(last, DC.pool_np(ref, mask, POOL_LAST))
        worst = max(worst, err)
        _note(f"[{kind}] {name}: max |last_hidden - HF| {err:.2e} (bar {HIDDEN_BAR}; worst row: {int(mask[int(np.argmax(per_row))].sum())} keys), "
              f"1 - cos mean {cos_mean:.2e} last {cos_last:.2e} (bar {COS_BAR})")
        assert np.isfinite(lh).all() and not lh[~keep].any(), name
        assert err <= HIDDEN_BAR, (name, err, per_row)
        assert cos_mean <= COS_BAR and cos_last <= COS_BAR, (name, cos_mean, cos_last)
    h.check()
    _note(f"[{kind}] causal attention at the edge lengths vs HF fp32 eager: worst {worst:.2e} (bar {HIDDEN_BAR})")


def _pool_norm(rows):
    """k_pool's normalisation of a [B, H <= 256] row in its own fp32 order: squares per lane, the xor-butterfly of each 64-lane wave (lane 0: halves folded
    32, 16, .. 1), the waves' sums added in wave order, sqrtf, one division per element"""
    x = np.ascontiguousarray(rows, np.float32)
    sq = x * x
    pad = (-sq.shape[1]) % 64
    sq = np.concatenate([sq, np.zeros((len(sq), pad), np.float32)], 1).reshape(len(sq), -1, 64)
    while sq.shape[2] > 1:
        half = sq.shape[2] // 2
        sq = sq[:, :, :half] + sq[:, :, half:]
    n2 = sq[:, 0, 0]
    for wv in range(1, sq.shape[1]):
        n2 = n2 + sq[:, wv, 0]
    return x / np.maximum(np.sqrt(n2), np.float32(1e-12))[:, None]


@pytest.mark.parametrize("kind", A.DECODER_KINDS)
def test_decoder_last_token_pooling_on_the_long_batch(kind):
    """pool 5 == the normalised last attended row of kr_encoder_last_hidden for every sequence of the long batch, in every layout: bit for bit under k_pool's
    own fp32 normalisation, and within 2e-7 of the float64 one (test_last_token_pooling's)"""
    cfg, w, h, m = _decoder(kind)
    for name, ids, mask in _decoder_batches()[:3]:
        out, lh = _run(h, ids, mask, POOL_LAST)
        at = DC.last_index(mask)
        assert (at >= 0).all() and (mask[np.arange(len(ids)), at] == 1).all()
        rows = lh[np.arange(len(ids)), at]
        want64 = rows.astype(np.float64)
        want64 = (want64 / np.linalg.norm(want64, axis=1, keepdims=True)).astype(np.float32)
        assert np.abs(out - want64).max() <= 2e-7, (name, float(np.abs(out - want64).max()))
        want = _pool_norm(rows)
        bad = [int(mask[r].sum()) for r in range(len(ids)) if not _same(out[r], want[r])]
        assert not bad, (name, bad)


@pytest.mark.parametrize("kind", A.DECODER_KINDS)
def test_decoder_causality_at_the_q_group_edges(kind):
    """one full sequence of 1024 tokens: changing the token at column c leaves every row of a column < c bit-identical and moves some row >= c by > 1e-2, for c
    on both sides of every q-group edge and at the last column"""
    cfg, w, h, m = _decoder(kind)
    ids, mask = DC.tokens(1, A.DECODER_LONG_S, "F", 77)
    base = _run(h, ids, mask)[1]
    assert np.isfinite(base).all()
    for c in A.CAUSAL_COLUMNS:
        lh = _run(h, A.one_changed(ids, c), mask)[1]
        assert _same(lh[0, :c], base[0, :c]), c
        assert np.abs(lh[0, c:] - base[0, c:]).max() > 1e-2, c


# ---------------------------------------------------------------------------------------------------------
# 4. DeBERTa
# ---------------------------------------------------------------------------------------------------------
DEBERTA_PARAMS = [(bm, heads) for bm in A.DEBERTA_SHAPES for heads in A.DEBERTA_HEADS]
DEBERTA_IDS = [f"Bk{bm[0]}-heads{heads}" for bm, heads in DEBERTA_PARAMS]


def _deberta_parity(h, m, name, ids, mask, cls, tag):
    """one batch against HF: returns the worst element-wise error"""
    att = mask.astype(bool)
    ref = DB.hf_hidden(m, ids, mask)
    out, hid = _run(h, ids, mask, POOL_MEAN)
    err = float(np.abs(hid - ref)[att].max())
    per_row = [float(np.abs(hid[r] - ref[r])[att[r]].max()) for r in range(len(ids))]
    cos = _cos_gap(out, DB.pooled(ref, mask, POOL_MEAN))
    line = f"[{tag}] {name}: max |last_hidden - HF| {err:.2e} (bar {HIDDEN_BAR}; worst row: {int(mask[int(np.argmax(per_row))].sum())} keys), 1 - cos mean {cos:.2e}"
    assert np.isfinite(hid).all() and not hid[~att].any(), name
    if cls:
        assert att[:, 0].all()
        cos_cls = _cos_gap(h.forward_np(ids, mask, POOL_CLS), DB.pooled(ref, mask, POOL_CLS))
        line += f" cls {cos_cls:.2e}"
    _note(line + f" (bar {COS_BAR})")
    assert err <= HIDDEN_BAR, (name, err, per_row)
    assert cos <= COS_BAR and (not cls or cos_cls <= COS_BAR), (name, cos)
    return err


@pytest.mark.parametrize("bm,heads", DEBERTA_PARAMS, ids=DEBERTA_IDS)
def test_deberta_parity_at_the_edges(bm, heads):
    """the long batch (12 lengths on the remainders of the 128-key kchunk, up to 512 = max_pos) right-padded, left-padded and with holes; the short batches for
    each HPB right- and left-padded; B = 3 at S = 1 (W = 32), one sequence of 127 / 128 / 129 rows (the k_pos_scores block) and the width of W = 96: element-wise
    and mean-pooled everywhere, CLS-pooled on the right-padded batches"""
    c, w, h, m = _deberta(bm, heads)
    tag = f"Bk {bm[0]} M {bm[1]} heads {heads}"
    worst = 0.0
    L, S = A.DEBERTA_LONG, A.DEBERTA_LONG_S
    worst = max(worst, _deberta_parity(h, m, "long right", *A.deberta_batch(L, S, "right", heads), True, tag))
    worst = max(worst, _deberta_parity(h, m, "long left", *A.deberta_batch(L, S, "left", heads), False, tag))
    worst = max(worst, _deberta_parity(h, m, "long holes", *A.deberta_batch(L, S, "right", heads, holes=True), False, tag))
    for Ss, lens in A.SHORT.items():
        worst = max(worst, _deberta_parity(h, m, f"short {Ss} right", *A.deberta_batch(lens, Ss, "right", Ss + heads), True, tag))
        worst = max(worst, _deberta_parity(h, m, f"short {Ss} left", *A.deberta_batch(lens, Ss, "left", Ss + heads), False, tag))
    for B, Se in A.deberta_extras(*bm):
        assert A.pos_span(Se, *bm)[1] in (32, 96) or B * Se in (A.POS_ROWS - 1, A.POS_ROWS, A.POS_ROWS + 1)
        worst = max(worst, _deberta_parity(h, m, f"extra {B} x {Se} (W {A.pos_span(Se, *bm)[1]})", *A.deberta_batch([Se] * B, Se, "right", 100 + Se), True, tag))
    h.check()
    _note(f"[{tag}] disentangled attention at the edge lengths vs HF fp32: worst {worst:.2e} (bar {HIDDEN_BAR})")


@pytest.mark.parametrize("bm,heads", DEBERTA_PARAMS, ids=DEBERTA_IDS)
def test_deberta_rows_do_not_depend_on_the_shift(bm, heads):
    """only column differences enter: the rows of every sequence of the long batch and of the short batches are the same bits left-padded and right-padded"""
    c, w, h, m = _deberta(bm, heads)
    for lens, S in [(A.DEBERTA_LONG, A.DEBERTA_LONG_S)] + [(lens, Ss) for Ss, lens in A.SHORT.items()]:
        ids, mask = A.deberta_batch(lens, S, "right", 3)
        out, hid = _run(h, ids, mask)
        lout, lhid = _run(h, *A.shifted(ids, mask))
        assert _same(lout, out), S
        for r, n in enumerate(lens):
            assert _same(lhid[r, S - n:], hid[r, :n]), (S, n)


@pytest.mark.parametrize("bm,heads", [(A.DEBERTA_SHAPES[0], 2), (A.DEBERTA_SHAPES[1], 4)], ids=["Bk256-heads2", "Bk32-heads4"])
def test_deberta_position_scores_buffer_across_widths(bm, heads):
    """one fresh handle: S = 1 (W = 32), then S = 512 (the whole table: the buffer grows), then S = 1 again in the larger buffer — the same bits, and the
    S = 512 rows in between are those of a handle that never ran another width"""
    c, w, h0, m = _deberta(bm, heads)
    h = _handle(c, w)
    one = A.deberta_batch([1, 1, 1], 1, "right", 5)
    wide = A.deberta_batch(A.DEBERTA_LONG, A.DEBERTA_LONG_S, "right", 6)
    assert A.pos_span(1, *bm)[1] == 32 and A.pos_span(A.DEBERTA_LONG_S, *bm)[1] == 2 * bm[0]
    first = _run(h, *one)
    assert np.isfinite(first[0]).all()
    middle = _run(h, *wide)
    again = _run(h, *one)
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    ref = _run(h0, *wide)
    assert _same(middle[0], ref[0]) and _same(middle[1], ref[1])
    h.check()


# ---------------------------------------------------------------------------------------------------------
# ModernBert's window on the same lengths (k_attn_dma: the ring of a second q-group starts at chunk c_lo = 3)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [2, 4])
def test_window_parity_at_the_edges(heads):
    """global / local / local layers, half-window 64, the 12 lengths of the DeBERTa list in one 512-wide batch, right-padded, left-padded and with 5 holes per
    row (gathered key columns): last_hidden_state within 3e-2 of HF fp32 on attended rows, mean-pooled embeddings within 1 - cos <= 5e-5.  (The window's edge
    decides rows of every one of these sequences: tests/test_attention_edges_host.py.)"""
    cfg, w = A.modernbert_model(heads)
    h = _handle(cfg, w)
    m = MB.hf_model(cfg, w)
    worst = 0.0
    right = A.modernbert_batch(A.DEBERTA_LONG, A.DEBERTA_LONG_S, "right")
    for name, (ids, mask) in (("right", right), ("left", A.shifted(*right)), ("holes", A.with_holes(*right, 5, 9))):
        keep = mask.astype(bool)
        ref = MB.hf_last_hidden(m, ids, mask)
        out, lh = _run(h, ids, mask)
        err = float(np.abs(lh - ref)[keep].max())
        per_row = [float(np.abs(lh[r] - ref[r])[keep[r]].max()) for r in range(len(ids))]
        cos = _cos_gap(out, MB.pool_np(ref, mask, POOL_MEAN))
        worst = max(worst, err)
        _note(f"[modernbert heads {heads}] long {name}: max |last_hidden - HF| {err:.2e} (bar {HIDDEN_BAR}; worst row: {int(mask[int(np.argmax(per_row))].sum())} keys), "
              f"1 - cos mean {cos:.2e} (bar {COS_BAR})")
        assert np.isfinite(lh).all() and not lh[~keep].any(), name
        assert err <= HIDDEN_BAR, (name, err, per_row)
        assert cos <= COS_BAR, (name, cos)
    h.check()
    _note(f"[modernbert heads {heads}] window of 64 at the edge lengths vs HF fp32 eager: worst {worst:.2e} (bar {HIDDEN_BAR})")


# ---------------------------------------------------------------------------------------------------------
# 5. one arithmetic at every edge length, all four non-plain modes
# ---------------------------------------------------------------------------------------------------------
def _mode(name, heads):
    """(config, weights, lengths, width, batch builder, pools): the builder makes right-padded rows of the family's token rule"""
    if name == "causal":
        kind = {2: "llama-64", 4: "qwen2-32"}[heads]
        cfg = DC.hf_config(kind, 2, max_pos=A.DECODER_LONG_S)
        return cfg, DC.weights(cfg), A.DECODER_IDENTITY, A.DECODER_LONG_S, lambda lens, S: A.decoder_batch(lens, S, "R", 51), (POOL_MEAN, POOL_LAST)
    if name == "disentangled":
        c = DB.cfg(heads=heads, Bk=256, M=512)
        return c, DB.weights(c), A.DEBERTA_LONG, A.DEBERTA_LONG_S, lambda lens, S: A.deberta_batch(lens, S, "right", 52), (POOL_MEAN, POOL_CLS)
    if name == "window":
        cfg, w = A.modernbert_model(heads)
        return cfg, w, A.DEBERTA_LONG, A.DEBERTA_LONG_S, lambda lens, S: A.modernbert_batch(lens, S, "right"), (POOL_MEAN, POOL_CLS)
    cfg, w = _t5(heads)
    return cfg, w, A.DEBERTA_LONG, A.DEBERTA_LONG_S, lambda lens, S: A.ragged(lens, S, "right", 54, 2, 1000), (POOL_MEAN,)


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("mode", ["causal", "disentangled", "window", "bias"])
def test_one_arithmetic_at_every_edge_length(mode, heads, monkeypatch):
    """The mode's long batch once, then bit for bit on last_hidden and the pooled rows: (a) each sequence alone at its own width (a length <= 128 thereby runs
    k_attn_lds with its own HPB, its rows in the batch k_attn_dma) == its rows in the batch; (b) the reversed batch; (c) kr_encoder_forward_packed; (d) except
    for DeBERTa (which runs k_attn_lds anyway) KIRAG_AMD_ATTN_LDS=1: k_attn_lds == k_attn_dma at every length above 128 — they stage K and V differently and
    must run the same steps by AttnBand; (e) a handle created under KIRAG_AMD_ATTN_BIAS_GATHER=1: consecutive == gathered key columns."""
    monkeypatch.delenv("KIRAG_AMD_ATTN_LDS", raising=False)
    cfg, w, lens, S, build, pools = _mode(mode, heads)
    h = _handle(cfg, w)
    ids, mask = build(lens, S)
    assert mask.sum(1).tolist() == list(lens)
    out, lh = _run(h, ids, mask)
    assert np.isfinite(out).all() and np.isfinite(lh).all() and np.ptp(out, axis=0).min() > 0
    other = {p: h.forward_np(ids, mask, p) for p in pools[1:]}
    # (a)
    for r, n in enumerate(lens):
        o1, l1 = _run(h, ids[r:r + 1, :n].copy(), mask[r:r + 1, :n].copy())
        assert _same(o1[0], out[r]) and _same(l1[0], lh[r, :n]), (mode, "alone", n)
    # (b)
    o2, l2 = _run(h, ids[::-1].copy(), mask[::-1].copy())
    assert _same(o2[::-1], out) and _same(l2[::-1], lh), (mode, "reversed")
    # (c)
    rag, rl = _rag(ids, mask)
    assert _same(h.forward_packed(rag, rl, S, POOL_MEAN).cpu().numpy(), out), (mode, "packed")
    assert _same(h.last_hidden(len(ids), S).numpy(), lh), (mode, "packed rows")
    for p, want in other.items():
        assert _same(h.forward_packed(rag, rl, S, p).cpu().numpy(), want), (mode, "packed", p)
    # (d)
    if mode != "disentangled":
        monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
        o4, l4 = _run(h, ids, mask)
        bad = [n for r, n in enumerate(lens) if not _same(l4[r], lh[r])]
        assert not bad and _same(o4, out), (mode, "k_attn_lds vs k_attn_dma", bad)
        for p, want in other.items():
            assert _same(h.forward_np(ids, mask, p), want), (mode, "k_attn_lds", p)
        monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
    # (e)
    hg = _handle(cfg, w, gather=True)
    o5, l5 = _run(hg, ids, mask)
    bad = [n for r, n in enumerate(lens) if not _same(l5[r], lh[r])]
    assert not bad and _same(o5, out), (mode, "gathered key columns", bad)
    for p, want in other.items():
        assert _same(hg.forward_np(ids, mask, p), want), (mode, "gathered", p)
    h.check(); hg.check()
