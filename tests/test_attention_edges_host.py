"""Host half of the attention edge tests (tests/test_gpu_attention_edges.py): no GPU, no library call.  (1) The length lists of attention_edges_util are the
ones the kernels' geometry asks for: every boundary class of k_attn_dma's causal mode, of k_attn_lds's multi-chunk loop, of the HPB choice and of k_pos_scores
is represented.  (2) The precondition of the parity tests, on the references alone: hiding one CLASS of keys (packed index 63 / 0 / 31 / 32 mod 64; DeBERTa also
127 / 0 mod 128 and the last key of every sequence) from every other query moves some attended row of the long batch by >= 10 x the 3e-2 bar — the keys at
the edges decide rows, so a kernel that dropped or doubled one could not stay inside the bar.  For the decoder the condition is on rows of column >= 256: the
rows only the new lengths reach."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_edges_util as A  # noqa: E402
import deberta_util as DB  # noqa: E402
import decoder_util as DC  # noqa: E402

HIDDEN_BAR = 3e-2


# ---------------------------------------------------------------------------------------------------------
# 1. the lists
# ---------------------------------------------------------------------------------------------------------
def test_the_lists_are_the_ones_the_geometry_asks_for():
    assert (A.Q_TILE, A.KEY_STEP, A.KCHUNK, A.Q_GROUP, A.POS_ROWS) == (32, 64, 128, 256, 128)
    assert A.DECODER_LONG_S == 1024 and A.DECODER_LONG == [160, 192, 193, 256, 257, 288, 289, 320, 384, 385, 511, 512, 513, 576, 640, 1000, 1024]
    assert A.DEBERTA_LONG_S == 512 and A.DEBERTA_LONG == [129, 160, 192, 193, 224, 256, 257, 288, 320, 384, 511, 512]
    assert A.SHORT == {32: [1, 2, 31, 32], 64: [33, 63, 64], 128: [65, 95, 96, 97, 127, 128]}
    assert A.DECODER_IDENTITY == [n for n in A.DECODER_LONG if n <= 513] + [1000]
    assert A.CAUSAL_COLUMNS == (255, 256, 257, 511, 512, 767, 1023)
    assert A.DECODER_KINDS == ("qwen2-32", "llama-64") and A.DEBERTA_SHAPES == ((256, 512), (32, 128)) and A.DEBERTA_HEADS == (2, 4)
    for S, lens in A.SHORT.items():
        assert max(lens) == S and min(lens) >= 1
    assert max(A.DECODER_LONG) == A.DECODER_LONG_S and max(A.DEBERTA_LONG) == A.DEBERTA_LONG_S
    assert min(A.DECODER_LONG) > A.LDS_MAX and min(A.DEBERTA_LONG) > A.KCHUNK      # every long length: k_attn_dma / the multi-chunk loop


def test_every_boundary_of_the_causal_ring_is_represented():
    """each class of decoder_classes by some length of the long batch, the named ones by the length the list gives for them; the bit-identity subset keeps
    every class but the fourth q-group's full ring (1024, which the parity and causality tests run)"""
    by = {n: A.decoder_classes(n) for n in A.DECODER_LONG}
    for cls in A.DECODER_CLASSES:
        assert any(cls in c for c in by.values()), cls
        assert any(cls in by[n] for n in A.DECODER_IDENTITY), cls
    assert all("last chunk of exactly 32 keys" in by[n] for n in (160, 288)) and "a partial last chunk of 32 keys in a q-group >= 1" in by[288]
    assert all("no partial chunk" in by[n] for n in (192, 320))
    assert "a q-group of one query whose last chunk holds one key" in by[257]
    assert "first length with two tiles per wave in q-group 1" in by[385] and "two tiles per wave in a q-group >= 1" not in by[384]
    assert "three q-groups" in by[513] and "three q-groups" not in by[512]
    assert all("four q-groups" in by[n] and "the ring wraps with a clipped nchunks" in by[n] for n in (1000, 1024))
    # the geometry behind the names, at 1000 tokens: q-group g streams chunks [0, 4 g + 4) of 16, the last group all of them with a partial chunk of 40 keys
    g = A.dma_groups(1000, 1024, 0)
    assert [x["nchunks"] for x in g] == [4, 8, 12, 16] and [x["nfull"] for x in g] == [4, 8, 12, 15] and all(x["c_lo"] == 0 for x in g)
    assert [x["tiles"] for x in g] == [8, 8, 8, 8] and all(x["two"] for x in g) and 1000 - 3 * A.Q_GROUP - 7 * A.Q_TILE == 8      # the last tile: 8 queries
    # 257: the block of q-group 1 holds one query; its ring has 5 chunks, the last of one key, and no wave has a second tile
    g = A.dma_groups(257, 1024, 0)
    assert (g[1]["nchunks"], g[1]["nfull"], g[1]["tiles"], g[1]["two"]) == (5, 4, 1, False) and (g[0]["nchunks"], g[0]["nfull"]) == (4, 4)
    # what the merged tests reached: one sequence of 300 never has a two-tile wave in q-group 1
    assert not A.dma_groups(300, 1024, 0)[1]["two"]


def test_the_causal_band_visits_exactly_the_steps_that_hold_an_admitted_key():
    """the restated AttnBand against brute force: a tile visits a 64-key step iff some (query, key) pair of it is admitted, for every tile of every length"""
    for n in A.DECODER_LONG + sum(A.SHORT.values(), []):
        for q0 in range(0, n, A.Q_TILE):
            b = A.band(q0, q0 + A.Q_TILE - 1, n, 1024, 0)
            for kb in range(0, n, A.KEY_STEP):
                want = kb <= min(q0 + A.Q_TILE - 1, n - 1)             # the step's first key is at or below the tile's last query
                assert A.visits(b, kb) == want, (n, q0, kb)


def test_what_the_band_clamp_does_not_decide():
    """The min(q1, nk - 1) of attn_band changes no visited step (every step starts below nk) and no ring length (nchunks is clipped to the sequence's chunks):
    a build without it computes the same rows, so no test is owed for it.  Its `+ wr` does decide: without it the tile of queries 32 .. 63 of every
    windowed sequence loses the step of keys 64 .. 127."""
    for n in A.DECODER_LONG + A.DEBERTA_LONG + sum(A.SHORT.values(), []):
        for wl, wr in ((1024, 0), (A.WINDOW, A.WINDOW)):
            chunks = (n + A.KEY_STEP - 1) // A.KEY_STEP
            for q0 in range(0, n, A.Q_TILE):
                b, loose = A.band(q0, q0 + A.Q_TILE - 1, n, wl, wr), (max(q0 - wl, 0), q0 + A.Q_TILE - 1 + wr)
                assert all(A.visits(b, kb) == A.visits(loose, kb) for kb in range(0, n, A.KEY_STEP)), (n, q0)
            for g in range(0, n, A.Q_GROUP):
                assert min(chunks, A.band(g, g + A.Q_GROUP - 1, n, wl, wr)[1] // A.KEY_STEP + 1) == min(chunks, (g + A.Q_GROUP - 1 + wr) // A.KEY_STEP + 1)
    for n in A.DEBERTA_LONG:
        b = A.band(32, 63, n, A.WINDOW, A.WINDOW)
        assert A.visits(b, 64) and not A.visits((b[0], b[1] - A.WINDOW), 64)


def test_every_boundary_of_the_register_staged_kernel_is_represented():
    by = {n: A.lds_classes(n) for n in A.DEBERTA_LONG}
    for cls in A.LDS_CLASSES:
        assert any(cls in c for c in by.values()), cls
    assert "kchunk remainder 0" in by[256] and "kchunk remainder 1" in by[129] and "kchunk remainder 1" in by[257]
    assert "kchunk remainder 32" in by[160] and "kchunk remainder 64" in by[192]
    assert A.last_step_mode(160) == 2 and A.last_step_mode(129) == 1 and A.last_step_mode(192) == 0 and A.last_step_mode(511) == 3
    # the short batches: each HPB instantiation, and on each side of every q-tile count boundary a length
    assert [A.hpb(S) for S in sorted(A.SHORT)] == [4, 2, 1]
    short = sorted(sum(A.SHORT.values(), []))
    for edge in (32, 64, 128):
        assert edge - 1 in short and edge in short and (edge + 1 in short or edge + 1 in A.DEBERTA_LONG), edge
    # ... and every MODE of a last step in each of them (a width of 32 has no step of more than 32 keys)
    for S, lens in A.SHORT.items():
        modes = {A.last_step_mode(n, min(S, A.KCHUNK)) for n in lens}
        assert modes == ({1, 2} if S == 32 else {0, 3} if S == 64 else {0, 1, 2, 3}), (S, modes)


def test_every_boundary_of_the_windowed_ring_is_represented():
    """ModernBert's half-window 64 on the DeBERTa list: a second q-group starts its ring at chunk (256 - 64) / 64 = 3, with every kind of last chunk; the first
    q-group of a long sequence is clipped at (255 + 64) / 64 + 1 = 5 chunks"""
    by = {n: A.window_classes(n) for n in A.DEBERTA_LONG}
    for cls in A.WINDOW_CLASSES:
        assert any(cls in c for c in by.values()), cls
    g = A.dma_groups(512, A.WINDOW, A.WINDOW)
    assert [(x["c_lo"], x["nchunks"]) for x in g] == [(0, 5), (3, 8)]
    assert "c_lo > 0, a last chunk of one key" in by[257] and "c_lo > 0, a last chunk of 32 keys" in by[288] and "c_lo > 0, no partial chunk" in by[320]
    # brute force: a tile visits a step iff a (query, key) pair of it lies inside the window (consecutive columns: packed index == column difference)
    for n in A.DEBERTA_LONG:
        for q0 in range(0, n, A.Q_TILE):
            b = A.band(q0, q0 + A.Q_TILE - 1, n, A.WINDOW, A.WINDOW)
            for kb in range(0, n, A.KEY_STEP):
                q = np.arange(q0, min(q0 + A.Q_TILE, n))[:, None]; k = np.arange(kb, min(kb + A.KEY_STEP, n))[None]
                assert A.visits(b, kb) == bool((np.abs(q - k) <= A.WINDOW).any()), (n, q0, kb)


def _bucket(r, Bk, M):
    """deberta_bucket restated in float64: linear up to Bk / 2, then logarithmic up to M - 1, clamped into the table"""
    mid = Bk // 2
    a = abs(r)
    if a <= mid:
        d = r
    else:
        d = int(math.copysign(math.ceil(math.log(a / mid) / math.log((M - 1) / mid) * (mid - 1)) + mid, r))
    return min(max(d + Bk, 0), 2 * Bk - 1)


def _span(S, Bk, M):
    lo, hi = _bucket(-(S - 1), Bk, M), _bucket(S - 1, Bk, M)
    p0 = lo & ~31
    return p0, (hi + 1 - p0 + 31) // 32 * 32


@pytest.mark.parametrize("Bk,M", A.DEBERTA_SHAPES)
def test_the_position_score_widths(Bk, M):
    """pos_span restated twice (HF's bucket rule in the util, the closed form here) agrees at every width; S = 1 is the only width of W = 32; the extras hold
    W = 32, T = 127 / 128 / 129 and, for the 512-row table, the one width of W = 96 (the 64-row table never spans 96); the long batch spans the whole table"""
    for S in (1, 2, 3, 17, 31, 32, 33, 34, 63, 64, 65, 96, 97, 127, 128, 129, 130, 255, 256, 257, 300, 511, 512):
        assert A.pos_span(S, Bk, M) == _span(S, Bk, M), S
    assert A.widths_with_span(32, Bk, M) == [1]
    extras = A.deberta_extras(Bk, M)
    assert extras[:4] == [(3, 1), (1, 127), (1, 128), (1, 129)]
    assert {B * S for B, S in extras[1:4]} == {A.POS_ROWS - 1, A.POS_ROWS, A.POS_ROWS + 1}
    w96 = A.widths_with_span(96, Bk, M)
    if Bk == 256:
        assert w96 == [33] and extras[4] == (1, 33) and _span(33, Bk, M) == (224, 96) and 96 % A.POS_CHUNK == A.POS_CHUNK // 2
    else:
        assert w96 == [] and len(extras) == 4 and 2 * Bk < 96
    p0, W = _span(A.DEBERTA_LONG_S, Bk, M)
    assert (p0, W) == (0, 2 * Bk)
    # a width of every parity of W / 64: whole chunks and a half chunk at the end
    spans = {_span(S, Bk, M)[1] for S in list(A.SHORT) + [A.DEBERTA_LONG_S] + [s for _, s in extras]}
    assert any(w % A.POS_CHUNK == 0 for w in spans) and any(w % A.POS_CHUNK == 32 for w in spans)


def test_the_batches_hold_their_lengths():
    ids, mask = A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "R", 1)
    assert mask.sum(1).tolist() == A.DECODER_LONG and (mask[:, 0] == 1).all() and ((ids != 0) == (mask != 0)).all()
    il, ml = A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "L", 1)
    assert ml.sum(1).tolist() == A.DECODER_LONG and (ml[:, -1] == 1).all()
    ih, mh = A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "R", 1, holes=5)
    assert mh.sum(1).tolist() == [n - 5 for n in A.DECODER_LONG] and (DC.last_index(mh) == np.array(A.DECODER_LONG) - 1).all()
    ids, mask = A.deberta_batch(A.DEBERTA_LONG, A.DEBERTA_LONG_S, "right", 2)
    assert mask.sum(1).tolist() == A.DEBERTA_LONG and (ids[:, 0] == DB.CLS_ID).all()
    i2, m2 = A.shifted(ids, mask)
    for r, n in enumerate(A.DEBERTA_LONG):
        assert (i2[r, 512 - n:] == ids[r, :n]).all() and m2[r].sum() == n and (m2[r, :512 - n] == 0).all()
    ih, mh = A.deberta_batch(A.DEBERTA_LONG, A.DEBERTA_LONG_S, "right", 2, holes=True)
    assert (mh[:, 0] == 1).all() and (mh.sum(1) < mask.sum(1)).all() and (mh <= mask).all()
    hide = A.hidden_keys(mh, None)
    assert hide.sum(1).tolist() == [1] * len(ih) and (np.argmax(hide, 1) == np.array(A.DEBERTA_LONG) - 1).all()
    hide = A.hidden_keys(mask, (63, 64))
    assert hide[0].nonzero()[0].tolist() == [63, 127] and hide[-1].sum() == 8


# ---------------------------------------------------------------------------------------------------------
# 2. the preconditions, on the references alone
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", A.DECODER_KINDS)
def test_the_keys_at_the_edges_decide_decoder_rows(kind):
    """the long batch, right-padded (packed index == column): the hand-made causal 4-D mask gives HF's own rows exactly, and each class of hidden keys moves a
    row of column >= 256 by >= 0.3"""
    cfg = DC.hf_config(kind, 2, max_pos=A.DECODER_LONG_S)
    m = DC.hf_model(cfg, DC.weights(cfg))
    ids, mask = A.decoder_batch(A.DECODER_LONG, A.DECODER_LONG_S, "R", 31)
    ref = A.decoder_hidden(m, ids, mask)
    own = DC.hf_last_hidden(m, ids, mask, chunk=6)
    assert float(np.abs(own - ref)[mask != 0].max()) == 0.0
    rows = np.broadcast_to(np.arange(A.DECODER_LONG_S)[None] >= A.Q_GROUP, mask.shape)
    d = A.class_distances(ref, lambda hide: A.decoder_hidden(m, ids, mask, hide), mask, A.KEY_CLASSES, rows)
    print(f"[{kind}] rows >= {A.Q_GROUP}: " + ", ".join(f"{k} {v:.2f}" for k, v in d.items()))
    for name, v in d.items():
        assert v >= 10 * HIDDEN_BAR, ("precondition", kind, name, v)


@pytest.mark.parametrize("heads", A.DEBERTA_HEADS)
@pytest.mark.parametrize("Bk,M", A.DEBERTA_SHAPES)
def test_the_keys_at_the_edges_decide_deberta_rows(Bk, M, heads):
    """the long batch, right-padded: the model's embeddings + encoder under the full 3-D mask give the 2-D path's rows exactly, and each class of hidden keys —
    the last key of every sequence among them, which only the clamp of the gathered bias tile to nk - 1 protects — moves an attended row by >= 0.3"""
    c = DB.cfg(heads=heads, Bk=Bk, M=M)
    m = DB.hf_model(c, DB.weights(c))
    ids, mask = A.deberta_batch(A.DEBERTA_LONG, A.DEBERTA_LONG_S, "right", heads)
    ref = A.deberta_hidden(m, ids, mask)
    assert float(np.abs(DB.hf_hidden(m, ids, mask) - ref)[mask != 0].max()) == 0.0
    d = A.class_distances(ref, lambda hide: A.deberta_hidden(m, ids, mask, hide), mask, A.DEBERTA_KEY_CLASSES)
    print(f"[Bk {Bk} M {M} heads {heads}] " + ", ".join(f"{k} {v:.2f}" for k, v in d.items()))
    for name, v in d.items():
        assert v >= 10 * HIDDEN_BAR, ("precondition", Bk, M, heads, name, v)


@pytest.mark.parametrize("heads", [2, 4])
def test_the_window_edge_decides_rows_of_every_sequence(heads):
    """ModernBert (global / local / local, half-window 64) on the DeBERTa list: no window, a window one narrower and one wider each move an attended row of
    EVERY sequence by >= 0.3 — on the CPU, from HF alone"""
    import modernbert_util as MB
    cfg, w = A.modernbert_model(heads)
    m = MB.hf_model(cfg, w, "cpu")
    ids, mask = A.modernbert_batch(A.DEBERTA_LONG, A.DEBERTA_LONG_S, "right")
    ref = MB.hf_last_hidden(m, ids, mask)
    for how in MB.WINDOW_BREAKS:
        with MB.broken(m, how):
            other = MB.hf_last_hidden(m, ids, mask)
        d = [float(np.abs(ref[r] - other[r])[mask[r] != 0].max()) for r in range(len(ids))]
        print(f"[heads {heads}] {how}: weakest sequence {min(d):.2f}")
        assert min(d) >= 10 * HIDDEN_BAR, ("precondition", heads, how, d)
