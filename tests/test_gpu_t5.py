"""GPU tests of T5 encoder checkpoints (sentence-transformers/gtr-t5-*, sentence-t5-*, hkunlp/instructor-*: T5EncoderModel = a pre-LN stack with RMS norms, the
embedding row straight into the residual stream, one learned bias per (head, bucket of the column distance) added to the UNSCALED scores of every layer, no
linear bias, a relu or a gated gelu_new feed-forward, and optionally the sentence-transformers Dense head behind the pooling).  The reference is
transformers.T5EncoderModel in fp32 with eager attention on synthetic weights (t5_util.weights: last_hidden_state of rms 1.0, max |x| 4.5 - 6).  Every part of
the family is tested where it has teeth: on last_hidden_state, element-wise, with the distance to a reference that lacks the part asserted as a precondition.

Bars: HIDDEN_BAR 3e-2 element-wise on attended rows, set for LayerNorm outputs of |x| <= ~4; an element whose reference is larger is
held to 3e-2 * |ref| / 4 (the same relative error), and both figures are printed.  COS_BAR 5e-5 / SCORE_BAR 1e-3 on embeddings.

What no test here can see through a 16-bit forward: gelu_new against erf-GELU in the gated feed-forward moves the reference's rows by 6e-4 - 9e-4, far under
any bar.  That the epilogue computes the tanh form is checked by reading (encoder_proj.hpp: gelu_tanh_mul)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpnet_util as M  # noqa: E402
import t5_util as T  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL = -22
COS_BAR, SCORE_BAR = 5e-5, 1e-3
HIDDEN_BAR = 3e-2
L, FF, VOCAB = 3, 1024, 1000
KINDS = [(64, T.RELU), (64, T.GATED), (32, T.RELU), (32, T.GATED)]


def _hip(cfg, w, **kw):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(cfg, 0, **kw)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _model(dh, ff, **kw):
    H, heads = T.WIDTHS[dh]
    return T.cfg(H, L, heads, FF, VOCAB, ff), T.weights(H, L, heads, FF, VOCAB, ff, **kw)


def _hidden_check(lh, ref, keep, what):
    """every attended element within HIDDEN_BAR * max(1, |ref| / 4); returns (worst error, worst error among |ref| <= 4)"""
    err = np.abs(lh - ref)[keep]
    mag = np.abs(ref)[keep]
    small = float(err[mag <= 4].max())
    worst = float(err.max())
    if worst > HIDDEN_BAR:
        print(f"{what}: worst {worst:.2e} at |ref| {float(mag[err.argmax()]):.2f}; worst among |ref| <= 4: {small:.2e}")
    assert np.isfinite(lh[keep]).all() and (err <= HIDDEN_BAR * np.maximum(1.0, mag / 4)).all(), (what, worst, small)
    return worst, small


def _min_move(ref, other, keep):
    """the smallest, over the sequences, of the largest move of an attended element"""
    return min(float(np.abs(ref[r] - other[r])[keep[r]].max()) for r in range(len(ref)))


@pytest.mark.parametrize("dh,ff", KINDS)
def test_last_hidden_state_parity_where_every_part_has_teeth(dh, ff, monkeypatch):
    """kr_encoder_last_hidden against HF's last_hidden_state on attended rows: right-padded, left-padded, full-length and ragged (forward_packed, bit-identical)
    batches at S = 32, 128 (k_attn_lds), 200, 512 (k_attn_dma), both pools (CLS with a masked column 0: the extra query row).  Preconditions per sequence, on
    the reference, each >= 10 x the bar: the table zeroed, the distance mirrored, q divided by sqrt(d_h), and the feed-forward broken (relu -> erf-GELU, or
    wi_0 and wi_1 exchanged)."""
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")          # read at handle creation: every row of the last layer is kept under CLS pooling too
    cfg, w = _model(dh, ff)
    h, m = _hip(cfg, w), T.hf_model(cfg, w)
    assert h.is_t5 and h.out_dim == cfg.d_model
    W = w[T.BIAS_NAME]
    ff_break = "erf_gelu" if ff == T.RELU else "wi_exchanged"
    worst, worst_small, weakest = 0.0, 0.0, {}
    for S in (32, 128, 200, 512):
        for layout in ("R", "L", "F"):
            B = 3 if S >= 200 else 5
            ids, mask = T.tokens(B, S, layout, 1000 + S + ord(layout), VOCAB)
            keep = mask.astype(bool)
            ref = T.hf_last_hidden(m, ids, mask)
            moves = {}
            T.set_bias(m, 0 * W); moves["table zeroed"] = _min_move(ref, T.hf_last_hidden(m, ids, mask), keep)
            T.set_bias(m, M.mirrored(W)); moves["distance mirrored"] = _min_move(ref, T.hf_last_hidden(m, ids, mask), keep)
            T.set_bias(m, W)
            for how in ("q_scaled", ff_break):
                with T.broken(m, how):
                    moves[how] = _min_move(ref, T.hf_last_hidden(m, ids, mask), keep)
            for k, v in moves.items():
                weakest[k] = min(weakest.get(k, np.inf), v)
                assert v >= 10 * HIDDEN_BAR, ("precondition", k, S, layout, v)
            for pool in (0, 1):
                out = h.forward_np(ids, mask, pool)
                assert out.shape == (B, cfg.d_model)
                lh = h.last_hidden(B, S).numpy()
                a, b = _hidden_check(lh, ref, keep, f"[d_h {dh} {ff}] S {S} {layout} pool {pool}")
                worst, worst_small = max(worst, a), max(worst_small, b)
                if pool == 1 and layout == "L":
                    # the CLS row of a sequence whose column 0 is masked: a query-only row with column 0
                    col0 = np.zeros_like(keep); col0[:, 0] = True
                    assert (mask[:, 0] == 0).any()
                    _hidden_check(lh, ref, col0, f"[d_h {dh} {ff}] S {S} L cls rows")
                if layout == "R":
                    rag, lens = _rag(ids, mask)
                    h.forward_packed(rag, lens, S, pool)
                    assert _same(h.last_hidden(B, S).numpy()[keep], lh[keep]), (S, pool)
    print(f"[d_h {dh} {ff}] worst |last_hidden - HF| {worst:.2e}, among |ref| <= 4 {worst_small:.2e} (bar {HIDDEN_BAR}); weakest preconditions "
          + ", ".join(f"{k} {v:.2f}" for k, v in weakest.items()))


@pytest.mark.parametrize("dh,ff", KINDS)
def test_rms_norm_against_layer_norm(dh, ff):
    """Embeddings with +1.0 added to every entry: rows have a common offset that only a mean-subtracting norm removes.  Precondition: T5LayerNorm replaced by
    a mean-subtracting norm moves the reference by >= 10 x the bar (with zero-mean embeddings the same exchange moves it by only 0.2 - 0.5); then parity."""
    cfg, w = _model(dh, ff, offset=1.0)
    h, m = _hip(cfg, w), T.hf_model(cfg, w)
    for S, layout in ((32, "R"), (200, "L")):
        B = 3
        ids, mask = T.tokens(B, S, layout, 7 + S, VOCAB)
        keep = mask.astype(bool)
        ref = T.hf_last_hidden(m, ids, mask)
        with T.broken(m, "layer_norm"):
            move = _min_move(ref, T.hf_last_hidden(m, ids, mask), keep)
        assert move >= 10 * HIDDEN_BAR, ("precondition", S, move)
        h.forward_np(ids, mask, 0)
        worst, small = _hidden_check(h.last_hidden(B, S).numpy(), ref, keep, f"[d_h {dh} {ff}] offset embeddings S {S}")
        print(f"[d_h {dh} {ff}] S {S}: mean-subtracting norm moves the reference by {move:.2f}; worst |last_hidden - HF| {worst:.2e} ({small:.2e} among |ref| <= 4)")


INSIDE = {8: 11, 12: 15, 16: 22, 23: 31, 32: 45, 46: 63, 64: 90}     # boundary -> the last distance of its bucket


@pytest.mark.parametrize("dh", [64, 32])
def test_every_bucket_boundary_and_the_distance_as_a_column_difference(dh):
    """Sequences of S = 256 with two attended columns c0 < c1: T5 has no position input, so only the bias sees c1 - c0.  Table 2 (-1)^b (b < 16) / -2 (-1)^b
    (b >= 16).  Across every boundary n0 the rows for distances n0 - 1 and n0 each match HF and differ from each other, in the reference, by >= 10 x the bar; two
    distances inside one bucket give bit-identical rows."""
    S = 256
    H, heads = T.WIDTHS[dh]
    cfg, w = _model(dh, T.RELU, bias=M.boundary_table(heads))
    h, m = _hip(cfg, w), T.hf_model(cfg, w)
    weakest, worst = np.inf, 0.0
    for c0 in (0, 37, 120):
        dist = sorted({n for n0 in (2, 3, 4, 5, 6, 7) + M.BOUNDARIES for n in (n0 - 1, n0)} | set(INSIDE.values()) | {219 - c0})
        assert c0 + max(dist) < S
        ids = np.zeros((len(dist), S), np.int64); mask = np.zeros((len(dist), S), np.int64)
        for r, n in enumerate(dist):
            ids[r, c0], ids[r, c0 + n] = 5, 7
            mask[r, c0] = mask[r, c0 + n] = 1
        ref = T.hf_last_hidden(m, ids, mask)
        h.forward_np(ids, mask, 0)
        lh = h.last_hidden(len(dist), S).numpy()
        rows = {n: (lh[r, [c0, c0 + n]], ref[r, [c0, c0 + n]]) for r, n in enumerate(dist)}
        for n, (got, exp) in rows.items():
            a, _ = _hidden_check(got, exp, np.ones(got.shape, bool), f"[d_h {dh}] c0 {c0} distance {n}")
            worst = max(worst, a)
        for n0 in (2, 3, 4, 5, 6, 7) + M.BOUNDARIES:
            assert M.bucket(n0 - 1) != M.bucket(n0)
            sep = np.abs(rows[n0 - 1][1] - rows[n0][1]).max(axis=1)          # per row (the token at c0, the token at c1), in the reference
            weakest = min(weakest, float(sep.min()))
            assert (sep >= 10 * HIDDEN_BAR).all(), ("precondition", c0, n0, sep)
        for n0, n1 in list(INSIDE.items()) + [(91, 219 - c0)]:
            assert M.bucket(n0) == M.bucket(n1) and n0 != n1
            assert _same(rows[n0][0], rows[n1][0]), (c0, n0, n1)
    print(f"[d_h {dh}] worst |row - HF| {worst:.2e}; smallest separation across a boundary {weakest:.2f}")


@pytest.mark.parametrize("dh,P,ff", [(64, 512, T.RELU), (32, 768, T.GATED), (64, 768, T.GATED)])
def test_dense_head(dh, P, ff):
    """out [B, P] = normalize(W . pooled) through forward_np, forward and forward_packed, against normalize(W . pool(HF last_hidden)) in float64 at COS_BAR,
    scores between 8 queries and 32 passages at SCORE_BAR, both pools; an all-masked sequence gives a NaN row.  P = H: the embeddings without W are >= 10 x
    COS_BAR away (for P != H the shapes differ already)."""
    H, heads = T.WIDTHS[dh]
    cfg, w = _model(dh, ff)
    Wd = T.dense_weight(P, H)
    h, h0, m = _hip(cfg, dict(w, **{"dense.weight": Wd})), _hip(cfg, w), T.hf_model(cfg, w)
    assert h.out_dim == P and h0.out_dim == H
    qi, qm = T.tokens(8, 32, "R", 3, VOCAB, lo=4)
    pi, pm = T.tokens(32, 128, "R", 4, VOCAB, lo=16)
    li, lm = T.tokens(3, 200, "L", 5, VOCAB)
    for pool in (0, 1):
        embs, refs = [], []
        for ids, mask in ((qi, qm), (pi, pm), (li, lm)):
            lh = T.hf_last_hidden(m, ids, mask)
            ref = T.pool_np(lh, mask, pool, Wd)
            out = h.forward_np(ids, mask, pool)
            assert out.shape == (len(ids), P) and out.dtype == np.float32 and np.isfinite(out).all()
            cos = float((1 - (out.astype(np.float64) * ref).sum(1) / np.linalg.norm(out.astype(np.float64), axis=1)).max())
            norm = float(np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1).max())
            print(f"[d_h {dh} P {P} {ff}] pool {pool} B {len(ids)} S {ids.shape[1]}: 1 - cos {cos:.2e}, | |out| - 1 | {norm:.1e}")
            assert cos <= COS_BAR and norm <= 1e-5, (pool, cos, norm)
            if P == H:
                plain = T.pool_np(lh, mask, pool)
                gap = float((1 - (plain * ref).sum(1)).min())
                assert gap >= 10 * COS_BAR, ("precondition", gap)
                assert not _same(out, h0.forward_np(ids, mask, pool))
            # the three ways in: the same bits, the same shape
            dev = h.forward(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), pool)
            assert tuple(dev.shape) == (len(ids), P) and _same(dev.cpu().numpy(), out)
            if not (mask[:, 0] == 0).any():
                rag, lens = _rag(ids, mask)
                pk = h.forward_packed(rag, lens, ids.shape[1], pool)
                assert tuple(pk.shape) == (len(ids), P) and _same(pk.cpu().numpy(), out)
            embs.append(out); refs.append(ref)
        score = float(np.abs(embs[0].astype(np.float64) @ embs[1].astype(np.float64).T - refs[0] @ refs[1].T).max())
        print(f"[d_h {dh} P {P} {ff}] pool {pool}: worst |q.d - ref| over 8 x 32 {score:.2e}")
        assert score <= SCORE_BAR, score
    # an all-masked sequence: the reference's own NaN (mean of nothing), not an error; its neighbours are untouched
    mask2 = qm.copy(); mask2[2] = 0
    out = h.forward_np(qi, mask2, 0)
    assert out.shape == (8, P) and np.isnan(out[2]).all() and np.isfinite(np.delete(out, 2, 0)).all()
    assert _same(np.delete(out, 2, 0), np.delete(h.forward_np(qi, qm, 0), 2, 0))
    h.check()
    assert h0.forward_np(qi, qm, 0).shape == (8, H)


@pytest.mark.parametrize("ff", [T.RELU, T.GATED])
def test_projection_loops_agree(ff, monkeypatch):
    """KIRAG_AMD_PROJ_TILE = 256, 128, 64, 32 (k_proj on both tiles, k_proj_skinny on both; 130: k_proj_split) give bit-identical last_hidden, so both new
    epilogues compute the same through every loop"""
    cfg, w = _model(64, ff)
    h = _hip(cfg, w)
    ids, mask = T.tokens(5, 128, "R", 21, VOCAB)
    got = {}
    for tile in (0, 256, 128, 130, 64, 32):
        if tile:
            monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
        h.forward_np(ids, mask, 0)
        got[tile] = h.last_hidden(5, 128).numpy()
        assert np.isfinite(got[tile]).all()
    monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
    for tile in (256, 128, 130, 64, 32):
        assert _same(got[tile], got[0]), tile


def _raw_handle(H=128, heads=4, FF=256, layers=1):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(H, layers, heads, FF, 100, 512, 1, 1e-6)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _load(lib, h, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)


def test_refusals_through_the_c_abi():
    from oracle import encoder_np as E
    H, heads, FFs = 128, 4, 256
    w = T.weights(H, 1, heads, FFs, 100, T.RELU)
    wg = T.weights(H, 1, heads, FFs, 100, T.GATED)
    bert = dict(E.synth_weights(H, 1, FFs, 100, 512, seed=3))
    bert["embeddings.token_type_embeddings.weight"] = np.zeros((1, H), np.float32)      # the raw handles have one token type

    def fresh(setting=None, tensors=None):
        lib, h = _raw_handle(H, heads, FFs)
        if setting is not None:
            assert _load(lib, h, T.SETTING, [setting]) == 0
        for k, v in (tensors or {}).items():
            assert _load(lib, h, k, v) == 0, k
        return lib, h

    # the setting itself
    lib, h = fresh()
    try:
        for bad in ([2.0], [0.5], [-1.0], [0.0, 1.0]):
            assert _load(lib, h, T.SETTING, bad) == KR_EINVAL
        assert _load(lib, h, "config.no_such_setting", [0.0]) == KR_EINVAL and b"config.t5_feed_forward" in lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(h)
    # next to each foreign setting: refused at finalize, by name
    half = H // heads // 2
    for name, val in (("config.position_padding_idx", [1.0]), ("config.rotary_inv_freq", np.ones(half)), ("config.rotary_inv_freq_local", np.ones(half)),
                      ("config.local_attention_layers", [0.0]), ("config.attention_half_window", [4.0])):
        lib, h = fresh(0.0, w)
        try:
            assert _load(lib, h, name, val) == 0, name
            assert lib.kr_encoder_finalize(h) == KR_EINVAL and b"config.t5_feed_forward" in lib.kr_last_error(), name
        finally:
            lib.kr_encoder_destroy(h)
    # T5's names on a BERT handle; BERT's names on a T5 handle; MPNet's spelling of the table on a T5 handle; the wrong feed-forward spelling
    for setting, tensors, extra in ((None, bert, {"encoder.block.0.layer.0.SelfAttention.q.weight": w["encoder.block.0.layer.0.SelfAttention.q.weight"]}),
                                    (None, bert, {T.BIAS_NAME: w[T.BIAS_NAME]}),
                                    (None, w, {}),
                                    (0.0, w, {"encoder.layer.0.attention.self.query.weight": bert["encoder.layer.0.attention.self.query.weight"]}),
                                    (0.0, {k: v for k, v in w.items() if k != T.BIAS_NAME}, {M.BIAS_NAME: w[T.BIAS_NAME]}),
                                    (0.0, wg, {}), (1.0, w, {})):
        lib, h = fresh(setting, tensors)
        try:
            for k, v in extra.items():
                assert _load(lib, h, k, v) == 0, k
            assert lib.kr_encoder_finalize(h) == KR_EINVAL, (setting, list(extra))
        finally:
            lib.kr_encoder_destroy(h)
    # a T5 handle without its table, or without a matrix: never loaded
    for drop in (T.BIAS_NAME, "encoder.final_layer_norm.weight", "encoder.block.0.layer.1.DenseReluDense.wi_1.weight"):
        src = wg if "wi_1" in drop else w
        lib, h = fresh(1.0 if src is wg else 0.0, {k: v for k, v in src.items() if k != drop})
        try:
            assert lib.kr_encoder_finalize(h) != 0 and b"never loaded" in lib.kr_last_error(), drop
        finally:
            lib.kr_encoder_destroy(h)
    # the table: 32 x heads, block 0 only
    lib, h = fresh(0.0)
    try:
        assert _load(lib, h, T.BIAS_NAME, np.zeros((16, heads))) == KR_EINVAL
        assert _load(lib, h, T.BIAS_NAME.replace("block.0", "block.1"), np.zeros((32, heads))) == KR_EINVAL
        # dense.weight: a count that is no multiple of H, P outside [4, 2048], P % 4 != 0
        for n in (H * 8 + 1, H * 2, H * 6, H * 2052):
            assert _load(lib, h, "dense.weight", np.zeros(n)) == KR_EINVAL, n
        assert b"dense.weight" in lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(h)
    # dense.weight on a handle that is no T5 handle
    lib, h = fresh(None, bert)
    try:
        assert _load(lib, h, "dense.weight", np.zeros((8, H))) == 0
        assert lib.kr_encoder_finalize(h) == KR_EINVAL and b"dense.weight" in lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(h)
    # after the first finalize everything is fixed: the setting, the presence and the width of the head; the same values are accepted
    ids = np.arange(2, 34, dtype=np.int64).reshape(2, 16); mask = np.ones((2, 16), np.int64)
    lib, h = fresh(0.0, w)
    try:
        assert lib.kr_encoder_finalize(h) == 0
        assert _load(lib, h, T.SETTING, [0.0]) == 0 and _load(lib, h, T.SETTING, [1.0]) == KR_EINVAL and b"finalize" in lib.kr_last_error()
        assert _load(lib, h, "dense.weight", np.zeros((8, H))) == KR_EINVAL and b"finalize" in lib.kr_last_error()
        assert _load(lib, h, "config.position_padding_idx", [1.0]) == KR_EINVAL
        out = np.empty((2, H), np.float32)
        assert lib.kr_encoder_finalize(h) == 0
        assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, 2, 16, 0, out.ctypes.data, None) == 0 and np.isfinite(out).all()
    finally:
        lib.kr_encoder_destroy(h)
    lib, h = fresh(0.0, dict(w, **{"dense.weight": T.dense_weight(8, H)}))
    try:
        assert lib.kr_encoder_finalize(h) == 0
        assert _load(lib, h, "dense.weight", T.dense_weight(12, H)) == KR_EINVAL
        assert _load(lib, h, "dense.weight", T.dense_weight(8, H, seed=9)) == 0 and lib.kr_encoder_finalize(h) == 0
        out = np.empty((2, 8), np.float32)
        assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, 2, 16, 0, out.ctypes.data, None) == 0 and np.isfinite(out).all()
    finally:
        lib.kr_encoder_destroy(h)
    # a BERT handle finalized without the setting stays one
    lib, h = fresh(None, bert)
    try:
        assert lib.kr_encoder_finalize(h) == 0
        assert _load(lib, h, T.SETTING, [0.0]) == KR_EINVAL and b"finalize" in lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(h)


def test_token_id_outside_the_vocabulary_and_both_operand_types():
    from kirag_amd import _lib
    cfg, w = _model(32, T.GATED)
    h = _hip(cfg, w)
    ids, mask = T.tokens(4, 64, "R", 3, VOCAB)
    good = h.forward_np(ids, mask, 0)
    bad = ids.copy(); bad[1, 3] = VOCAB
    with pytest.raises(_lib.KiragAmdError) as ei:
        h.forward_np(bad, mask, 0)
    assert ei.value.code == KR_EINVAL and "token id" in str(ei.value)
    assert _same(h.forward_np(ids, mask, 0), good)
    # bf16 operands round every stored activation to 8 significand bits (relative 2^-9 = 2e-3 per element); 1 - cos is quadratic in the relative error of the
    # pooled vector, so 1e-4 leaves a factor of ~25 over (2e-3)^2 for the accumulation over three layers
    hb = _hip(cfg, w, operand_dtype="bf16")
    m = T.hf_model(cfg, w)
    ref = T.pool_np(T.hf_last_hidden(m, ids, mask), mask, 0)
    for out, bar in ((good, COS_BAR), (hb.forward_np(ids, mask, 0), 1e-4)):
        assert np.isfinite(out).all() and float((1 - (out * ref).sum(1) / np.linalg.norm(out, axis=1)).max()) <= bar


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_end_to_end_from_a_checkpoint_folder(tmp_path, name, pool):
    """T5EncoderModel.save_pretrained + a hand-written modules.json and 2_Dense/: load_retriever(<existing name>, dir) returns the T5 twin with its head; the
    eval() forward (HIP) matches the train()-mode forward (torch: HF's last_hidden_state, pooling, Dense, normalise) at the embedding bars."""
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import load_retriever
    H, heads = T.WIDTHS[32]
    cfg = T.cfg(H, 2, heads, 512, VOCAB, T.GATED)
    w = T.weights(H, 2, heads, 512, VOCAB, T.GATED)
    td = str(tmp_path / "gtr-like")
    T.hf_model(cfg, w, device="cpu").save_pretrained(td)
    Wd = T.dense_weight(256, H)
    T.write_st_dense(td, Wd)
    e = load_retriever(name, td)
    assert type(e) is {"E5Retriever": ENC.T5E5Encoder, "BGERetriever": ENC.T5BGEEncoder}[name] and e.embedding_size == 256
    e = e.cuda()
    qi, qm = T.tokens(8, 32, "R", 3, VOCAB, lo=4)
    pi, pm = T.tokens(32, 96, "R", 4, VOCAB, lo=16)
    outs, refs = [], []
    for ids, mask in ((qi, qm), (pi, pm)):
        a, k = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
        out = e.eval()(a, k)
        assert tuple(out.shape) == (len(ids), 256) and out.is_cuda and not out.requires_grad
        with torch.no_grad():
            ref = e.train()(a, k)
        e.eval()
        out, ref = out.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
        cos = float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())
        assert np.isfinite(out).all() and cos <= COS_BAR, cos
        outs.append(out); refs.append(ref)
    assert e._hip.is_t5 and e._hip.out_dim == 256
    score = float(np.abs(outs[0] @ outs[1].T - refs[0] @ refs[1].T).max())
    print(f"[{name}] HIP eval() vs torch train(): worst |q.d - ref| {score:.2e}")
    assert score <= SCORE_BAR
    # ... and against the float64 head on HF's own last_hidden_state
    m = T.hf_model(cfg, w)
    ref64 = T.pool_np(T.hf_last_hidden(m, qi, qm), qm, pool, Wd)
    assert float((1 - (outs[0] * ref64).sum(1) / np.linalg.norm(outs[0], axis=1)).max()) <= COS_BAR
    # the ragged entry point through the model
    rag, lens = _rag(qi, qm)
    assert _same(e.forward_packed(rag, lens, 32).cpu().numpy(), e(torch.from_numpy(qi).cuda(), torch.from_numpy(qm).cuda()).cpu().numpy())


def test_checkpoint_check_tool_on_a_t5_folder_with_a_dense_head(tmp_path):
    """tools/checkpoint_check.py is where the README sends users with real GTR / Sentence-T5 weights.  On a saved synthetic checkpoint with a Dense head: it
    loads the twin with its head, its reference is HF's forward + pooling + head (equal to the float64 restatement), the hooks on encoder.block report every
    layer's residual stream, and the default mode holds the embedding bars."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import checkpoint_check as CC
    H, heads = T.WIDTHS[32]
    cfg = T.cfg(H, 2, heads, 512, VOCAB, T.GATED)
    w = T.weights(H, 2, heads, 512, VOCAB, T.GATED)
    td = str(tmp_path / "st5-like")
    T.hf_model(cfg, w, device="cpu").save_pretrained(td)
    Wd = T.dense_weight(256, H)
    T.write_st_dense(td, Wd)
    args = CC.parse([td, "--n", "8", "--max-length", "48", "--random-tokens", "--json", str(tmp_path / "out.json")])
    out = CC.check(td, args)
    assert out["tested_path"] == "hip" and len(out["layers"]) == 2
    for row in out["layers"]:
        assert row["ln1"]["max"] > 0 and row["ln2"]["max"] > 0 and 1.0 < row["max_16bit_tensor"] < 65504 and row["f16_headroom"] > 4
    modes = {(r["operand_dtype"], r["residual_lo"]): r for r in out["modes"]}
    assert len(modes) == 4 and all(r["finite"] for r in modes.values())
    assert modes[("f16", True)]["worst_1_minus_cos"] <= COS_BAR and modes[("f16", True)]["worst_score_error"] <= SCORE_BAR
    assert os.path.exists(str(tmp_path / "out.json"))
    # the tool's reference is HF's last_hidden_state + mean pooling + the folder's head
    from kirag_amd.retriever.encoders import T5E5Encoder
    model = T5E5Encoder.from_pretrained(td).float().eval().cuda()
    assert model.dense is not None
    batches = CC.load_inputs(args, td, VOCAB)
    ref, _ = CC.reference_and_stats(model, batches, "mean", torch.device("cuda:0"))
    m = T.hf_model(cfg, w)
    for (ids, mask), r in zip(batches, ref):
        exp = T.pool_np(T.hf_last_hidden(m, ids, mask), mask, 0, Wd)
        assert r.shape == (8, 256) and np.abs(r - exp).max() <= 1e-5
