"""GPU tests of decoder-LLM embedders (Qwen2Model / LlamaModel used as sentence encoders: a pre-LN stack of RMS norms, rotary q / k, SwiGLU, grouped-query
attention expanded at weight sync, a CAUSAL mask — key column <= query column, AM_CAUSAL in both attention kernels — and mean or last-token pooling,
KR_POOL_LAST).  The reference is transformers' Qwen2Model / LlamaModel in fp32 with eager attention on synthetic weights (tests/decoder_util.py).  HF's rows
at masked query positions are artefacts of its finite mask value, so only attended rows are compared.  Bars: last_hidden_state 3e-2
element-wise, embeddings 1 - cos <= 5e-5, scores within 1e-3.  The worst measured values are printed, and appended to the file KIRAG_AMD_MEASUREMENTS_FILE names
(section 1 of profiles/decoder/measurements.txt is such a run)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL, KR_ERANGE = -22, -34
HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
POOL_MEAN, POOL_LAST = D.POOL_MEAN, D.POOL_LAST
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _note(line):
    print(line)
    path = os.environ.get("KIRAG_AMD_MEASUREMENTS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _hip(cfg, w, attention=1.0, **kw):
    from kirag_amd.retriever.encoders import HipBertForward

    class H(HipBertForward):
        DECODER_ATTENTION = float(attention)
    h = H(cfg, 0, **kw)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


@pytest.fixture(scope="module")
def models():
    """kind -> (config, weights, handle, HF model on the GPU), made once"""
    cache = {}

    def get(kind, L=2):
        if (kind, L) not in cache:
            cfg = D.hf_config(kind, L=L)
            w = D.weights(cfg)
            cache[(kind, L)] = (cfg, w, _hip(cfg, w), D.hf_model(cfg, w, "cuda"))
        return cache[(kind, L)]
    return get


def _lh(h, ids, mask, pool=POOL_MEAN):
    h.forward_np(ids, mask, pool)
    return h.last_hidden(*ids.shape).numpy()


# ---------------------------------------------------------------------------------------------------------
# the test that fails without the feature
# ---------------------------------------------------------------------------------------------------------
def test_a_decoder_handle_finalizes_and_runs_every_entry_point():
    """Without the feature "config.decoder_attention" is an unknown setting and pool 5 is KR_EINVAL.  With it a DECODER handle finalizes and runs
    kr_encoder_forward, _forward_tt and _forward_packed with pools 0 and 5; pool 5 on a BERT handle and pools 1 / 2 / 4 (and 5 with a flag) on a DECODER
    handle are KR_EINVAL."""
    from kirag_amd import _lib
    from kirag_amd.retriever.encoders import expand_kv
    from oracle import encoder_np as E
    lib = _lib.load()
    cfg = D.hf_config("qwen2-32")
    w = D.weights(cfg)
    H, heads = cfg.hidden_size, cfg.num_attention_heads
    bc = _lib.BertCfg(H, cfg.num_hidden_layers, heads, cfg.intermediate_size, cfg.vocab_size, 512, 1, 1e-6)
    h = C.c_void_p()
    assert lib.kr_encoder_create_ex(C.byref(bc), 0, -1, -1, C.byref(h)) == 0
    try:
        def load(name, arr):
            a = np.ascontiguousarray(arr, np.float32)
            return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)
        inv = D.hf_model(cfg, w).rotary_emb.inv_freq.numpy()
        assert load(D.INV_FREQ_NAME, inv) == 0, lib.kr_last_error()
        assert load(D.SETTING, [1.0]) == 0, lib.kr_last_error()
        for k, v in w.items():
            assert load(k, expand_kv(k, v, heads, cfg.num_key_value_heads)) == 0, (k, lib.kr_last_error())
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        ids, mask = D.tokens(3, 20, "R", 1)
        B, S = ids.shape
        tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32); tt = np.zeros_like(ids)
        for pool in (POOL_MEAN, POOL_LAST):
            outs = [np.full((B, H), 7.0, np.float32) for _ in range(3)]
            assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, outs[0].ctypes.data, None) == 0, lib.kr_last_error()
            assert lib.kr_encoder_forward_tt(h, ids.ctypes.data, mask.ctypes.data, tt.ctypes.data, B, S, pool, outs[1].ctypes.data, None) == 0, lib.kr_last_error()
            assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), pool, outs[2].ctypes.data, None) == 0, lib.kr_last_error()
            assert np.isfinite(outs[0]).all() and np.allclose(np.linalg.norm(outs[0], axis=1), 1, atol=1e-5)
            assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), pool
        out = np.zeros((B, H + S * 2), np.float32)
        for pool, word in ((1, b"KR_POOL_CLS"), (2, b"KR_POOL_CLASSIFY"), (4, b"KR_POOL_SPLADE"), (POOL_LAST | 0x10, b"not with 5 (last token)"), (POOL_LAST | 0x20, b"not with 5 (last token)"), (3, b"pool must be"), (6, b"pool must be")):
            assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, out.ctypes.data, None) == KR_EINVAL, pool
            assert word in lib.kr_last_error(), (pool, lib.kr_last_error())
        assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), 1, out.ctypes.data, None) == KR_EINVAL
    finally:
        lib.kr_encoder_destroy(h)
    # a BERT handle refuses pool 5, and says why
    from kirag_amd.retriever.encoders import HipBertForward
    from types import SimpleNamespace
    bcfg = SimpleNamespace(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=100, max_position_embeddings=64,
                           type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")
    hb = HipBertForward(bcfg, 0)
    hb.load_state(E.synth_weights(128, 1, 256, 100, 64, seed=5))
    i2, m2 = E.synth_tokens(2, 8, seed=1, vocab_lo=5, vocab_hi=100)
    with pytest.raises(_lib.KiragAmdError) as ei:
        hb.forward_np(i2, m2, POOL_LAST)
    assert ei.value.code == KR_EINVAL and "decoder handles" in str(ei.value)


# ---------------------------------------------------------------------------------------------------------
# parity with HF, element-wise, and the preconditions
# ---------------------------------------------------------------------------------------------------------
def _assert_teeth(m, ids, mask, ref, what):
    """each way of breaking the feature moves some attended row of the batch's reference by >= 10 x the bar"""
    keep = mask.astype(bool)
    weakest = np.inf
    for how in D.MASK_BREAKS + D.MODEL_BREAKS:
        if how == "no_bias" and not D.has_bias(m):
            continue
        if how in D.MASK_BREAKS:
            other = D.hf_last_hidden(m, ids, mask, how)
        else:
            with D.broken(m, how):
                other = D.hf_last_hidden(m, ids, mask)
        d = float(np.abs(ref - other)[keep].max())
        weakest = min(weakest, d)
        assert d >= 10 * HIDDEN_BAR, ("precondition", what, how, d)
    return weakest


CASES = [(3, S, lay, 0) for S in (12, 40, 150) for lay in ("R", "L")] + [(2, S, "R", 0) for S in (31, 32, 33, 63, 64, 65, 129)] + \
        [(2, S, "L", 0) for S in (33, 65)] + [(3, 40, "R", 4), (2, 150, "L", 9), (2, 129, "R", 5)]


@pytest.mark.parametrize("kind", ["qwen2-32", "llama-64", "qwen2-384"])
def test_last_hidden_state_parity_where_the_causal_mask_has_teeth(kind, models):
    """kr_encoder_last_hidden against HF (own causal mask), attended rows, bar 3e-2: S in {12, 40, 150} right / left padded, S in {31 .. 65, 129} so that the
    diagonal crosses the 32-query tile and the 64-key step in every position, masks with holes, one sequence of 300 (k_attn_dma) and lengths
    {5, 7, 33, 1, 64} in one batch.  Preconditions on the reference for every batch: no mask, the mirrored mask, the strict mask, no q / k / v biases, a
    mean-subtracting norm, no final norm, gate and up exchanged and no rotation each move an attended row by >= 0.3."""
    cfg, w, h, m = models(kind, 3 if kind == "qwen2-32" else 2)
    assert h.is_decoder and h.kv_heads < h.heads
    worst, weakest = 0.0, np.inf
    batches = [D.tokens(B, S, lay, 100 + S + ord(lay) + holes, holes=holes) + ((S, lay, holes),) for B, S, lay, holes in CASES]
    batches.append(D.tokens(1, 300, "F", 300) + ((300, "F", 0),))
    batches.append(D.tokens(5, 64, "R", 64, lens=[5, 7, 33, 1, 64]) + ((64, "ragged", 0),))
    for ids, mask, what in batches:
        keep = mask.astype(bool)
        ref = D.hf_last_hidden(m, ids, mask)
        if what[0] in (12, 40, 150, 65, 300) or what[1] == "ragged":       # the preconditions cost 8 reference forwards: on the batches of every kernel path
            weakest = min(weakest, _assert_teeth(m, ids, mask, ref, what))
        lh = _lh(h, ids, mask)
        err = float(np.abs(lh - ref)[keep].max())
        worst = max(worst, err)
        print(f"[{kind}] S {what[0]} {what[1]} holes {what[2]}: max |last_hidden - HF| {err:.2e}")
        assert np.isfinite(lh).all() and not lh[~keep].any() and err <= HIDDEN_BAR, (what, err)
    _note(f"[{kind}] last_hidden_state vs HF fp32 eager: worst {worst:.2e} (bar {HIDDEN_BAR}); weakest precondition distance {weakest:.2f} (required 0.3)")


def test_left_and_right_padded_references_agree(models):
    """HF's own runs of one sequence under right and left padding (default position ids) agree far below the bar: the reference does not depend on the layout"""
    cfg, w, h, m = models("qwen2-32", 3)
    ids, mask = D.tokens(1, 40, "F", 3)
    r = np.zeros((1, 60), np.int64); rm = np.zeros((1, 60), np.int64); l = np.zeros((1, 60), np.int64); lm = np.zeros((1, 60), np.int64)
    r[0, :40], rm[0, :40], l[0, 20:], lm[0, 20:] = ids[0], 1, ids[0], 1
    d = float(np.abs(D.hf_last_hidden(m, r, rm)[0, :40] - D.hf_last_hidden(m, l, lm)[0, 20:]).max())
    print(f"HF right vs left padded: {d:.2e}")
    assert d <= 1e-5


@pytest.mark.parametrize("kind", ["qwen2-32", "llama-64"])
def test_causality_without_a_reference(kind, models):
    """changing the token at column c leaves every row of columns < c bit-identical and moves some row >= c: c at 0, 31, 32, 64, S - 1, at S = 100
    (k_attn_lds) and S = 200 (k_attn_dma)"""
    cfg, w, h, m = models(kind, 3 if kind == "qwen2-32" else 2)
    for S in (100, 200):
        ids, mask = D.tokens(1, S, "F", 40 + S)
        base = _lh(h, ids, mask)
        for c in (0, 31, 32, 64, S - 1):
            i2 = ids.copy()
            i2[0, c] = 3 + (ids[0, c] - 3 + 17) % (D.VOCAB - 3)
            lh = _lh(h, i2, mask)
            assert _same(lh[0, :c], base[0, :c]), (S, c)
            assert np.abs(lh[0, c:] - base[0, c:]).max() > 1e-2, (S, c)


def test_bidirectional_setting(models):
    """config.decoder_attention = 0 on the same stack: parity with HF under an all-admitting 4-D mask at the same bar, and its rows differ from value 1's"""
    cfg, w, h1, m = models("qwen2-32", 3)
    h0 = _hip(cfg, w, attention=0.0)
    worst = 0.0
    for B, S, lay, holes in ((3, 40, "R", 0), (2, 150, "L", 0), (2, 65, "R", 3)):
        ids, mask = D.tokens(B, S, lay, 500 + S, holes=holes)
        keep = mask.astype(bool)
        ref = D.hf_last_hidden(m, ids, mask, "none")
        lh = _lh(h0, ids, mask)
        err = float(np.abs(lh - ref)[keep].max())
        worst = max(worst, err)
        assert err <= HIDDEN_BAR, (S, lay, err)
        assert np.abs(lh - _lh(h1, ids, mask))[keep].max() >= 10 * HIDDEN_BAR
    _note(f"[qwen2-32] bidirectional (setting 0) vs HF with an all-admitting mask: worst {worst:.2e} (bar {HIDDEN_BAR})")


# ---------------------------------------------------------------------------------------------------------
# one arithmetic
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["qwen2-32", "llama-64", "qwen2-384"])
def test_one_arithmetic(kind, models, monkeypatch):
    """A sequence's rows are bit-identical alone, in a batch, in the reversed batch, right / left padded and from kr_encoder_forward_packed; both attention
    kernels (KIRAG_AMD_ATTN_LDS=1) and every KIRAG_AMD_PROJ_TILE give the same bits; consecutive key columns == gathered ones."""
    cfg, w, h, m = models(kind, 3 if kind == "qwen2-32" else 2)
    for B, S, lay in ((6, 64, "R"), (4, 200, "L"), (2, 32, "F")):
        ids, mask = D.tokens(B, S, lay, 700 + S)
        for pool in (POOL_MEAN, POOL_LAST):
            monkeypatch.delenv("KIRAG_AMD_PROJ_TILE", raising=False)
            auto = h.forward_np(ids, mask, pool)
            lh = h.last_hidden(B, S).numpy()
            assert np.isfinite(auto).all()
            for tile in (256, 130, 128, 64, 32):
                monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
                assert _same(h.forward_np(ids, mask, pool), auto), (B, S, pool, tile)
            monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
            monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
            assert _same(h.forward_np(ids, mask, pool), auto) and _same(h.last_hidden(B, S).numpy(), lh), (B, S, pool, "attn_lds")
            monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
    monkeypatch.setenv("KIRAG_AMD_ATTN_BIAS_GATHER", "1")
    hg = _hip(cfg, w)
    monkeypatch.delenv("KIRAG_AMD_ATTN_BIAS_GATHER")
    # a 100-token sequence alone (k_attn_lds), next to a 300-token one (k_attn_dma), in the reversed batch, left-padded, ragged, with gathered columns
    rng = np.random.default_rng(5)
    ids = np.zeros((2, 300), np.int64); mask = np.zeros((2, 300), np.int64)
    ids[0, :100] = rng.integers(3, D.VOCAB, 100); ids[1] = rng.integers(3, D.VOCAB, 300)
    mask[0, :100] = 1; mask[1] = 1
    left = np.zeros((1, 300), np.int64); lmask = np.zeros((1, 300), np.int64)
    left[0, 200:], lmask[0, 200:] = ids[0, :100], 1
    rag, lens = _rag(ids, mask)
    for pool in (POOL_MEAN, POOL_LAST):
        alone = h.forward_np(ids[:1, :100], mask[:1, :100], pool)
        rows = h.last_hidden(1, 100).numpy()[0]
        both = h.forward_np(ids, mask, pool)
        assert _same(h.last_hidden(2, 300).numpy()[0, :100], rows)
        rev = h.forward_np(ids[::-1].copy(), mask[::-1].copy(), pool)
        lft = h.forward_np(left, lmask, pool)
        assert _same(h.last_hidden(1, 300).numpy()[0, 200:], rows)
        packed = h.forward_packed(rag, lens, 300, pool).cpu().numpy()
        assert _same(h.last_hidden(2, 300).numpy()[0, :100], rows)
        gathered = hg.forward_np(ids, mask, pool)
        assert np.isfinite(both).all()
        assert _same(alone[0], both[0]) and _same(both, rev[::-1]) and _same(alone[0], lft[0]) and _same(both, packed) and _same(both, gathered), pool


# ---------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------
def test_last_token_pooling(models):
    """pool 5 == the normalised last attended row of kr_encoder_last_hidden under left padding, right padding and a hole just before the end; an all-masked
    sequence gives a NaN row with return code 0 (both pools)"""
    cfg, w, h, m = models("qwen2-32", 3)
    ids, mask = D.tokens(4, 40, "R", 11, lens=[40, 17, 33, 9])
    i2, m2 = D.tokens(3, 40, "L", 12, lens=[40, 5, 32])
    m3 = mask.copy(); m3[0, 38] = 0; m3[1, 15] = 0; m3[2, 30:32] = 0; m3[3, 7] = 0
    for a, k in ((ids, mask), (i2, m2), (ids, m3)):
        out = h.forward_np(a, k, POOL_LAST)
        lh = h.last_hidden(*a.shape).numpy()
        rows = lh[np.arange(len(a)), D.last_index(k)].astype(np.float64)
        want = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
        assert np.abs(out - want).max() <= 2e-7, float(np.abs(out - want).max())
    m4 = mask.copy(); m4[1] = 0
    for pool in (POOL_MEAN, POOL_LAST):
        out = h.forward_np(ids, m4, pool)
        assert np.isnan(out[1]).all() and np.isfinite(out[[0, 2, 3]]).all(), pool
        h.check()


def test_a_nan_weight_is_kr_erange():
    from kirag_amd import _lib
    cfg = D.hf_config("llama-32")
    w = D.weights(cfg)
    w["layers.1.mlp.down_proj.weight"] = w["layers.1.mlp.down_proj.weight"].copy()
    w["layers.1.mlp.down_proj.weight"][3, 5] = np.nan
    h = _hip(cfg, w)
    ids, mask = D.tokens(2, 12, "R", 2)
    for pool in (POOL_MEAN, POOL_LAST):
        with pytest.raises(_lib.KiragAmdError) as ei:
            h.forward_np(ids, mask, pool)
        assert ei.value.code == KR_ERANGE, ei.value


@pytest.mark.parametrize("kind", ["qwen2-32", "llama-64", "qwen2-384"])
def test_embeddings_against_hf(kind, models):
    """pools 0 / 5 against HF + numpy pooling on the f16 default: 1 - cos <= 5e-5, scores within 1e-3; the bf16 handle runs and is finite (figures only)"""
    cfg, w, h, m = models(kind, 3 if kind == "qwen2-32" else 2)
    hb = _hip(cfg, w, operand_dtype="bf16")
    assert h.operand_dtype == "f16" and hb.operand_dtype == "bf16"
    parts = [D.tokens(6, 48, lay, 900 + i) for i, lay in enumerate("RL")]
    ids, mask = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    lh = D.hf_last_hidden(m, ids, mask)
    for pool in (POOL_MEAN, POOL_LAST):
        ref = D.pool_np(lh, mask, pool)
        out = h.forward_np(ids, mask, pool)
        cos, ds = _cos_gap(out, ref), float(np.abs(out @ out.T - ref @ ref.T).max())
        ob = hb.forward_np(ids, mask, pool)
        assert np.isfinite(ob).all()
        _note(f"[{kind}] pool {pool} vs HF fp32: f16 1 - cos {cos:.2e} (bar {COS_BAR}), |score - ref| {ds:.2e} (bar {SCORE_BAR}); bf16 1 - cos {_cos_gap(ob, ref):.2e} (no bar)")
        assert cos <= COS_BAR and ds <= SCORE_BAR, (pool, cos, ds)


# ---------------------------------------------------------------------------------------------------------
# the reference's entry points
# ---------------------------------------------------------------------------------------------------------
class _Corpus:
    def __init__(self, n, words, rng):
        self.p = ["title:  " + " ".join(rng.choice(words, 2)) + ", text:  " + " ".join(rng.choice(words, int(rng.integers(3, 40)))) for _ in range(n)]
        self.index_to_passage_id = {i: str(2 * i + 5) for i in range(n)}

    def __len__(self):
        return len(self.p)

    def __getitem__(self, i):
        return {"index": i, "passage": self.p[i]}

    def get_document(self, docid):
        return {"id": docid, "text": self.p[(int(docid) - 5) // 2]}


@pytest.mark.parametrize("name,pool,override", [("E5Retriever", POOL_MEAN, None), ("BGERetriever", POOL_LAST, None), ("E5Retriever", POOL_LAST, "last")])
def test_reference_entry_points_on_a_saved_qwen2_checkpoint(tmp_path, name, pool, override):
    """save_pretrained a tiny Qwen2Model + a toy fast tokenizer; load_retriever(<existing name>, dir) returns the Qwen2 twin (E5 -> mean, BGE -> last, a
    1_Pooling/config.json overrides the class default); a save_pretrained / reload round trip keeps class, pooling and bits; cal_doc_embeddings from text
    through the packed path writes rows that equal the padded forward bit for bit and the HF fp32 embeddings within the bars."""
    import json
    import pickle
    import xlmr_util as X
    from kirag_amd import compute_corpus_embeddings as CC
    from kirag_amd.collators import COLLATOR_MAP
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import InBatchRetriever, load_retriever
    words = X.toy_words(190)
    tok = X.toy_tokenizer(words)
    cfg = D.hf_config("qwen2-32", vocab_size=max(D.VOCAB, tok.vocab_size))
    w = D.weights(cfg)
    td = str(tmp_path / "model")
    m = D.hf_model(cfg, w)
    m.save_pretrained(td)
    tok.save_pretrained(td)
    if override:
        os.makedirs(os.path.join(td, "1_Pooling"))
        with open(os.path.join(td, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": cfg.hidden_size, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False, "pooling_mode_lasttoken": True}, f)
    twin = {"E5Retriever": ENC.Qwen2E5Encoder, "BGERetriever": ENC.Qwen2BGEEncoder}[name]
    enc = load_retriever(name, td)
    assert type(enc) is twin and enc._pool == pool and enc.pooling == ("mean" if pool == POOL_MEAN else "last")
    rng = np.random.default_rng(9)
    corpus = _Corpus(300, words, rng)
    tag = name.lower()
    enc_args = CC.setup_parser(["--retriever_name", name, "--retriever_model_name_or_path", td, "--tokenizer_name_or_path", td, "--save_dir", str(tmp_path),
                                "--name", tag, "--index_folder", "c", "--doc_maxlength", "48", "--per_gpu_batch_size", "8",
                                "--num_passage_per_index_file", "300", "--encode_batch_size", "128", "--tokenizer_workers", "0"])
    ret = InBatchRetriever(name, td, temperature=0.01)
    assert type(ret.encoder) is twin and ret.hidden_size == cfg.hidden_size and ret.encoder._pool == pool
    col = COLLATOR_MAP[name](tokenizer=tok, query_maxlength=24, doc_maxlength=48)
    CC.cal_doc_embeddings(enc_args, ret, corpus, col)
    assert ret.encoder._hip.is_decoder
    folder = os.path.join(str(tmp_path), tag, "c")
    files = sorted(f for f in os.listdir(folder) if f.startswith("corpus_embeddings_"))
    assert len(files) == 1
    with open(os.path.join(folder, files[0]), "rb") as f:
        x = pickle.load(f).numpy()
    assert x.shape == (300, cfg.hidden_size)
    a = col.encode_doc(corpus.p[:128])
    ids, mask = a["input_ids"].numpy(), a["attention_mask"].numpy()
    assert (mask == 0).any()
    ret.encoder.eval()
    padded = ret.encoder(a["input_ids"].cuda(), a["attention_mask"].cuda()).cpu().numpy()
    assert _same(padded, np.ascontiguousarray(x[:128]))
    ref = D.pool_np(D.hf_last_hidden(m.cuda(), ids, mask), mask, pool)
    cos, ds = _cos_gap(x[:128], ref), float(np.abs(x[:128] @ x[:128].T - ref @ ref.T).max())
    _note(f"[{name}{' + 1_Pooling' if override else ''}] written rows vs HF fp32: 1 - cos {cos:.2e}, |q.d - ref| {ds:.2e}")
    assert cos <= COS_BAR and ds <= SCORE_BAR
    # round trip: the pooling travels with the checkpoint
    td2 = str(tmp_path / "again")
    ret.encoder.save_pretrained(td2)
    again = load_retriever("E5Retriever" if name == "BGERetriever" else "BGERetriever", td2)
    assert again._pool == pool and type(again).__name__.startswith("Qwen2")
    again = again.cuda().eval()
    assert _same(again(a["input_ids"].cuda(), a["attention_mask"].cuda()).cpu().numpy(), padded)
    assert load_retriever(name, td2, pooling="mean")._pool == POOL_MEAN


@pytest.mark.parametrize("pool", ["mean", "last"])
def test_checkpoint_check_tool_on_a_qwen2_folder(tmp_path, pool):
    """tools/checkpoint_check.py on a saved Qwen2 folder without a tokenizer (seeded random tokens): every precision mode finite, the f16 default inside the bars
    against HF fp32 with eager attention"""
    import importlib.util
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(REPO, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    cfg = D.hf_config("qwen2-32")
    d = str(tmp_path / "q")
    D.hf_model(cfg, D.weights(cfg)).save_pretrained(d)
    out = cc.check(d, cc.parse([d, "--n", "8", "--max-length", "48", "--random-tokens", "--pool", pool]))
    assert [m["operand_dtype"] for m in out["modes"]] == ["f16", "f16", "bf16", "bf16"] and all(m["finite"] for m in out["modes"])
    assert out["modes"][0]["worst_1_minus_cos"] <= COS_BAR and out["modes"][0]["worst_score_error"] <= SCORE_BAR, out["modes"][0]
