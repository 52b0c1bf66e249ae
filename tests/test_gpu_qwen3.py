"""GPU tests of Qwen3 handles: the decoders' stack with a head width of its own ("config.head_dim": q and the context heads x head_dim wide, 128-wide heads
through k_attn_wide at every length), an RMS norm over every head of q and of k in front of the rotation (k_qk_norm_rope behind the EPI_QKV_SPLIT projection)
and the score head.  The reference is transformers' Qwen3Model / Qwen3ForSequenceClassification in fp32 with eager attention on synthetic weights
(tests/qwen3_util.py); only attended rows are compared.  Bars: last_hidden_state 3e-2 element-wise, embeddings 1 - cos <= 5e-5, scores
within 1e-3; the reranker's is twice the worst |logit - HF fp32| measured on the MI355X over its cases (below).  Measured values are printed, and appended to the
file KIRAG_AMD_MEASUREMENTS_FILE names (profiles/qwen3/measurements.txt holds such a run).

No Qwen3 weights exist offline: real-checkpoint numerics are NOT measured here."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402
import qwen3_util as Q  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL = -22
HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
POOL_MEAN, POOL_LAST, POOL_CLASSIFY = Q.POOL_MEAN, Q.POOL_LAST, Q.POOL_CLASSIFY
KINDS = tuple(sorted(Q.SHAPES))
# Reranker bar: 2 x the worst |logit - HF fp32| measured on the MI355X over RERANK_CASES with 1 and 3 labels on q3-128 (the project's convention): worst
# 4.827e-3 (both label counts, S 40 left-padded), so the bar is 9.654e-3; the other cases measure 4.4e-4 .. 2.9e-3 (profiles/qwen3/measurements.txt)
RERANK_MEASURED_WORST = 4.827e-3
RERANK_BAR = 2 * RERANK_MEASURED_WORST
RERANK_CASES = [(3, 12, "R", 0, None), (3, 40, "L", 0, None), (2, 150, "R", 0, None), (1, 300, "F", 0, None), (3, 40, "R", 2, None), (5, 64, "R", 0, (5, 7, 33, 1, 64))]
SCORE_NAME = "score.weight"
DIGESTS = os.path.join(REPO, "profiles", "qwen3", "unchanged_handles.json")


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
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _lh(h, ids, mask, pool=POOL_MEAN):
    h.forward_np(ids, mask, pool)
    return h.last_hidden(*ids.shape).numpy()


@pytest.fixture(scope="module")
def models():
    """(kind, layers) -> (config, weights, handle, HF model on the GPU), made once"""
    cache = {}

    def get(kind, L=2):
        if (kind, L) not in cache:
            cfg = Q.hf_config(kind, L=L)
            w = Q.weights(cfg)
            cache[(kind, L)] = (cfg, w, _hip(cfg, w), Q.hf_model(cfg, w, "cuda"))
        return cache[(kind, L)]
    return get


# ---------------------------------------------------------------------------------------------------------
# what fails without the feature
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_qwen3_handle_finalizes_and_runs_every_entry_point(kind):
    """Through the C interface alone: the head width, HF's frequencies, the mask, the state dict as it is.  kr_encoder_forward, _forward_tt and
    _forward_packed agree bit for bit with pools 0 and 5; q_proj with hidden rows is refused once the width is set."""
    import ctypes as C
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = Q.hf_config(kind)
    w = Q.weights(cfg)
    H, heads = cfg.hidden_size, cfg.num_attention_heads
    bc = _lib.BertCfg(H, cfg.num_hidden_layers, heads, cfg.intermediate_size, cfg.vocab_size, 512, 1, 1e-6)
    h = C.c_void_p()
    assert lib.kr_encoder_create_ex(C.byref(bc), 0, -1, -1, C.byref(h)) == 0
    try:
        def load(name, arr):
            a = np.ascontiguousarray(arr, np.float32)
            return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)
        for name, v in Q.library_settings(cfg):
            assert load(name, v) == 0, (name, lib.kr_last_error())
        if heads * cfg.head_dim != H:
            assert load("layers.0.self_attn.q_proj.weight", np.zeros((H, H))) == KR_EINVAL and b"config.head_dim" in lib.kr_last_error()
        for k, v in w.items():
            assert load(k, v) == 0, (k, lib.kr_last_error())
        assert load(Q.HEAD_DIM_NAME, [float(cfg.head_dim)]) == KR_EINVAL and b"before the weights" in lib.kr_last_error()
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        ids, mask = Q.tokens(3, 20, "R", 1)
        B, S = ids.shape
        tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32); tt = np.zeros_like(ids)
        for pool in (POOL_MEAN, POOL_LAST):
            outs = [np.full((B, H), 7.0, np.float32) for _ in range(3)]
            assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, outs[0].ctypes.data, None) == 0, lib.kr_last_error()
            assert lib.kr_encoder_forward_tt(h, ids.ctypes.data, mask.ctypes.data, tt.ctypes.data, B, S, pool, outs[1].ctypes.data, None) == 0, lib.kr_last_error()
            assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), pool, outs[2].ctypes.data, None) == 0, lib.kr_last_error()
            assert np.isfinite(outs[0]).all() and np.allclose(np.linalg.norm(outs[0], axis=1), 1, atol=1e-5)
            assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), pool
    finally:
        lib.kr_encoder_destroy(h)


# ---------------------------------------------------------------------------------------------------------
# parity with HF, element-wise
# ---------------------------------------------------------------------------------------------------------
def _assert_teeth(m, ids, mask, ref, what):
    """each way of breaking what is new moves some attended row of the batch's reference by >= 10 x the bar (HF alone, before the library is looked at)"""
    keep = mask.astype(bool)
    for how in Q.BREAKS:
        if how == "partner_32" and m.config.head_dim == 64:
            continue
        with Q.broken(m, how):
            moved = float(np.abs(Q.hf_last_hidden(m, ids, mask) - ref)[keep].max())
        assert moved >= 10 * HIDDEN_BAR, (what, how, moved)


# S 12 / 40 / 150 / 300 right- and left-padded, with holes; the lengths where the diagonal crosses tile and step edges
PARITY = [(4, 12, "R", 0, None), (4, 40, "L", 0, None), (4, 40, "R", 3, None), (3, 150, "R", 0, None), (3, 150, "L", 2, None), (2, 300, "R", 0, None),
          (6, 65, "R", 0, (31, 32, 33, 63, 64, 65)), (6, 65, "L", 0, (31, 32, 33, 63, 64, 65))]


@pytest.mark.parametrize("kind", KINDS)
def test_last_hidden_state_parity(kind, models):
    cfg, w, h, m = models(kind)
    worst = 0.0
    for n, (B, S, layout, holes, lens) in enumerate(PARITY):
        ids, mask = Q.tokens(B, S, layout, seed=300 + n, lens=lens, holes=holes)
        keep = mask.astype(bool)
        ref = Q.hf_last_hidden(m, ids, mask)
        if n in (1, 3):
            _assert_teeth(m, ids, mask, ref, (kind, n))
        out = _lh(h, ids, mask)
        err = float(np.abs(out - ref)[keep].max())
        worst = max(worst, err)
        print(f"[{kind}] B {B} S {S} {layout} holes {holes} lens {lens}: max |last_hidden - HF| {err:.3e}")
        assert np.isfinite(out[keep]).all() and err <= HIDDEN_BAR, (kind, PARITY[n], err)
        if layout == "R" and not holes:      # the ragged input computes the same rows
            tok, ln = _rag(ids, mask)
            h.forward_packed(tok, ln, S, POOL_MEAN)
            assert _same(h.last_hidden(B, S).numpy()[keep], out[keep])
    _note(f"[{kind}] last_hidden_state vs HF fp32 eager over {len(PARITY)} batches: worst {worst:.3e} (bar {HIDDEN_BAR:.0e})")


@pytest.mark.parametrize("kind", ["q3-128", "q3-64"])
def test_bidirectional_setting(kind, models):
    cfg, w, _, m = models(kind)
    h = _hip(cfg, w, attention=0.0)
    for S in (40, 150):
        ids, mask = Q.tokens(3, S, "R", seed=S)
        keep = mask.astype(bool)
        ref = Q.hf_last_hidden(m, ids, mask, rule="none")
        assert np.abs(ref - Q.hf_last_hidden(m, ids, mask))[keep].max() >= 10 * HIDDEN_BAR      # the mask decides rows
        err = float(np.abs(_lh(h, ids, mask) - ref)[keep].max())
        print(f"[{kind} bidirectional] S {S}: {err:.3e}")
        assert err <= HIDDEN_BAR


@pytest.mark.parametrize("kind", ["q3-128", "q3-64"])
def test_one_layer_handle_shows_the_norm_kernel_alone(kind, models):
    """one layer: q and k pass k_qk_norm_rope once, nothing averages its error away"""
    cfg, w, h, m = models(kind, L=1)
    ids, mask = Q.tokens(4, 70, "R", seed=70)
    keep = mask.astype(bool)
    ref = Q.hf_last_hidden(m, ids, mask)
    _assert_teeth(m, ids, mask, ref, (kind, "L1"))
    err = float(np.abs(_lh(h, ids, mask) - ref)[keep].max())
    _note(f"[{kind} 1 layer] last_hidden_state vs HF fp32: {err:.3e}")
    assert err <= HIDDEN_BAR


@pytest.mark.parametrize("kind", KINDS)
def test_embeddings_against_hf(kind, models):
    cfg, w, h, m = models(kind)
    for S, layout in ((40, "R"), (150, "L"), (300, "R")):
        ids, mask = Q.tokens(6, S, layout, seed=500 + S)
        lh = Q.hf_last_hidden(m, ids, mask)
        for pool in (POOL_MEAN, POOL_LAST):
            ref = Q.pool_np(lh, mask, pool)
            out = h.forward_np(ids, mask, pool)
            cos, ds = _cos_gap(out, ref), float(np.abs(out @ out.T - ref @ ref.T).max())
            _note(f"[{kind}] S {S} {layout} pool {pool}: 1 - cos {cos:.2e}, |score - ref| {ds:.2e}")
            assert cos <= COS_BAR and ds <= SCORE_BAR, (kind, S, pool, cos, ds)


# ---------------------------------------------------------------------------------------------------------
# one arithmetic
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_arithmetic(kind, models, monkeypatch):
    """a sequence's rows are the same bits alone, in a batch, in the reversed batch, right / left padded, from packed input and under every projection tiling —
    across k_attn_wide's heads-per-block variants (and, for q3-64, across k_attn_lds / k_attn_dma)"""
    cfg, w, h, m = models(kind)
    lens = [150, 17, 64, 33, 1, 129]
    ids, mask = Q.tokens(6, 150, "R", seed=9, lens=lens)
    B, S = ids.shape
    base = _lh(h, ids, mask)
    emb = h.forward_np(ids, mask, POOL_LAST)
    for b in range(B):
        n = lens[b]
        for width in sorted({n, (n + 31) // 32 * 32, S}):      # alone, in batches of other widths: 1 / 2 / 4 heads per block, the other attention kernel
            one = _lh(h, ids[b:b + 1, :width], mask[b:b + 1, :width])
            assert _same(one[0, :n], base[b, :n]), (b, width)
        lid = np.zeros((1, S), np.int64); lm = np.zeros((1, S), np.int64)
        lid[0, S - n:] = ids[b, :n]; lm[0, S - n:] = 1
        assert _same(_lh(h, lid, lm)[0, S - n:], base[b, :n]), b
    rev = _lh(h, ids[::-1].copy(), mask[::-1].copy())
    for b in range(B):
        assert _same(rev[B - 1 - b, :lens[b]], base[b, :lens[b]])
    tok, ln = _rag(ids, mask)
    assert _same(h.forward_packed(tok, ln, S, POOL_LAST).cpu().numpy(), emb)
    for tile in (256, 130, 128, 64, 32):
        monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
        assert _same(h.forward_np(ids, mask, POOL_LAST), emb), tile
    monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")


# ---------------------------------------------------------------------------------------------------------
# rerankers
# ---------------------------------------------------------------------------------------------------------
def _rr_weights(cfg, seed=5):
    w = Q.weights(cfg, seed)
    for k in w:
        if k.endswith(("self_attn.v_proj.weight", "self_attn.o_proj.weight")):
            w[k] = w[k] * np.float32(2.0)
    rng = np.random.default_rng(11)
    w[SCORE_NAME] = np.ascontiguousarray(rng.standard_normal((cfg.num_labels, cfg.hidden_size)) / cfg.hidden_size ** 0.5, dtype=np.float32)
    return w


@functools.lru_cache(maxsize=None)
def _hf_classifier(labels):
    from transformers import Qwen3ForSequenceClassification
    cfg = Q.hf_config("q3-128", num_labels=labels)
    w = _rr_weights(cfg)
    m = Qwen3ForSequenceClassification(cfg)
    res = m.load_state_dict({(k if k == SCORE_NAME else "model." + k): torch.from_numpy(v) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval()


@torch.no_grad()
def _hf_logits(m, ids, mask, chunk=8):
    outs = []
    for i in range(0, len(ids), chunk):
        outs.append(m(input_ids=torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])), attention_mask=torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk]))).logits.double().numpy())
    return np.concatenate(outs)


@pytest.fixture(scope="module")
def rerankers(tmp_path_factory):
    from kirag_amd.retriever.rerankers import BaseReranker
    cache = {}

    def get(labels):
        if labels not in cache:
            d = str(tmp_path_factory.mktemp("qwen3_reranker") / f"q3-{labels}")
            _hf_classifier(labels).save_pretrained(d)
            cache[labels] = BaseReranker("BGEReranker", d).to("cuda").eval()
        return cache[labels]
    return get


@pytest.mark.parametrize("labels", [1, 3])
def test_reranker_parity_with_hf(labels, rerankers):
    from kirag_amd.retriever.rerankers import Qwen3Reranker
    rr = rerankers(labels)
    assert type(rr.reranker) is Qwen3Reranker
    worst = 0.0
    for B, S, layout, holes, lens in RERANK_CASES:
        ids, mask = D.tokens(B, S, layout, seed=100 + S + ord(layout) + holes, lens=lens, holes=holes)
        ref = _hf_logits(_hf_classifier(labels), ids, mask)
        out = rr.score(dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))).float().cpu().numpy().reshape(ref.shape)
        if lens is not None:
            packed = rr.reranker._synced_hip().forward_packed(*_rag(ids, mask), S, POOL_CLASSIFY).cpu().numpy()
            assert _same(packed, out)
        err = float(np.abs(out - ref).max())
        worst = max(worst, err)
        print(f"[q3-128 L {labels}] B {B} S {S} {layout} holes {holes}: max |logit - HF| {err:.3e}")
        assert np.isfinite(out).all() and err <= RERANK_BAR, (S, layout, err)
    _note(f"[q3-128 L {labels}] logits vs HF fp32 eager over {len(RERANK_CASES)} cases: worst {worst:.3e} (bar {RERANK_BAR:.3e})")


def test_reranker_shortcut_and_full_handles_agree_bit_for_bit(monkeypatch):
    cfg = Q.hf_config("q3-128", num_labels=3)
    w = _rr_weights(cfg)
    short = _hip(cfg, w)
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
    full = _hip(cfg, w)
    monkeypatch.delenv("KIRAG_AMD_CLS_FULL")
    for B, S, layout, holes, lens in RERANK_CASES:
        ids, mask = D.tokens(B, S, layout, seed=7 + S, lens=lens, holes=holes)
        a, b = short.forward_np(ids, mask, POOL_CLASSIFY), full.forward_np(ids, mask, POOL_CLASSIFY)
        assert a.shape == (B, 3) and np.isfinite(a).all() and _same(a, b), (S, layout)
        if layout == "R" and not holes:
            assert _same(short.forward_packed(*_rag(ids, mask), S, POOL_CLASSIFY).cpu().numpy(), a)


def test_64_passages_come_back_in_hf_s_order(rerankers):
    from kirag_amd.retriever.rerankers import rank_order
    ids, mask = D.tokens(64, 40, "R", seed=64)
    ref = _hf_logits(_hf_classifier(1), ids, mask)[:, 0]
    out = rerankers(1).score(dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))).cpu().numpy()
    assert out.shape == (64,) and np.abs(out - ref).max() <= RERANK_BAR
    i, j = np.triu_indices(64, 1)
    decided = np.abs(ref[i] - ref[j]) > 2 * RERANK_BAR
    assert decided.sum() > 1000 and (np.sign(out[i] - out[j])[decided] == np.sign(ref[i] - ref[j])[decided]).all()
    pos = {int(p): r for r, p in enumerate(rank_order(out))}
    assert all((pos[a] < pos[b]) == (ref[a] > ref[b]) for a, b, d in zip(i, j, decided) if d)


def test_from_causal_lm_on_a_tied_qwen3_folder(tmp_path):
    """Qwen3-Reranker-0.6B's shape of checkpoint: a Qwen3ForCausalLM whose lm_head is embed_tokens.  The folded one-label head equals
    lm_head[pos] . x - lm_head[neg] . x on HF's last row.  The bar: the logit is w . x and the error of x does not depend on w, so the bar of the score-head
    cases scales with the norm of the row — the folded row (a difference of two embedding rows of N(0.4, 1): norm ~ 16) over the smallest row of the parity
    cases' score.weight (N(0, 1 / hidden): norm ~ 1)."""
    from transformers import Qwen3ForCausalLM
    from kirag_amd.retriever.rerankers import DecoderReranker, Qwen3Reranker
    cfg = Q.hf_config("q3-128", tie_word_embeddings=True)
    w = Q.weights(cfg)
    lm = Qwen3ForCausalLM(cfg)
    res = lm.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    lm.tie_weights()
    d = str(tmp_path / "lm")
    lm.float().eval().save_pretrained(d)
    pos, neg = 17, 23
    rr = DecoderReranker.from_causal_lm(d, pos, neg).to("cuda")
    assert type(rr) is Qwen3Reranker
    ids, mask = D.tokens(5, 40, "R", seed=3)
    with torch.no_grad():
        logits = lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).logits.double().numpy()
    last = D.last_index(mask)
    ref = logits[np.arange(len(ids)), last, pos] - logits[np.arange(len(ids)), last, neg]
    out = rr(input_ids=torch.from_numpy(ids).cuda(), attention_mask=torch.from_numpy(mask).cuda()).logits.float().cpu().numpy()[:, 0]
    err = float(np.abs(out - ref).max())
    folded = float(np.linalg.norm(w["embed_tokens.weight"][pos] - w["embed_tokens.weight"][neg]))
    smallest = min(float(np.linalg.norm(r)) for L in (1, 3) for r in _rr_weights(Q.hf_config("q3-128", num_labels=L))[SCORE_NAME])
    bar = RERANK_BAR * folded / smallest
    _note(f"[q3-128 from_causal_lm, tied] yes - no logit vs HF fp32: {err:.3e} (bar {bar:.3e} = {RERANK_BAR:.3e} x {folded:.2f} / {smallest:.2f})")
    assert err <= bar


# ---------------------------------------------------------------------------------------------------------
# nothing else moved
# ---------------------------------------------------------------------------------------------------------
def unchanged_digests():
    """sha256 of what a qwen2 and a llama handle of decoder_util compute (last_hidden_state of the attended rows, mean and last embeddings) on fixed batches
    that reach k_attn_lds with 1 / 2 / 4 heads per block and k_attn_dma.  profiles/qwen3/unchanged_handles.json holds the values of the library before Qwen3."""
    out = {}
    for kind in ("qwen2-32", "llama-64"):
        cfg = D.hf_config(kind)
        h = _hip(cfg, D.weights(cfg))
        for S in (24, 60, 120, 300):
            ids, mask = D.tokens(3, S, "R", seed=S)
            keep = mask.astype(bool)
            dig = hashlib.sha256()
            dig.update(np.ascontiguousarray(_lh(h, ids, mask)[keep]).tobytes())
            dig.update(np.ascontiguousarray(h.forward_np(ids, mask, POOL_MEAN)).tobytes())
            dig.update(np.ascontiguousarray(h.forward_np(ids, mask, POOL_LAST)).tobytes())
            out[f"{kind} S {S}"] = dig.hexdigest()
    return out


def test_qwen2_and_llama_handles_compute_the_bits_they_did():
    with open(DIGESTS) as f:
        want = json.load(f)
    assert unchanged_digests() == want["digests"]


# ---------------------------------------------------------------------------------------------------------
# a saved folder
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pool", [("E5Retriever", POOL_MEAN), ("BGERetriever", POOL_LAST)])
def test_saved_folder_round_trip(tmp_path, name, pool):
    """save_pretrained a tiny Qwen3Model + a toy tokenizer; load_retriever returns the Qwen3 twin (E5 -> mean, BGE -> last); its embeddings from text are HF's
    within the bars; a save_pretrained / reload round trip keeps class, pooling and bits"""
    import xlmr_util as X
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import load_retriever
    words = X.toy_words(190)
    tok = X.toy_tokenizer(words)
    cfg = Q.hf_config("q3-128", vocab_size=max(Q.VOCAB, tok.vocab_size))
    m = Q.hf_model(cfg, Q.weights(cfg))
    td = str(tmp_path / "model")
    m.save_pretrained(td)
    tok.save_pretrained(td)
    enc = load_retriever(name, td).cuda().eval()
    assert type(enc) is {"E5Retriever": ENC.Qwen3E5Encoder, "BGERetriever": ENC.Qwen3BGEEncoder}[name] and enc._pool == pool
    rng = np.random.default_rng(2)
    texts = [" ".join(rng.choice(words, int(n))) for n in rng.integers(3, 40, 24)]
    a = tok(texts, padding=True, return_tensors="pt")
    ids, mask = a["input_ids"].numpy(), a["attention_mask"].numpy()
    out = enc(a["input_ids"].cuda(), a["attention_mask"].cuda()).cpu().numpy()
    assert enc._hip.is_decoder
    ref = Q.pool_np(Q.hf_last_hidden(m, ids, mask), mask, pool)
    cos, ds = _cos_gap(out, ref), float(np.abs(out @ out.T - ref @ ref.T).max())
    _note(f"[{name} on a saved q3-128 folder] 1 - cos {cos:.2e}, |q.d - ref| {ds:.2e}")
    assert cos <= COS_BAR and ds <= SCORE_BAR
    td2 = str(tmp_path / "again")
    enc.save_pretrained(td2)
    again = load_retriever("E5Retriever" if name == "BGERetriever" else "BGERetriever", td2).cuda().eval()
    assert again._pool == pool and type(again).__name__.startswith("Qwen3")
    assert _same(again(a["input_ids"].cuda(), a["attention_mask"].cuda()).cpu().numpy(), out)
