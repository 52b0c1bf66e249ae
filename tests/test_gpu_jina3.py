"""GPU tests of jina-embeddings-v3 handles (family ROTARY_BERT: NomicBert's post-LN rotary stack with q / k / v / o biases — q's and k's added before the
rotation, EPI_QKV_ROTB — and BERT's feed-forward fc2(gelu(fc1 x + b1)) + b2, EPI_GELU on a plain-order fc1).  The reference is transformers'
JinaEmbeddingsV3Model in fp32 with eager attention on the CPU, on synthetic weights (tests/jina3_util.py).  HF's rows at masked query positions are artefacts of
its finite mask value, so only attended rows are compared.  Bars: last_hidden_state 3e-2 element-wise on rows of magnitude ~ 1, embeddings
1 - cos <= 5e-5, scores within 1e-3.  The worst measured values are printed, and appended to the file KIRAG_AMD_MEASUREMENTS_FILE names.

Preconditions (asserted on the CPU; the weights' seed is advanced until all hold): no rotation, the mirrored rotation, no q bias, no k bias, no o bias, no fc1
bias and the SwiGLU reading of fc1 each move an attended row of the reference by >= 10 x the bar.  tanh-GELU for erf-GELU is NOT among them: the two differ
by at most 4.7e-4 per activation, which moves no row of these models by 0.3 (measured: ~ 1e-3), so the test has no teeth against that exchange."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jina3_util as J  # noqa: E402

pytestmark = pytest.mark.gpu

HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
POOL_MEAN, POOL_CLS = J.POOL_MEAN, J.POOL_CLS
KINDS = ["jina-64", "jina-32"]


def _note(line):
    print(line)
    path = os.environ.get("KIRAG_AMD_MEASUREMENTS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _hip(cfg, w, **kw):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(cfg, 0, **kw)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _lh(h, ids, mask, pool=POOL_MEAN):
    h.forward_np(ids, mask, pool)
    return h.last_hidden(*ids.shape).numpy()


# S = 300 takes k_attn_dma, the others k_attn_lds; 40 and 150 cross the 32-query tile and the 64-key step
CASES = [(3, 12, "R", 0), (3, 40, "R", 0), (3, 40, "L", 0), (2, 150, "R", 0), (2, 150, "L", 0), (2, 300, "R", 0), (2, 300, "L", 0), (3, 40, "R", 2), (2, 150, "L", 2),
         (2, 300, "R", 2)]


def _batches():
    out = [J.tokens(B, S, lay, 100 + S + ord(lay) + holes, holes=holes) + ((S, lay, holes),) for B, S, lay, holes in CASES]
    out.append(J.tokens(5, 64, "R", 64, lens=[5, 7, 33, 1, 64]) + ((64, "ragged", 0),))
    return out


def _weakest_break(m, ids, mask, ref):
    keep = mask.astype(bool)
    worst = {}
    for how in J.BREAKS:
        with J.broken(m, how):
            worst[how] = float(np.abs(ref - J.hf_last_hidden(m, ids, mask))[keep].max())
    return worst


@pytest.fixture(scope="module")
def models():
    """kind -> (config, weights, handle, HF model on the CPU), made once.  The seed is advanced (at most 8 times) until every broken
    reference moves an attended row of the S = 40 batch by >= 10 x the bar: a precondition on the weights, decided on the CPU before the library runs."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cfg = J.hf_config(kind)
            ids, mask = J.tokens(3, 40, "R", 100 + 40 + ord("R"))
            for seed in range(5, 13):
                w = J.weights(cfg, seed)
                m = J.hf_model(cfg, w)
                dist = _weakest_break(m, ids, mask, J.hf_last_hidden(m, ids, mask))
                if min(dist.values()) >= 10 * HIDDEN_BAR:
                    break
            else:
                raise AssertionError(("precondition", kind, dist))
            print(f"[{kind}] seed {seed}: broken references move a row by {dist}")
            cache[kind] = (cfg, w, _hip(cfg, w), m)
        return cache[kind]
    return get


def test_a_rotary_bert_handle_finalizes_and_runs_every_entry_point():
    """Without the feature "config.rotary_feed_forward" is an unknown setting and mlp.fc1 an unknown tensor.  With it the handle finalizes from HF's own state
    dict and runs kr_encoder_forward, _forward_tt and _forward_packed with pools 0 and 1; pool 5 stays KR_EINVAL (no decoder handle)."""
    import ctypes as C
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = J.hf_config("jina-32")
    w = J.weights(cfg)
    H = cfg.hidden_size
    bc = _lib.BertCfg(H, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size, cfg.vocab_size, 512, cfg.type_vocab_size, 1e-5)
    h = C.c_void_p()
    assert lib.kr_encoder_create_ex(C.byref(bc), 0, -1, -1, C.byref(h)) == 0
    try:
        def load(name, arr):
            a = np.ascontiguousarray(arr, np.float32)
            return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)
        assert load(J.INV_FREQ_NAME, J.hf_model(cfg, w).rotary_emb.inv_freq.numpy()) == 0, lib.kr_last_error()
        assert load(J.SETTING, [1.0]) == 0, lib.kr_last_error()
        for k, v in w.items():
            assert load(k, v) == 0, (k, lib.kr_last_error())
        assert lib.kr_encoder_finalize(h) == 0, lib.kr_last_error()
        ids, mask = J.tokens(3, 20, "R", 1)
        B, S = ids.shape
        tok = np.ascontiguousarray(ids[mask != 0], np.int32); lens = mask.sum(1).astype(np.int32); tt = np.zeros_like(ids)
        for pool in (POOL_MEAN, POOL_CLS):
            outs = [np.full((B, H), 7.0, np.float32) for _ in range(3)]
            assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, pool, outs[0].ctypes.data, None) == 0, lib.kr_last_error()
            assert lib.kr_encoder_forward_tt(h, ids.ctypes.data, mask.ctypes.data, tt.ctypes.data, B, S, pool, outs[1].ctypes.data, None) == 0, lib.kr_last_error()
            assert lib.kr_encoder_forward_packed(h, tok.ctypes.data, lens.ctypes.data, B, S, C.c_int64(tok.size), pool, outs[2].ctypes.data, None) == 0, lib.kr_last_error()
            assert np.isfinite(outs[0]).all() and np.allclose(np.linalg.norm(outs[0], axis=1), 1, atol=1e-5)
            assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), pool
        out = np.zeros((B, H), np.float32)
        assert lib.kr_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, B, S, 5, out.ctypes.data, None) == -22 and b"decoder handles" in lib.kr_last_error()
        assert load(J.SETTING, [0.0]) == -22 and b"fixed at the handle's first finalize" in lib.kr_last_error()
        assert load(J.SETTING, [1.0]) == 0
    finally:
        lib.kr_encoder_destroy(h)


@pytest.mark.parametrize("kind", KINDS)
def test_last_hidden_state_parity(kind, models):
    """kr_encoder_last_hidden against HF, attended rows, bar 3e-2: S in {12, 40, 150, 300}, right and left padding, two holes in the mask, lengths
    {5, 7, 33, 1, 64} in one batch through kr_encoder_forward and the same batch through kr_encoder_forward_packed.  The preconditions are asserted again on a
    batch of every kernel path (S = 150, S = 300, the ragged batch)."""
    cfg, w, h, m = models(kind)
    worst, weakest = 0.0, np.inf
    for ids, mask, what in _batches():
        keep = mask.astype(bool)
        ref = J.hf_last_hidden(m, ids, mask)
        assert 0.5 <= np.abs(ref[keep]).mean() * (np.pi / 2) ** 0.5 <= 2.0           # rows of magnitude ~ 1: the bar is absolute
        if what in ((150, "R", 0), (300, "L", 0)) or what[1] == "ragged":
            dist = _weakest_break(m, ids, mask, ref)
            weakest = min(weakest, min(dist.values()))
            assert min(dist.values()) >= 10 * HIDDEN_BAR, ("precondition", what, dist)
        lh = _lh(h, ids, mask)
        err = float(np.abs(lh - ref)[keep].max())
        worst = max(worst, err)
        print(f"[{kind}] S {what[0]} {what[1]} holes {what[2]}: max |last_hidden - HF| {err:.2e}")
        assert np.isfinite(lh).all() and not lh[~keep].any() and err <= HIDDEN_BAR, (what, err)
        if what[1] == "ragged":
            rag, lens = _rag(ids, mask)
            h.forward_packed(rag, lens, ids.shape[1], POOL_MEAN).cpu()
            lp = h.last_hidden(*ids.shape).numpy()
            errp = float(np.abs(lp - ref)[keep].max())
            print(f"[{kind}] the same batch through kr_encoder_forward_packed: {errp:.2e}")
            assert errp <= HIDDEN_BAR and _same(lp, lh)
    _note(f"[{kind}] last_hidden_state vs HF fp32 eager: worst {worst:.2e} (bar {HIDDEN_BAR}); weakest precondition distance {weakest:.2f} (required 0.3)")


@pytest.mark.parametrize("kind", KINDS)
def test_embeddings_against_hf(kind, models):
    """pools 0 / 1 against HF + numpy pooling on the f16 default: 1 - cos <= 5e-5, scores within 1e-3; the bf16 handle runs and is finite (figures only)"""
    cfg, w, h, m = models(kind)
    hb = _hip(cfg, w, operand_dtype="bf16")
    assert h.operand_dtype == "f16" and hb.operand_dtype == "bf16" and h.is_jina3
    ids, mask = J.tokens(12, 48, "R", 900)
    lh = J.hf_last_hidden(m, ids, mask)
    for pool in (POOL_MEAN, POOL_CLS):
        ref = J.pool_np(lh, mask, pool)
        out = h.forward_np(ids, mask, pool)
        cos, ds = _cos_gap(out, ref), float(np.abs(out @ out.T - ref @ ref.T).max())
        ob = hb.forward_np(ids, mask, pool)
        assert np.isfinite(ob).all()
        _note(f"[{kind}] pool {pool} vs HF fp32: f16 1 - cos {cos:.2e} (bar {COS_BAR}), |score - ref| {ds:.2e} (bar {SCORE_BAR}); bf16 1 - cos {_cos_gap(ob, ref):.2e} (no bar)")
        assert cos <= COS_BAR and ds <= SCORE_BAR, (pool, cos, ds)


@pytest.mark.parametrize("kind", KINDS)
def test_one_arithmetic(kind, models, monkeypatch):
    """A sequence's rows are bit-identical alone, in a batch, in the reversed batch, right / left padded and from kr_encoder_forward_packed; both attention
    kernels (KIRAG_AMD_ATTN_LDS=1) and every KIRAG_AMD_PROJ_TILE give the same bits."""
    cfg, w, h, m = models(kind)
    for B, S, lay in ((6, 64, "R"), (3, 200, "L")):
        ids, mask = J.tokens(B, S, lay, 700 + S)
        monkeypatch.delenv("KIRAG_AMD_PROJ_TILE", raising=False)
        auto = h.forward_np(ids, mask, POOL_MEAN)
        lh = h.last_hidden(B, S).numpy()
        assert np.isfinite(auto).all()
        for tile in (256, 130, 128, 64, 32):
            monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
            assert _same(h.forward_np(ids, mask, POOL_MEAN), auto), (B, S, tile)
        monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
        monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
        assert _same(h.forward_np(ids, mask, POOL_MEAN), auto) and _same(h.last_hidden(B, S).numpy(), lh), (B, S, "attn_lds")
        monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
    # a 100-token sequence alone (k_attn_lds), next to a 300-token one (k_attn_dma), in the reversed batch, left-padded, ragged
    rng = np.random.default_rng(5)
    ids = np.zeros((2, 300), np.int64); mask = np.zeros((2, 300), np.int64)
    ids[0, :100] = rng.integers(3, J.VOCAB, 100); ids[1] = rng.integers(3, J.VOCAB, 300)
    mask[0, :100] = 1; mask[1] = 1
    left = np.zeros((1, 300), np.int64); lmask = np.zeros((1, 300), np.int64)
    left[0, 200:], lmask[0, 200:] = ids[0, :100], 1
    rag, lens = _rag(ids, mask)
    alone = h.forward_np(ids[:1, :100], mask[:1, :100], POOL_MEAN)
    rows = h.last_hidden(1, 100).numpy()[0]
    both = h.forward_np(ids, mask, POOL_MEAN)
    assert _same(h.last_hidden(2, 300).numpy()[0, :100], rows)
    rev = h.forward_np(ids[::-1].copy(), mask[::-1].copy(), POOL_MEAN)
    lft = h.forward_np(left, lmask, POOL_MEAN)
    assert _same(h.last_hidden(1, 300).numpy()[0, 200:], rows)
    packed = h.forward_packed(rag, lens, 300, POOL_MEAN).cpu().numpy()
    assert _same(h.last_hidden(2, 300).numpy()[0, :100], rows)
    assert np.isfinite(both).all()
    assert _same(alone[0], both[0]) and _same(both, rev[::-1]) and _same(alone[0], lft[0]) and _same(both, packed)


def test_the_twins_run_a_saved_folder(tmp_path):
    """save_pretrained a tiny JinaEmbeddingsV3Model; E5Encoder / BGEEncoder.from_pretrained return the twins, whose eval forward (the library, weights through
    named_parameters()) matches HF + numpy pooling within the bars and equals the handle loaded from the state dict bit for bit"""
    from kirag_amd.retriever import encoders as ENC
    cfg = J.hf_config("jina-32")
    w = J.weights(cfg)
    m = J.hf_model(cfg, w)
    td = str(tmp_path / "m")
    m.save_pretrained(td)
    ids, mask = J.tokens(6, 40, "R", 31)
    lh = J.hf_last_hidden(m, ids, mask)
    direct = _hip(cfg, w)
    for cls, twin, pool in ((ENC.E5Encoder, ENC.JinaV3E5Encoder, POOL_MEAN), (ENC.BGEEncoder, ENC.JinaV3BGEEncoder, POOL_CLS)):
        enc = cls.from_pretrained(td).cuda().eval()
        assert type(enc) is twin
        out = enc(torch.from_numpy(ids), torch.from_numpy(mask)).cpu().numpy()
        assert enc._hip.is_jina3 and _same(out, direct.forward_np(ids, mask, pool))
        ref = J.pool_np(lh, mask, pool)
        assert _cos_gap(out, ref) <= COS_BAR and float(np.abs(out @ out.T - ref @ ref.T).max()) <= SCORE_BAR


def test_checkpoint_check_tool_on_a_jina3_folder(tmp_path):
    """tools/checkpoint_check.py on a saved folder without a tokenizer (seeded random tokens): every precision mode finite, the f16 default inside the bars
    against HF fp32 with eager attention"""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(repo, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    cfg = J.hf_config("jina-32")
    d = str(tmp_path / "j")
    J.hf_model(cfg, J.weights(cfg)).save_pretrained(d)
    for pool in ("mean", "cls"):
        out = cc.check(d, cc.parse([d, "--n", "8", "--max-length", "48", "--random-tokens", "--pool", pool]))
        assert [m["operand_dtype"] for m in out["modes"]] == ["f16", "f16", "bf16", "bf16"] and all(m["finite"] for m in out["modes"])
        assert out["modes"][0]["worst_1_minus_cos"] <= COS_BAR and out["modes"][0]["worst_score_error"] <= SCORE_BAR, out["modes"][0]
