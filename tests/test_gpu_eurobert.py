"""GPU tests of EuroBERT handles (a DECODER handle with config.decoder_attention = 0: pre-LN RMS norms, rotary q / k, SwiGLU, grouped-query k / v, a
BIDIRECTIONAL mask) and of the ``attention="bidirectional"`` switch of the Qwen2 / Llama / Mistral twins.  The reference is transformers' EuroBertModel (for the
switch: Qwen2Model under decoder_util.mask4d(mask, "none")) in fp32 with eager attention on the CPU, on synthetic weights (tests/eurobert_util.py).  Only
attended rows are compared.  Bars: last_hidden_state 3e-2 element-wise, embeddings 1 - cos <= 5e-5, scores within 1e-3.

Preconditions (asserted on the CPU; the weights' seed is advanced until all hold): a causal mask in place of none, no rotation, gate / up exchanged, a
mean-subtracting norm and no final norm each move an attended row of the reference by >= 10 x the bar."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402
import eurobert_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
POOL_MEAN, POOL_LAST = U.POOL_MEAN, U.POOL_LAST
KINDS = ["euro-64", "euro-32", "euro-384"]


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
    out = [U.tokens(B, S, lay, 100 + S + ord(lay) + holes, holes=holes) + ((S, lay, holes),) for B, S, lay, holes in CASES]
    out.append(U.tokens(5, 64, "R", 64, lens=[5, 7, 33, 1, 64]) + ((64, "ragged", 0),))
    return out


@pytest.fixture(scope="module")
def models():
    """kind -> (config, weights, handle, HF model on the CPU), made once.  The seed is advanced (at most 8 times) until every broken reference moves an
    attended row of the S = 40 batch by >= 10 x the bar: a precondition on the weights, decided on the CPU before the library runs."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cfg = U.hf_config(kind)
            ids, mask = U.tokens(3, 40, "R", 100 + 40 + ord("R"))
            for seed in range(5, 13):
                w = U.weights(cfg, seed)
                m = U.hf_model(cfg, w)
                dist = U.break_distances(m, ids, mask, U.hf_last_hidden(m, ids, mask))
                if min(dist.values()) >= 10 * HIDDEN_BAR:
                    break
            else:
                raise AssertionError(("precondition", kind, dist))
            print(f"[{kind}] seed {seed}: broken references move a row by {dist}")
            cache[kind] = (cfg, w, _hip(cfg, w), m)
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", KINDS)
def test_last_hidden_state_parity(kind, models):
    """kr_encoder_last_hidden against EuroBertModel, attended rows, bar 3e-2: S in {12, 40, 150, 300}, right and left padding, two holes in the mask, lengths
    {5, 7, 33, 1, 64} in one batch through kr_encoder_forward and through kr_encoder_forward_packed.  The handle is a decoder handle with the setting 0, made
    from the config alone (model_type eurobert); k / v go to the library in their grouped-query shape.  The preconditions are asserted again on a batch of
    every kernel path (S = 150, S = 300, the ragged batch)."""
    cfg, w, h, m = models(kind)
    assert h.is_decoder and h.decoder_attention == 0.0 and h.kv_heads < h.heads
    worst, weakest = 0.0, np.inf
    for ids, mask, what in _batches():
        keep = mask.astype(bool)
        ref = U.hf_last_hidden(m, ids, mask)
        if what in ((150, "R", 0), (300, "L", 0)) or what[1] == "ragged":
            dist = U.break_distances(m, ids, mask, ref)
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
            assert float(np.abs(lp - ref)[keep].max()) <= HIDDEN_BAR and _same(lp, lh)
    _note(f"[{kind}] last_hidden_state vs HF fp32 eager: worst {worst:.2e} (bar {HIDDEN_BAR}); weakest precondition distance {weakest:.2f} (required 0.3)")


@pytest.mark.parametrize("kind", KINDS)
def test_embeddings_against_hf(kind, models):
    """pools 0 (mean) / 5 (last) against HF + numpy pooling on the f16 default: 1 - cos <= 5e-5, scores within 1e-3; the bf16 handle runs and is finite"""
    cfg, w, h, m = models(kind)
    hb = _hip(cfg, w, operand_dtype="bf16")
    assert h.operand_dtype == "f16" and hb.operand_dtype == "bf16"
    parts = [U.tokens(6, 48, lay, 900 + i) for i, lay in enumerate("RL")]
    ids, mask = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    lh = U.hf_last_hidden(m, ids, mask)
    for pool in (POOL_MEAN, POOL_LAST):
        ref = U.pool_np(lh, mask, pool)
        out = h.forward_np(ids, mask, pool)
        cos, ds = _cos_gap(out, ref), float(np.abs(out @ out.T - ref @ ref.T).max())
        ob = hb.forward_np(ids, mask, pool)
        assert np.isfinite(ob).all()
        _note(f"[{kind}] pool {pool} vs HF fp32: f16 1 - cos {cos:.2e} (bar {COS_BAR}), |score - ref| {ds:.2e} (bar {SCORE_BAR}); bf16 1 - cos {_cos_gap(ob, ref):.2e} (no bar)")
        assert cos <= COS_BAR and ds <= SCORE_BAR, (pool, cos, ds)


def test_cls_pooling_is_refused_by_the_library(models):
    from kirag_amd import _lib
    cfg, w, h, m = models("euro-32")
    ids, mask = U.tokens(2, 12, "R", 2)
    with pytest.raises(_lib.KiragAmdError) as ei:
        h.forward_np(ids, mask, 1)
    assert ei.value.code == -22 and "KR_POOL_CLS" in str(ei.value) and "on a decoder handle" in str(ei.value)


@pytest.mark.parametrize("kind", ["euro-64", "euro-384"])
def test_one_arithmetic(kind, models, monkeypatch):
    """A sequence's rows are bit-identical alone, in a batch, in the reversed batch, right / left padded and from kr_encoder_forward_packed; both attention
    kernels (KIRAG_AMD_ATTN_LDS=1) and every KIRAG_AMD_PROJ_TILE give the same bits."""
    cfg, w, h, m = models(kind)
    for B, S, lay in ((6, 64, "R"), (3, 200, "L")):
        ids, mask = U.tokens(B, S, lay, 700 + S)
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
    rng = np.random.default_rng(5)
    ids = np.zeros((2, 300), np.int64); mask = np.zeros((2, 300), np.int64)
    ids[0, :100] = rng.integers(3, U.VOCAB, 100); ids[1] = rng.integers(3, U.VOCAB, 300)
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
        assert np.isfinite(both).all()
        assert _same(alone[0], both[0]) and _same(both, rev[::-1]) and _same(alone[0], lft[0]) and _same(both, packed), pool


def test_the_twins_run_a_saved_folder(tmp_path):
    """save_pretrained a tiny EuroBertModel; E5Encoder / BGEEncoder.from_pretrained return the twins (mean pooling both), whose eval forward matches HF +
    numpy pooling within the bars; pooling="last" likewise"""
    from kirag_amd.retriever import encoders as ENC
    cfg = U.hf_config("euro-32")
    w = U.weights(cfg)
    m = U.hf_model(cfg, w)
    td = str(tmp_path / "m")
    m.save_pretrained(td)
    ids, mask = U.tokens(6, 40, "L", 31)
    lh = U.hf_last_hidden(m, ids, mask)
    direct = _hip(cfg, w)
    for cls, twin, kw, pool in ((ENC.E5Encoder, ENC.EuroBertE5Encoder, {}, POOL_MEAN), (ENC.BGEEncoder, ENC.EuroBertBGEEncoder, {}, POOL_MEAN),
                                (ENC.BGEEncoder, ENC.EuroBertBGEEncoder, {"pooling": "last"}, POOL_LAST)):
        enc = cls.from_pretrained(td, **kw).cuda().eval()
        assert type(enc) is twin
        out = enc(torch.from_numpy(ids), torch.from_numpy(mask)).cpu().numpy()
        assert enc._hip.decoder_attention == 0.0 and _same(out, direct.forward_np(ids, mask, pool))
        ref = U.pool_np(lh, mask, pool)
        assert _cos_gap(out, ref) <= COS_BAR and float(np.abs(out @ out.T - ref @ ref.T).max()) <= SCORE_BAR


def test_the_bidirectional_switch_of_a_qwen2_folder(tmp_path):
    """A Qwen2 state dict loaded with attention="bidirectional" matches Qwen2Model under decoder_util.mask4d(mask, "none") at the 3e-2 bar and differs from the
    causal handle's rows by >= 10 x the bar; save_pretrained -> from_pretrained restores the choice and the bits"""
    from kirag_amd.retriever import encoders as ENC
    cfg = D.hf_config("qwen2-32")
    m = D.hf_model(cfg, D.weights(cfg))
    td = str(tmp_path / "q")
    m.save_pretrained(td)
    bi = ENC.E5Encoder.from_pretrained(td, attention="bidirectional").cuda().eval()
    causal = ENC.E5Encoder.from_pretrained(td).cuda().eval()
    worst = 0.0
    for B, S, lay, holes in ((3, 40, "R", 0), (2, 150, "L", 2), (2, 300, "R", 0)):
        ids, mask = D.tokens(B, S, lay, 500 + S, holes=holes)
        keep = mask.astype(bool)
        ref = D.hf_last_hidden(m, ids, mask, "none")
        out_bi = bi(torch.from_numpy(ids), torch.from_numpy(mask)).cpu().numpy()
        lh = bi.hip_last_hidden_state(B, S).numpy()
        causal(torch.from_numpy(ids), torch.from_numpy(mask))
        lc = causal.hip_last_hidden_state(B, S).numpy()
        err = float(np.abs(lh - ref)[keep].max())
        worst = max(worst, err)
        assert bi._hip.decoder_attention == 0.0 and causal._hip.decoder_attention == 1.0
        assert err <= HIDDEN_BAR, (S, lay, err)
        assert np.abs(lh - lc)[keep].max() >= 10 * HIDDEN_BAR
        assert float(np.abs(lc - D.hf_last_hidden(m, ids, mask))[keep].max()) <= HIDDEN_BAR      # the default is HF's own causal forward, unchanged
    _note(f"[qwen2-32 attention=bidirectional] last_hidden_state vs Qwen2Model under an all-admitting mask: worst {worst:.2e} (bar {HIDDEN_BAR})")
    td2 = str(tmp_path / "again")
    bi.save_pretrained(td2)
    again = ENC.BGEEncoder.from_pretrained(td2).cuda().eval()
    assert again.attention == "bidirectional" and _same(again(torch.from_numpy(ids), torch.from_numpy(mask)).cpu().numpy(), out_bi)


def test_checkpoint_check_tool_on_eurobert_and_bidirectional_folders(tmp_path):
    """tools/checkpoint_check.py on a saved EuroBERT folder and on a Qwen2 folder saved with attention="bidirectional" (seeded random tokens): every precision
    mode finite, the f16 default inside the bars against HF fp32 with eager attention under the mask the folder asks for"""
    import importlib.util
    from kirag_amd.retriever import encoders as ENC
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(repo, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    cfg = U.hf_config("euro-32")
    d = str(tmp_path / "e")
    U.hf_model(cfg, U.weights(cfg)).save_pretrained(d)
    qcfg = D.hf_config("qwen2-32")
    q0, q = str(tmp_path / "q0"), str(tmp_path / "q")
    D.hf_model(qcfg, D.weights(qcfg)).save_pretrained(q0)
    ENC.E5Encoder.from_pretrained(q0, attention="bidirectional").save_pretrained(q)
    for folder, pool in ((d, "mean"), (d, "last"), (q, "mean")):
        out = cc.check(folder, cc.parse([folder, "--n", "8", "--max-length", "48", "--random-tokens", "--pool", pool]))
        assert [m["operand_dtype"] for m in out["modes"]] == ["f16", "f16", "bf16", "bf16"] and all(m["finite"] for m in out["modes"])
        assert out["modes"][0]["worst_1_minus_cos"] <= COS_BAR and out["modes"][0]["worst_score_error"] <= SCORE_BAR, (folder, pool, out["modes"][0])
