"""GPU tests of the DeBERTa-v2 / v3 cross-encoder rerankers (DebertaV2ForSequenceClassification: mixedbread-ai/mxbai-rerank-*-v1, cross-encoder/nli-deberta-v3-*,
naver/trecdl22-crossencoder-debertav3): the dispatch of BGEReranker.from_pretrained (the test that fails without the feature), logits end to end against HF
fp32 through BaseReranker.score, the erf-GELU variant of the head kernel against an a-priori fp32 bound on the library's own CLS rows, batch invariance, ranking
through BaseReranker.rerank, and that pools 0 / 1 of a handle with the head are those of a handle without it.  Synthetic weights (deberta_util.weights + head);
no DeBERTa checkpoint exists offline.  HF runs on the CPU (DeBERTa's attention is eager only)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deberta_util as D  # noqa: E402
import reranker_util as R  # noqa: E402

pytestmark = pytest.mark.gpu

KR_ESTATE = -1
POOL_MEAN, POOL_CLS, POOL_CLASSIFY = 0, 1, 2
# |logit - HF fp32 logit|: twice the worst value measured over the end-to-end cases below on MI355X (WORST_MEASURED, profiles/deberta/measurements.txt), rounded
# up to two significant digits.  The kernels are deterministic; the factor leaves room for cases added later.  (Larger than the other families' bars because
# these weights are: deberta_util's scales put the f16 emulation of the encoder at 3e-3 per element of the CLS row, and the head spreads it by out_scale 4.)
WORST_MEASURED = 6.757e-3
LOGIT_BAR = 1.4e-2
SHAPES = {2: (128, 2, 2, 256), 4: (128, 2, 4, 256)}      # heads -> (H, layers, heads, FF): 2 heads of 64 / 4 heads of 32


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _model(heads, labels, bm=(256, 512), layers=None, H=None):
    Hd, L, hd, FF = SHAPES[heads] if H is None else (H, layers, heads, 256)
    c = D.cfg(Hd, L if layers is None else layers, hd, FF, bm[0], bm[1], labels=labels)
    w = dict(D.weights(c))
    w.update(D.head(Hd, labels))
    return c, w


def _hip(c, w):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(c, 0)
    h.load_state(w)
    return h


def _reranker(tmp_path, heads, labels=1, bm=(256, 512), **kw):
    from kirag_amd.retriever.rerankers import BaseReranker
    c, w = _model(heads, labels, bm)
    m = D.hf_classifier(c, w)
    d = str(tmp_path / f"deberta{heads}_{labels}")
    m.save_pretrained(d)
    rr = BaseReranker("BGEReranker", d, **kw)
    rr.to("cuda")
    rr.eval()
    return rr, m, w


def test_from_pretrained_dispatches_a_deberta_folder(tmp_path):
    """the test that fails without the feature: BGEReranker.from_pretrained of a deberta-v2 folder raised NotImplementedError"""
    from kirag_amd.retriever import rerankers as RR
    rr, m, _ = _reranker(tmp_path, 2)
    assert type(rr.reranker) is RR.DebertaV2Reranker and rr.device.type == "cuda"
    ids, mask = D.tokens(5, 24, seed=1)
    s = rr.score({"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask), "token_type_ids": torch.zeros(5, 24, dtype=torch.long)})
    assert s.is_cuda and s.shape == (5,) and not s.requires_grad and rr.reranker._hip.is_deberta and rr.reranker._hip.num_labels == 1
    assert np.abs(s.double().cpu().numpy() - D.hf_logits(m, ids, mask)[:, 0]).max() < 0.05          # the head, not an embedding (the bar proper: below)


E2E_CASES = [(S, layout) for S in (12, 40, 150) for layout in ("right", "holes")]


@pytest.mark.parametrize("heads,labels", [(2, 1), (4, 3)])
def test_end_to_end_against_hf_fp32(heads, labels, tmp_path):
    """BaseReranker.score of a saved checkpoint against DebertaV2ForSequenceClassification in fp32: S = 12, 40, 150, right padding and holes in the mask (the
    head reads the row of column 0: a left-padded row whose column 0 is masked has no reference — HF attends uniformly over masked columns there — and is only
    asked to be finite), 1 and 3 labels.  Teeth, on the reference before anything runs on the GPU: the head restated by hand agrees with the task model, and
    each broken variant (tanh for the GELU, bd or bo dropped, the mean row, the normalised row, the neighbour's row) moves some logit by more than 10 x
    LOGIT_BAR.  Measured on MI355X (profiles/deberta/measurements.txt): worst |logit - HF| see WORST_MEASURED."""
    rr, m, w = _reranker(tmp_path, heads, labels)
    cases = {cs: D.tokens(9, cs[0], seed=cs[0] + heads, holes=cs[1] == "holes") for cs in E2E_CASES}
    refs = {cs: D.hf_logits(m, *v) for cs, v in cases.items()}
    hidden = {cs: D.hf_hidden(m.deberta, *v) for cs, v in cases.items()}
    assert max(float(np.abs(D.head_by_hand(w, hidden[cs], cases[cs][1]) - refs[cs]).max()) for cs in E2E_CASES) < 1e-5
    moves = {b: max(float(np.abs(D.head_by_hand(w, hidden[cs], cases[cs][1], broken=b) - refs[cs]).max()) for cs in E2E_CASES) for b in D.HEAD_MUTATIONS}
    print(f"[heads {heads} labels {labels}] teeth: " + ", ".join(f"{k} {v:.3f}" for k, v in moves.items()))
    assert min(moves.values()) > 10 * LOGIT_BAR, moves
    worst = 0.0
    for cs, (ids, mask) in cases.items():
        args = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}
        if cs[1] == "holes":
            args = {k: v.cuda() for k, v in args.items()}
        s = rr.score(args)
        assert s.is_cuda and s.shape == ((9,) if labels == 1 else (9, labels)) and not s.requires_grad
        err = float(np.abs(s.double().cpu().numpy().reshape(9, labels) - refs[cs]).max())
        worst = max(worst, err)
        print(f"[heads {heads} labels {labels}] S {cs[0]} {cs[1]}: worst |logit - HF| {err:.2e} (logits {refs[cs].min():.2f} .. {refs[cs].max():.2f})")
    lids, lmask = D.tokens(9, 40, "left", seed=3)
    left = rr.score({"input_ids": torch.from_numpy(lids), "attention_mask": torch.from_numpy(lmask)})
    assert torch.isfinite(left).all()
    rr.reranker._hip.check()
    print(f"[heads {heads} labels {labels}] worst |logit - HF fp32| over the end-to-end cases {worst:.3e} (bar {LOGIT_BAR})")
    assert worst <= LOGIT_BAR, worst


def test_train_mode_and_weight_sync(tmp_path):
    """train() mode is HF's own autograd forward on the same parameters; back in eval() an in-place update of either half of the head is followed"""
    rr, m, _ = _reranker(tmp_path, 4, labels=3, bm=(32, 128))
    ids, mask = D.tokens(5, 24, seed=2)
    args = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}
    ref = D.hf_logits(m, ids, mask)
    assert np.abs(rr.score(args).double().cpu().numpy() - ref).max() <= LOGIT_BAR
    rr.train()
    out = rr.reranker(**{k: v.cuda() for k, v in args.items()}).logits
    assert out.requires_grad and np.abs(out.detach().double().cpu().numpy() - ref).max() < 1e-4
    rr.eval()
    with torch.no_grad():
        rr.reranker.classifier.bias.add_(1.0)
    assert np.abs(rr.score(args).double().cpu().numpy() - (ref + 1.0)).max() <= LOGIT_BAR
    with torch.no_grad():
        rr.reranker.pooler.dense.bias.add_(0.5)          # the half of the head the weight sync would leave out as "pooler.*"
        m.pooler.dense.bias.add_(0.5); m.classifier.bias.add_(1.0)
    assert np.abs(rr.score(args).double().cpu().numpy() - D.hf_logits(m, ids, mask)).max() <= LOGIT_BAR


@pytest.mark.parametrize("H,heads,labels", [(128, 2, 1), (384, 6, 3), (1024, 16, 1), (2048, 32, 3)])
def test_head_kernel_inside_its_a_priori_fp32_bound(H, heads, labels, monkeypatch):
    """The erf-GELU variant of k_cls_head alone, whatever the encoder's error: on the library's OWN CLS rows x (kr_encoder_last_hidden of a KIRAG_AMD_CLS_FULL=1
    handle) the logits are within 2 x bound of the head evaluated in float64 — deberta_util.head_bound, derived as reranker_util.head_bound, not measured.
    One H per instantiation (NJ = 1, 2, 4, 8), one layer; B = 1, 4, 5, 9: one partial group, one full, full + 1, two full + 1.  The default handle (CLS
    shortcut) gives the same bits."""
    c, w = _model(heads, labels, (32, 128), layers=1, H=H)
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
    full = _hip(c, w)
    monkeypatch.delenv("KIRAG_AMD_CLS_FULL")
    short = _hip(c, w)
    assert full.num_labels == short.num_labels == labels
    for B in (1, 4, 5, 9):
        ids, mask = D.tokens(B, 20, seed=B)
        out = full.forward_np(ids, mask, POOL_CLASSIFY)
        x = full.last_hidden(B, 20).numpy()[:, 0]
        assert out.shape == (B, labels) and np.isfinite(out).all()
        ref, bound = D.head_bound(x, w)
        ratio = float((np.abs(out - ref) / bound).max())
        print(f"[H {H} L {labels} B {B}] worst |logit - logit64| / bound {ratio:.2e}, |logit - logit64| {np.abs(out - ref).max():.2e} (bound up to {bound.max():.2e})")
        assert ratio <= 2.0, (B, ratio)
        assert _same(short.forward_np(ids, mask, POOL_CLASSIFY), out), B


def test_invariance_pools_and_state():
    """each of 9 pairs alone == its row of the batch == its row of the reversed batch == kr_encoder_forward_packed, bit for bit; pools 0 / 1 of a handle with
    the head are the bits of a handle without it; KR_POOL_CLASSIFY without the head is KR_ESTATE"""
    from kirag_amd import _lib
    c, w = _model(2, 3)
    h = _hip(c, w)
    ids, mask = D.tokens(9, 40, seed=4)
    out = h.forward_np(ids, mask, POOL_CLASSIFY)
    assert out.shape == (9, 3) and np.ptp(out, axis=0).min() > 0.05
    assert _same(h.forward_np(ids[::-1].copy(), mask[::-1].copy(), POOL_CLASSIFY)[::-1].copy(), out)
    for r in range(9):
        assert _same(h.forward_np(ids[r:r + 1], mask[r:r + 1], POOL_CLASSIFY), out[r:r + 1]), r
    lens = mask.sum(1).astype(np.int32)
    toks = torch.from_numpy(np.concatenate([ids[r, :lens[r]] for r in range(9)]).astype(np.int32))
    assert _same(h.forward_packed(toks, torch.from_numpy(lens), 40, POOL_CLASSIFY).cpu().numpy(), out)
    plain = _hip(c, {k: v for k, v in w.items() if k not in D.HEAD})
    assert plain.num_labels == 0 and h.num_labels == 3 and h.out_dim == 128
    for S in (24, 150):
        ids, mask = D.tokens(5, S, seed=S)
        for pool in (POOL_MEAN, POOL_CLS):
            a, b = plain.forward_np(ids, mask, pool), h.forward_np(ids, mask, pool)
            assert a.shape == (5, 128) and np.allclose(np.linalg.norm(a, axis=1), 1.0, atol=1e-5) and _same(a, b), (S, pool)
    with pytest.raises(_lib.KiragAmdError) as ei:
        plain.forward_np(ids, mask, POOL_CLASSIFY)
    assert ei.value.code == KR_ESTATE


def test_ranking_through_rerank(tmp_path):
    """One query against 64 passages of mixed length through BaseReranker.rerank: every two passages whose HF fp32 logits differ by more than 2 x LOGIT_BAR
    come in HF's order.  Condition (HF alone, asserted): at most 10 % of the adjacent pairs of HF's order lie within 2 x LOGIT_BAR — the 64 are those of a pool
    of 512 random passages whose HF logits are most evenly spaced (reranker_util.spread_by_value), chosen by the reference before anything runs in the
    library.  batch_size 7 and 64 give identical scores."""
    tok = R.xlmr_pair_tokenizer()
    rr, m, _ = _reranker(tmp_path, 2, tokenizer=tok, maxlength=64)
    query, pool = "aa0 bb27 query", R.passages(512, seed=5)
    col = rr._collator()
    a = col.encode_pairs([query] * len(pool), pool)
    ps = [pool[i] for i in R.spread_by_value(D.hf_logits(m, a["input_ids"].numpy(), a["attention_mask"].numpy())[:, 0], 64)]
    assert len(set(ps)) == 64
    a = col.encode_pairs([query] * 64, ps)
    lens = a["attention_mask"].sum(1)
    assert int(lens.max()) > 40 and int(lens.min()) < 16 and len(set(lens.tolist())) > 20      # mixed lengths
    ref = D.hf_logits(m, a["input_ids"].numpy(), a["attention_mask"].numpy())[:, 0]
    gaps = -np.diff(np.sort(ref)[::-1])
    close = float((gaps <= 2 * LOGIT_BAR).mean())
    print(f"HF logits {ref.min():.4f} .. {ref.max():.4f}, median adjacent gap {np.median(gaps):.2e}; adjacent pairs within 2 x bar: {100 * close:.1f} %")
    assert close <= 0.10, close
    idx, scores = rr.rerank(query, ps, batch_size=64)
    idx7, scores7 = rr.rerank(query, ps, batch_size=7)
    assert torch.equal(idx, idx7) and torch.equal(scores, scores7)
    assert sorted(idx.tolist()) == list(range(64))
    got = np.empty(64); got[idx.numpy()] = scores.numpy()
    print(f"worst |score - HF| {np.abs(got - ref).max():.2e}")
    rank = np.empty(64, np.int64); rank[idx.numpy()] = np.arange(64)
    checked = 0
    for i in range(64):
        for j in range(64):
            if ref[i] - ref[j] > 2 * LOGIT_BAR:
                checked += 1
                assert rank[i] < rank[j], (i, j, ref[i], ref[j], got[i], got[j])
    assert checked >= 0.9 * 64 * 63 / 2, checked
    top, top_scores = rr.rerank(query, ps, top_k=5, batch_size=16)
    assert torch.equal(top, idx[:5]) and torch.equal(top_scores, scores[:5])


def test_checkpoint_check_tool_on_a_deberta_folder(tmp_path):
    """tools/checkpoint_check.py on a saved DeBERTa reranker folder and a saved encoder folder without a tokenizer: seeded random tokens, the worst
    |logit - HF fp32| / embedding deviation per precision mode"""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(repo, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    c, w = _model(2, 1, (32, 128))
    d = str(tmp_path / "rr")
    D.hf_classifier(c, w).save_pretrained(d)
    out = cc.check(d, cc.parse([d, "--n", "8", "--max-length", "48", "--random-tokens", "--json", str(tmp_path / "out.json")]))
    assert out["kind"] == "sequence-classification" and out["pairs"] == 8 and [m["operand_dtype"] for m in out["modes"]] == ["f16", "f16", "bf16", "bf16"]
    assert all(m["finite"] for m in out["modes"]) and out["modes"][0]["worst_logit_error"] <= LOGIT_BAR and os.path.exists(str(tmp_path / "out.json"))
    e = str(tmp_path / "enc")
    D.hf_model(c, w).save_pretrained(e)
    out = cc.check(e, cc.parse([e, "--n", "8", "--max-length", "48", "--random-tokens"]))
    assert all(m["finite"] for m in out["modes"]) and out["modes"][0]["operand_dtype"] == "f16"
