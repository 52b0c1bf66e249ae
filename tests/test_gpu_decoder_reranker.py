"""GPU tests of the decoder cross-encoders (Qwen2ForSequenceClassification / LlamaForSequenceClassification: the decoder stack, the row of the highest
attended column behind the final norm, score.weight without a bias — HEAD_SCORE, k_score_head and the last-row shortcut of KR_POOL_CLASSIFY on a decoder
handle).  The reference is the HF class in fp32 with eager attention on the CPU, on synthetic weights (tests/decoder_reranker_util.py).

Parity bar.  BAR = 2 x the worst |logit - HF fp32| measured on the MI355X over the parity cases below (both kinds, L 1 and 3, S 12 / 40 / 150 / 300, right
and left padding, holes, the ragged batch, the bidirectional case): worst 2.784e-3 (llama-64, L 3, S 40 left-padded), so BAR = 5.568e-3; HF's own bf16
forward (on the CPU) deviates from its fp32 forward by 2.8e-2 (qwen2-32) and 4.8e-2 (llama-64) on the same cases (profiles/decoder_reranker/measurements.txt).
The figures are printed, and appended to the file KIRAG_AMD_MEASUREMENTS_FILE names."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_reranker_util as U  # noqa: E402
import decoder_util as D  # noqa: E402

pytestmark = pytest.mark.gpu

KR_EINVAL, KR_ESTATE, KR_ERANGE = -22, -1, -34
MEASURED_WORST = 2.784e-3
BAR = 2 * MEASURED_WORST
POOL_MEAN, POOL_LAST, POOL_CLASSIFY = D.POOL_MEAN, D.POOL_LAST, U.POOL_CLASSIFY
NO_HEAD_MESSAGE = ("pool = 2 (KR_POOL_CLASSIFY) on a decoder handle: it takes KR_POOL_MEAN (0) and KR_POOL_LAST (5) — under a causal mask the first token sees itself "
                   "alone, and the handle has no head")
# (B, S, layout, holes, lens): S 300 runs k_attn_dma (as 150 does); 40 and 150 cross the 32-query tile and the 64-key step; the last one is the ragged batch
CASES = [(3, 12, "R", 0, None), (3, 12, "L", 0, None), (3, 40, "R", 0, None), (3, 40, "L", 0, None), (2, 150, "R", 0, None), (2, 150, "L", 0, None),
         (1, 300, "F", 0, None), (3, 40, "R", 2, None), (2, 150, "L", 2, None), (5, 64, "R", 0, (5, 7, 33, 1, 64))]


def _note(line):
    print(line)
    path = os.environ.get("KIRAG_AMD_MEASUREMENTS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _batch(i):
    B, S, layout, holes, lens = CASES[i]
    return U.pairs(B, S, layout, seed=100 + S + ord(layout) + holes, lens=lens, holes=holes)


@functools.lru_cache(maxsize=None)
def _hf(kind, labels):
    cfg = U.hf_config(kind, labels)
    return U.hf_classifier(cfg, U.weights(cfg))


@functools.lru_cache(maxsize=None)
def _ref(kind, labels, i):
    """HF's logits of case i, computed once and shared"""
    out = U.hf_logits(_hf(kind, labels), *_batch(i))
    out.setflags(write=False)
    return out


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


@pytest.fixture(scope="module")
def rerankers(tmp_path_factory):
    """(kind, labels, attention) -> BaseReranker on the GPU, from a saved ...ForSequenceClassification folder"""
    from kirag_amd.retriever.rerankers import BaseReranker
    cache = {}

    def get(kind, labels, attention="causal"):
        key = (kind, labels, attention)
        if key not in cache:
            d = str(tmp_path_factory.mktemp("decoder_reranker") / f"{kind}-{labels}")
            _hf(kind, labels).save_pretrained(d)
            cache[key] = BaseReranker("BGEReranker", d, reranker_kwargs={} if attention == "causal" else {"attention": attention}).to("cuda").eval()
        return cache[key]
    return get


def _raw(kind_or_cfg, labels=1, head=True, score=None):
    """a handle straight from the weights: the embedders' names plus score.weight"""
    from kirag_amd.retriever.encoders import HipBertForward
    cfg = U.hf_config(kind_or_cfg, labels) if isinstance(kind_or_cfg, str) else kind_or_cfg
    w = U.weights(cfg)
    if score is not None:
        w[U.SCORE_NAME] = score
    if not head:
        del w[U.SCORE_NAME]
    h = HipBertForward(cfg, 0)
    h.load_state(w)
    return h, w


def _score_args(ids, mask):
    return dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))


# ---------------------------------------------------------------------------------------------------------
# what fails without the feature
# ---------------------------------------------------------------------------------------------------------
def test_score_weight_loads_and_pool_2_runs_from_every_entry_point():
    """Without the feature "score.weight" is an unknown tensor name and pool 2 on a decoder handle is KR_EINVAL.  With it the three entry points agree bit
    for bit on [B, L]; the flags stay KR_EINVAL; a handle without the head answers as before, byte for byte."""
    from kirag_amd import _lib
    h, _ = _raw("qwen2-32", 3)
    assert h.is_decoder and h.num_labels == 3
    ids, mask = U.pairs(3, 20, "R", seed=1)
    B, S = ids.shape
    a = h.forward_np(ids, mask, POOL_CLASSIFY)
    b = h.forward_np(ids, mask, POOL_CLASSIFY, token_type_ids=np.zeros_like(ids))
    c = h.forward_packed(*_rag(ids, mask), S, POOL_CLASSIFY).cpu().numpy()
    assert a.shape == (B, 3) and np.isfinite(a).all() and _same(a, b) and _same(a, c)
    out = np.zeros((B, 3 + 2 * S * 128), np.float32)
    for flag in (0x10, 0x20):
        assert h._lib.kr_encoder_forward(h._h, ids.ctypes.data, mask.ctypes.data, B, S, POOL_CLASSIFY | flag, out.ctypes.data, None) == KR_EINVAL
        assert b"not with 2 (classify)" in h._lib.kr_last_error()
    bare, _ = _raw("qwen2-32", 3, head=False)
    with pytest.raises(_lib.KiragAmdError) as ei:
        bare.forward_np(ids, mask, POOL_CLASSIFY)
    assert ei.value.code == KR_EINVAL and NO_HEAD_MESSAGE in str(ei.value)
    assert bare._lib.kr_last_error().decode() == NO_HEAD_MESSAGE


# ---------------------------------------------------------------------------------------------------------
# parity with HF and its preconditions
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [1, 3])
@pytest.mark.parametrize("kind", U.KINDS)
def test_score_parity_with_hf(kind, labels, rerankers):
    """BaseReranker.score of a saved folder against the HF class (fp32, eager, CPU) on every case; the ragged batch through kr_encoder_forward_packed"""
    rr = rerankers(kind, labels)
    worst = 0.0
    for i, case in enumerate(CASES):
        ids, mask = _batch(i)
        ref = _ref(kind, labels, i)
        if case[4] is None:
            out = rr.score(_score_args(ids, mask)).float().cpu().numpy().reshape(ref.shape)
        else:
            out = rr.reranker._synced_hip().forward_packed(*_rag(ids, mask), ids.shape[1], POOL_CLASSIFY).cpu().numpy()
            assert _same(out, rr.score(_score_args(ids, mask)).cpu().numpy().reshape(ref.shape))
        err = float(np.abs(out - ref).max())
        worst = max(worst, err)
        print(f"[{kind} L {labels}] case {case}: max |logit - HF| {err:.3e}")
        assert np.isfinite(out).all() and err <= BAR, (case, err)
    _note(f"[{kind} L {labels}] logits vs HF fp32 eager over {len(CASES)} cases: worst {worst:.3e} (bar {BAR:.3e})")


def test_bidirectional_parity(rerankers):
    """attention="bidirectional": Qwen2Model under the 4-D mask that admits every attended key, then score.weight in float64"""
    rr = rerankers("qwen2-32", 3, "bidirectional")
    worst = 0.0
    for i in (2, 3, 5, 7):
        ids, mask = _batch(i)
        ref = U.reference_by_hand(_hf("qwen2-32", 3), ids, mask, rule="none")
        err = float(np.abs(rr.score(_score_args(ids, mask)).cpu().numpy() - ref).max())
        worst = max(worst, err)
        assert err <= BAR, (CASES[i], err)
    _note(f"[qwen2-32 L 3 bidirectional] logits vs Qwen2Model (all-admitting 4-D mask) + float64 head: worst {worst:.3e} (bar {BAR:.3e})")


@pytest.mark.parametrize("kind", U.KINDS)
def test_the_bar_has_teeth(kind):
    """preconditions on the reference: the normalised row, the mean row, the first row, the neighbour's last row, the row before the final norm and no
    causal mask each move some logit of the parity cases by more than 10 x the bar"""
    m = _hf(kind, 3)
    weakest = np.inf
    for name, (row, rule, how) in U.TEETH.items():
        moved = max(float(np.abs(U.reference_by_hand(m, *_batch(i), row=row, rule=rule, how=how) - _ref(kind, 3, i)).max()) for i in (2, 3, 4, 5, 9))
        print(f"[{kind}] {name}: moves a logit by {moved:.3f}")
        weakest = min(weakest, moved)
        assert moved > 10 * BAR, (name, moved)
    # the by-hand head on the right row IS HF's logit
    assert max(float(np.abs(U.reference_by_hand(m, *_batch(i)) - _ref(kind, 3, i)).max()) for i in (2, 9)) < 1e-4
    _note(f"[{kind}] weakest precondition distance {weakest:.3f} (required {10 * BAR:.3f})")


# ---------------------------------------------------------------------------------------------------------
# the head kernel alone
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [1, 3, 64])
@pytest.mark.parametrize("H", [128, 896, 2048])
def test_head_kernel_against_float64_on_the_library_s_own_rows(H, labels, monkeypatch):
    """logits against float64 score.weight . x, x = the rows kr_encoder_last_hidden returns on a KIRAG_AMD_CLS_FULL=1 handle, within the a-priori bound
    gamma_H sum |w_i x_i| of an fp32 sum of H products in any order"""
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
    h, w = _raw(U.wide_config(H, labels, L=2 if H == 128 else 1))
    ids, mask = U.pairs(5, 24, "R", seed=H + labels, lens=[24, 7, 1, 13, 20])
    out = h.forward_np(ids, mask, POOL_CLASSIFY).astype(np.float64)
    x = h.last_hidden(*ids.shape).numpy().astype(np.float64)[np.arange(len(ids)), D.last_index(mask)]
    W = w[U.SCORE_NAME].astype(np.float64)
    ref, bound = x @ W.T, U.gamma(H) * (np.abs(x) @ np.abs(W).T)
    ratio = float((np.abs(out - ref) / bound).max())
    print(f"[H {H} L {labels}] worst |logit - float64| / (gamma_H sum |w x|) = {ratio:.2e}")
    assert out.shape == (5, labels) and np.isfinite(out).all() and (np.abs(out - ref) <= bound).all(), ratio


# ---------------------------------------------------------------------------------------------------------
# the last-row shortcut
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", U.KINDS)
def test_shortcut_and_full_handles_agree_bit_for_bit(kind, monkeypatch):
    from kirag_amd import _lib
    short, _ = _raw(kind, 3)
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
    full, _ = _raw(kind, 3)
    monkeypatch.delenv("KIRAG_AMD_CLS_FULL")
    for i in (2, 3, 5, 7, 9):
        ids, mask = _batch(i)
        a, b = short.forward_np(ids, mask, POOL_CLASSIFY), full.forward_np(ids, mask, POOL_CLASSIFY)
        assert _same(a, b), CASES[i]
        with pytest.raises(_lib.KiragAmdError) as ei:
            short.last_hidden(*ids.shape)
        assert ei.value.code == KR_ESTATE and "KIRAG_AMD_CLS_FULL=1" in str(ei.value)
        assert np.isfinite(full.last_hidden(*ids.shape).numpy()).all()
        if CASES[i][2] == "R" and not CASES[i][3]:
            tok, lens = _rag(ids, mask)
            assert _same(short.forward_packed(tok, lens, ids.shape[1], POOL_CLASSIFY).cpu().numpy(), a)
            assert _same(full.forward_packed(tok, lens, ids.shape[1], POOL_CLASSIFY).cpu().numpy(), a)
    # the embedding pools keep every row: last_hidden answers after them on the shortcut handle too
    ids, mask = _batch(2)
    short.forward_np(ids, mask, POOL_LAST)
    assert np.isfinite(short.last_hidden(*ids.shape).numpy()).all()


# ---------------------------------------------------------------------------------------------------------
# invariance
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", U.KINDS)
def test_a_pair_s_logits_do_not_depend_on_the_batch_or_the_tiling(kind, monkeypatch):
    h, _ = _raw(kind, 3)
    ids, mask = U.pairs(6, 40, "R", seed=9, lens=[40, 17, 33, 5, 1, 26])
    S = ids.shape[1]
    base = h.forward_np(ids, mask, POOL_CLASSIFY)
    for b in range(len(ids)):
        assert _same(h.forward_np(ids[b:b + 1], mask[b:b + 1], POOL_CLASSIFY), base[b:b + 1]), b
    assert _same(h.forward_np(ids[::-1], mask[::-1], POOL_CLASSIFY), base[::-1])
    assert _same(h.forward_packed(*_rag(ids, mask), S, POOL_CLASSIFY).cpu().numpy(), base)
    for tile in (256, 130, 128, 64, 32):
        monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", str(tile))
        assert _same(h.forward_np(ids, mask, POOL_CLASSIFY), base), tile
    monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")


def test_64_passages_come_back_in_hf_s_order(rerankers):
    from kirag_amd.retriever.rerankers import rank_order
    ids, mask = U.pairs(64, 40, "R", seed=64)
    ref = U.hf_logits(_hf("qwen2-32", 1), ids, mask)[:, 0]
    out = rerankers("qwen2-32", 1).score(_score_args(ids, mask)).cpu().numpy()
    assert out.shape == (64,) and np.abs(out - ref).max() <= BAR
    i, j = np.triu_indices(64, 1)
    decided = np.abs(ref[i] - ref[j]) > 2 * BAR
    assert decided.sum() > 1000 and (np.sign(out[i] - out[j])[decided] == np.sign(ref[i] - ref[j])[decided]).all()
    pos = {int(p): r for r, p in enumerate(rank_order(out))}
    assert all((pos[a] < pos[b]) == (ref[a] > ref[b]) for a, b, d in zip(i, j, decided) if d)


# ---------------------------------------------------------------------------------------------------------
# nothing else moved
# ---------------------------------------------------------------------------------------------------------
def test_embedding_pools_masked_sequences_and_non_finite_weights():
    from kirag_amd import _lib
    h, w = _raw("qwen2-32", 3)
    bare, _ = _raw("qwen2-32", 3, head=False)
    ids, mask = _batch(2)
    for pool in (POOL_MEAN, POOL_LAST):
        a = h.forward_np(ids, mask, pool)
        assert a.shape == (len(ids), 128) and _same(a, bare.forward_np(ids, mask, pool)), pool
    # an all-masked sequence: a NaN row, its neighbours untouched, no error
    want = h.forward_np(ids, mask, POOL_CLASSIFY)
    m2 = mask.copy(); m2[1] = 0
    got = h.forward_np(ids, m2, POOL_CLASSIFY)
    assert np.isnan(got[1]).all() and _same(got[[0, 2]], want[[0, 2]])
    h.check()
    m0 = np.zeros_like(mask)
    assert np.isnan(h.forward_np(ids, m0, POOL_CLASSIFY)).all()
    # a NaN in score.weight: KR_ERANGE for pool 2 only
    bad = w[U.SCORE_NAME].copy(); bad[1, 5] = np.nan
    hb, _ = _raw("qwen2-32", 3, score=bad)
    for pool in (POOL_MEAN, POOL_LAST):
        assert _same(hb.forward_np(ids, mask, pool), bare.forward_np(ids, mask, pool))
    with pytest.raises(_lib.KiragAmdError) as ei:
        hb.forward_np(ids, mask, POOL_CLASSIFY)
    assert ei.value.code == KR_ERANGE
    assert np.isnan(hb.forward_np(ids, m0, POOL_CLASSIFY)).all()          # ... and not for sequences without attended tokens
