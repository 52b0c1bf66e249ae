"""Shared pieces of the ModernBERT reranker tests (tests/test_modernbert_reranker_host.py, tests/test_gpu_modernbert_reranker.py): configs of
ModernBertForSequenceClassification checkpoints, the synthetic backbones of modernbert_util.weights plus a seeded head under HF's own names (at
reranker_util.head's scales), the HF fp32 reference with eager attention, the head restated in float64 — whole, or with one part broken at a time (the teeth of
the end-to-end bar) —, (query, passage) token pairs, and the a-priori fp32 error bound of the head kernel.

The head (transformers.ModernBertForSequenceClassification):

    x      = last_hidden_state[:, 0]                                   classifier_pooling "cls"
           = sum of the attended rows / their number                    classifier_pooling "mean"
    t      = LayerNorm_{norm_eps}(gelu(head.dense.weight . x + head.dense.bias)) * head.norm.weight + head.norm.bias        (erf GELU; biased variance)
    logits = classifier.weight . t + classifier.bias
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modernbert_util as M  # noqa: E402
import reranker_util as R  # noqa: E402

VOCAB = R.VOCAB
LAYERS, FF, LOCAL_ATTENTION = 3, 256, 128
TYPES = (M.FULL, M.SLIDING, M.SLIDING)
HEAD = ("head.dense.weight", "head.dense.bias", "head.norm.weight", "head.norm.bias", "classifier.weight", "classifier.bias")
HEAD_REQUIRED = (HEAD[0], HEAD[2], HEAD[4], HEAD[5])
HEAD_OPTIONAL = (HEAD[1], HEAD[3])
POOLING_NAME = "config.classifier_pooling"
POOLINGS = {"cls": 0.0, "mean": 1.0}
PAD, CLS, SEP = 0, 1, 2               # modernbert_util.cfg's special ids


def cfg(H, heads, labels=1, pooling="cls", biases=False, layers=LAYERS, ff=FF, types=None, **extra):
    """`biases`: classifier_bias (head.dense.bias) and norm_bias (head.norm.bias — and every LayerNorm bias of the backbone, which stay zero)"""
    if types is None:
        types = TYPES if layers == LAYERS else M.layer_types(layers)
    return M.cfg(H, layers, heads, ff, VOCAB, types=types, local_attention=LOCAL_ATTENTION, classifier_pooling=pooling, classifier_bias=biases,
                 norm_bias=biases, classifier_activation="gelu", classifier_dropout=0.0, num_labels=labels, **extra)


def head(H, labels, biases=False, seed=21, dense_scale=1.0, out_scale=4.0):
    """The head's tensors, seeded normal, at reranker_util.head's scales: Wd ~ N(0, dense_scale^2 / H) puts the GELU's argument at unit scale (where it bends),
    bd ~ N(0, 0.5^2); Wo ~ N(0, out_scale^2 / H) spreads the logits over several units and bo ~ N(0, 1) is visible next to them.  The LayerNorm's weight is
    1 + 0.5 N(0, 1) — a scale that is visibly not 1 — and its bias N(0, 0.5^2)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s)
    w = {HEAD[0]: f(H, H) * dense_scale / np.sqrt(H), HEAD[1]: 0.5 * f(H), HEAD[2]: 1.0 + 0.5 * f(H), HEAD[3]: 0.5 * f(H),
         HEAD[4]: f(labels, H) * out_scale / np.sqrt(H), HEAD[5]: f(labels)}
    if not biases:
        del w[HEAD[1]], w[HEAD[3]]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def weights(H, labels=1, biases=False, layers=LAYERS, ff=FF, with_head=True, pooling=None, **head_kw):
    """library names: the backbone of modernbert_util.weights + the head (+ the pooling setting when `pooling` is given)"""
    w = dict(M.weights(H, layers, ff, VOCAB))
    if with_head:
        w.update(head(H, labels, biases, **head_kw))
        if pooling is not None:
            w[POOLING_NAME] = np.array([POOLINGS[pooling]], np.float32)
    return w


def hf_state(w):
    """the library-named tensors under ModernBertForSequenceClassification's own names (the settings stay behind)"""
    return {(k if k in HEAD else "model." + k): torch.from_numpy(np.asarray(v)) for k, v in w.items() if not k.startswith("config.")}


def hf_classifier(c, w, device="cpu", cls=None):
    """the HF task model in fp32 (eager attention) holding `w`; LayerNorm biases that `w` does not name stay zero"""
    from transformers import ModernBertForSequenceClassification
    m = (cls or ModernBertForSequenceClassification)(M.hf_config(c))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.bias"):
                p.zero_()
    res = m.load_state_dict(hf_state(w), strict=False)
    assert not res.unexpected_keys and all(k.endswith("norm.bias") for k in res.missing_keys), res
    return m.float().eval().to(device)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@torch.no_grad()
def hf_logits(m, ids, mask):
    dev = next(m.parameters()).device
    return m(input_ids=_t(ids, dev), attention_mask=_t(mask, dev)).logits.double().cpu().numpy()


@torch.no_grad()
def hf_last_hidden(m, ids, mask):
    dev = next(m.parameters()).device
    return m.model(input_ids=_t(ids, dev), attention_mask=_t(mask, dev)).last_hidden_state.double().cpu().numpy()


def head_tensors(m):
    """the six tensors of an HF task model in float64 (absent biases: zeros)"""
    H = m.config.hidden_size
    g = lambda p: np.zeros(H) if p is None else p.detach().double().cpu().numpy()
    return {HEAD[0]: g(m.head.dense.weight), HEAD[1]: g(m.head.dense.bias), HEAD[2]: g(m.head.norm.weight), HEAD[3]: g(m.head.norm.bias),
            HEAD[4]: g(m.classifier.weight), HEAD[5]: g(m.classifier.bias)}


def gelu64(a):
    return 0.5 * a * (1.0 + np.vectorize(math.erf)(a / math.sqrt(2.0)))


def head64(x, w, eps, broken=None):
    """the head in float64 on the rows x [B, H]; `w`: the six tensors (a missing bias is zero).  broken: "no_norm", "tanh", "no_classifier_bias",
    "no_norm_scale" — one part of the formula changed"""
    g = lambda k: np.asarray(w[k], np.float64) if k in w else 0.0
    a = np.asarray(x, np.float64) @ g(HEAD[0]).T + g(HEAD[1])
    y = np.tanh(a) if broken == "tanh" else gelu64(a)
    if broken != "no_norm":
        d = y - y.mean(-1, keepdims=True)
        y = d / np.sqrt((d * d).mean(-1, keepdims=True) + eps) * (1.0 if broken == "no_norm_scale" else g(HEAD[2])) + g(HEAD[3])
    return y @ g(HEAD[4]).T + (0.0 if broken == "no_classifier_bias" else g(HEAD[5]))


def pooled_rows(lh, mask, pooling):
    lh, mk = np.asarray(lh, np.float64), (np.asarray(mask) != 0).astype(np.float64)
    return lh[:, 0] if pooling == "cls" else (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None]


MUTATIONS = ("no_norm", "tanh", "no_classifier_bias", "no_norm_scale", "other_pooling", "normalised_row", "neighbour_row")


def head_by_hand(m, ids, mask, broken=None):
    """The float64 head on the HF backbone's last_hidden_state: whole (`broken=None`: must reproduce the task model's logits) or with one part broken — the
    four of head64, the OTHER pooling's row (the CLS row under "mean", the mean row under "cls"), the L2-normalised row, the neighbouring sequence's row"""
    pooling = m.config.classifier_pooling
    lh = hf_last_hidden(m, ids, mask)
    x = pooled_rows(lh, mask, ({"cls": "mean", "mean": "cls"}[pooling]) if broken == "other_pooling" else pooling)
    if broken == "normalised_row":
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    if broken == "neighbour_row":
        x = np.roll(x, 1, axis=0)
    return head64(x, head_tensors(m), m.config.norm_eps, broken if broken in MUTATIONS[:4] else None)


def pairs(B, S, side="right", seed=0, min_len=8):
    """(ids, mask) [B, S] int64 of B (query, passage) pairs [CLS] q [SEP] p [SEP] with pad 0 — ModernBERT has no token types.  Row 0 has full length, the
    others between min_len and S tokens; `side`: where the padding goes."""
    rng = np.random.default_rng(seed)
    ids = np.full((B, S), PAD, np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        n = S if r == 0 else int(rng.integers(min_len, S + 1))
        nq = int(rng.integers(1, max(2, min(12, n - 4))))
        npass = n - 3 - nq
        assert npass >= 1
        row = [CLS, *rng.integers(10, VOCAB, nq), SEP, *rng.integers(10, VOCAB, npass), SEP]
        sl = slice(0, n) if side == "right" else slice(S - n, S)
        ids[r, sl] = row; mask[r, sl] = 1
    return ids, mask


E2E_CASES = [(S, side) for S in (12, 40, 150) for side in ("right", "left")]


def e2e_pairs(S, side, B=5):
    """The pairs of one end-to-end case.  A left-padded batch under "cls" pooling reads the row of a MASKED column 0; where that column's window of +- 64 holds
    no attended column, HF's row is an artefact of its finite mask value (a uniform average over every column, padding included: tests/test_gpu_modernbert.py),
    so the left-padded S = 150 pairs hold at least 150 - 64 tokens: every row's reference is defined, and four of the five still have a masked column 0."""
    return pairs(B, S, side, seed=S, min_len=S - LOCAL_ATTENTION // 2 if (side == "left" and S > LOCAL_ATTENTION // 2 + 8) else 8)


def head_bound(x, w, eps, x_err=0.0):
    """(logit64, bound): the head in float64 on the rows x [B, H], and an a-priori bound of an fp32 evaluation — derived, not measured.  u = 2^-24,
    gamma = (H + 2) u bounds the relative error of an H-term fp32 sum plus its bias, in any order.

      a_j = Wd_j . x + bd_j                  e_a_j = gamma (|Wd_j| . |x| + |bd_j|) + |Wd_j| . x_err     (x_err: what the rows handed to the kernel may differ from x by)
      y_j = gelu(a_j)                        e_y_j = 1.13 e_a_j + 8 u (|y_j| + |a_j|) + 4 u       (|gelu'| <= 1.13; erff, its argument's and the products' roundings)
      m   = sum_j y_j / H                    e_m   = mean_j e_y_j + gamma mean_j |y_j|
      d_j = y_j - m                          e_d_j = e_y_j + e_m + u |d_j|
      v   = sum_j d_j^2 / H                  e_v   = mean_j (2 |d_j| e_d_j + e_d_j^2) + gamma v       (the centred second pass: no cancellation)
      r   = 1 / sqrt(v + eps)                rel_r = e_v / (2 (v + eps)) + 3 u                        (v: the variance of the case, floored by eps)
      t_j = d_j r g_j + b_j                  e_t_j = |g_j| r (e_d_j + |d_j| (rel_r + 3 u)) + u |t_j|
      logit_l = Wo_l . t + bo_l              bound_l = sum_j |Wo_lj| e_t_j + gamma (sum_j |Wo_lj| |t_j| + |bo_l|)
    """
    g = lambda k: np.asarray(w[k], np.float64) if k in w else 0.0
    Wd, bd, ng, nb, Wo, bo = (g(k) for k in HEAD)
    x = np.asarray(x, np.float64)
    H = x.shape[1]
    u = 2.0 ** -24
    gm = (H + 2) * u
    a = x @ Wd.T + bd
    e_a = gm * (np.abs(x) @ np.abs(Wd).T + np.abs(bd)) + (np.zeros_like(x) + x_err) @ np.abs(Wd).T
    y = gelu64(a)
    e_y = 1.13 * e_a + 8 * u * (np.abs(y) + np.abs(a)) + 4 * u
    m = y.mean(-1, keepdims=True)
    e_m = e_y.mean(-1, keepdims=True) + gm * np.abs(y).mean(-1, keepdims=True)
    d = y - m
    e_d = e_y + e_m + u * np.abs(d)
    v = (d * d).mean(-1, keepdims=True)
    e_v = (2 * np.abs(d) * e_d + e_d * e_d).mean(-1, keepdims=True) + gm * v
    r = 1.0 / np.sqrt(v + eps)
    rel_r = e_v / (2 * (v + eps)) + 3 * u
    t = d * r * ng + nb
    e_t = np.abs(ng) * r * (e_d + np.abs(d) * (rel_r + 3 * u)) + u * np.abs(t)
    logit = t @ Wo.T + bo
    bound = e_t @ np.abs(Wo).T + gm * (np.abs(t) @ np.abs(Wo).T + np.abs(bo))
    return logit, bound


def pair_tokenizer(padding_side="right"):
    """a word-level tokenizer over xlmr_util's 200 toy words with ModernBERT's pair template [CLS] A [SEP] B [SEP], pad 0, and no token types"""
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    from transformers import PreTrainedTokenizerFast
    import xlmr_util as X
    vocab = {"[PAD]": PAD, "[CLS]": CLS, "[SEP]": SEP, "[UNK]": 3}
    for extra in (":", ",", "query", "passage", "and", "of"):
        vocab.setdefault(extra, len(vocab))
    for wd in X.toy_words():
        vocab.setdefault(wd, len(vocab))
    t = Tokenizer(WordLevel(vocab, unk_token="[UNK]"))
    t.pre_tokenizer = Whitespace()
    t.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]", special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    tok = PreTrainedTokenizerFast(tokenizer_object=t, unk_token="[UNK]", pad_token="[PAD]", cls_token="[CLS]", sep_token="[SEP]", padding_side=padding_side,
                                  model_input_names=["input_ids", "attention_mask"])       # as ModernBERT's tokenizer declares them: no token types
    assert tok.pad_token_id == PAD and tok.vocab_size == VOCAB, tok.vocab_size
    return tok
