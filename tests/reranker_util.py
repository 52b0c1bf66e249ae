"""Shared pieces of the cross-encoder reranker tests (tests/test_reranker_host.py, tests/test_gpu_reranker.py): synthetic backbones (oracle.encoder_np's
weights, as tests/xlmr_util.py) with a seeded classification head under the library's names, the HF fp32 references (XLMRobertaForSequenceClassification /
BertForSequenceClassification, eager attention), the head restated with one part broken at a time (the teeth of the end-to-end bar), (query, passage) token
pairs of both families, the a-priori fp32 error bound of the head kernel, and toy pair tokenizers."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xlmr_util as X  # noqa: E402

from oracle import encoder_np as E  # noqa: E402

VOCAB = 210
MAX_POS = 200                       # tokens; XLM-R's table has MAX_POS + 2 rows
HEAD = ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias")
# BERT's special ids in the 210-word toy vocabulary
B_PAD, B_UNK, B_CLS, B_SEP = 0, 1, 2, 3


def cfg(kind, H, layers, heads, FF, labels=1):
    if kind == "xlmr":
        c = X.cfg(H, layers, heads, FF, VOCAB, MAX_POS + 2)
    else:
        c = SimpleNamespace(hidden_size=H, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=FF, vocab_size=VOCAB,
                            max_position_embeddings=MAX_POS, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", model_type="bert", pad_token_id=B_PAD)
    c.num_labels = labels
    return c


def head(H, labels, seed=21, dense_scale=1.0, out_scale=4.0):
    """The four head tensors, seeded normal.  x (a LayerNorm output) has unit-scale elements: Wd ~ N(0, dense_scale^2 / H) puts tanh's argument at unit scale
    (where the tanh bends), bd ~ N(0, 0.5^2) is visible next to it; Wo ~ N(0, out_scale^2 / H) spreads the logits over several units and bo ~ N(0, 1) is
    visible next to them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s)
    w = {HEAD[0]: f(H, H) * dense_scale / np.sqrt(H), HEAD[1]: 0.5 * f(H), HEAD[2]: f(labels, H) * out_scale / np.sqrt(H), HEAD[3]: f(labels)}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def weights(kind, H, layers, FF, labels=1, seed=3, with_head=True, **head_kw):
    """backbone (library names: oracle.encoder_np's synthetic weights as they are) + head"""
    if kind == "xlmr":
        w = X.weights(H, layers, FF, VOCAB, MAX_POS + 2, seed=seed)
    else:
        w = dict(E.synth_weights(H, layers, FF, VOCAB, MAX_POS, seed=seed))
    if with_head:
        w.update(head(H, labels, **head_kw))
    return w


def hf_state(kind, w):
    """the library-named tensors under the HF task model's own names"""
    out = {}
    for k, v in w.items():
        if kind == "xlmr":
            name = k if k in HEAD else "roberta." + k
        else:
            name = {HEAD[0]: "bert.pooler.dense.weight", HEAD[1]: "bert.pooler.dense.bias", HEAD[2]: "classifier.weight", HEAD[3]: "classifier.bias"}.get(k, "bert." + k)
        out[name] = torch.from_numpy(np.asarray(v))
    return out


def hf_config(kind, c):
    from transformers import BertConfig, XLMRobertaConfig
    kw = dict(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
              vocab_size=c.vocab_size, max_position_embeddings=c.max_position_embeddings, num_labels=c.num_labels, attn_implementation="eager",
              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    if kind == "xlmr":
        return XLMRobertaConfig(type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=X.PAD, bos_token_id=0, eos_token_id=2, **kw)
    return BertConfig(type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=B_PAD, **kw)


def hf_classifier(kind, c, w, device="cpu", cls=None):
    """the HF task model in fp32 holding `w` (`cls`: another class over the same parameters, e.g. the library's twin)"""
    from transformers import BertForSequenceClassification, XLMRobertaForSequenceClassification
    cls = cls or (XLMRobertaForSequenceClassification if kind == "xlmr" else BertForSequenceClassification)
    m = cls(hf_config(kind, c))
    res = m.load_state_dict(hf_state(kind, w), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@torch.no_grad()
def hf_logits(m, ids, mask, tt=None):
    dev = next(m.parameters()).device
    kw = {} if tt is None else {"token_type_ids": _t(tt, dev)}
    return m(input_ids=_t(ids, dev), attention_mask=_t(mask, dev), **kw).logits.double().cpu().numpy()


MUTATIONS = ("no_tanh", "no_bd", "no_bo", "mean_row", "normalised_row")


@torch.no_grad()
def head_by_hand(kind, m, ids, mask, tt=None, broken=None):
    """The head applied by hand to the HF backbone's last_hidden_state (fp32), whole (`broken=None`: must reproduce the task model's logits) or with one part
    broken: the tanh dropped, bd dropped, bo dropped, the masked MEAN row in place of the CLS row, the L2-normalised CLS row."""
    dev = next(m.parameters()).device
    back = m.roberta if kind == "xlmr" else m.bert
    kw = {} if tt is None else {"token_type_ids": _t(tt, dev)}
    k = _t(mask, dev)
    lh = back(input_ids=_t(ids, dev), attention_mask=k, **kw).last_hidden_state
    if kind == "xlmr":
        Wd, bd, Wo, bo = m.classifier.dense.weight, m.classifier.dense.bias, m.classifier.out_proj.weight, m.classifier.out_proj.bias
    else:
        Wd, bd, Wo, bo = m.bert.pooler.dense.weight, m.bert.pooler.dense.bias, m.classifier.weight, m.classifier.bias
    x = lh[:, 0]
    if broken == "mean_row":
        x = (lh * k[..., None]).sum(1) / k.sum(1)[..., None]
    if broken == "normalised_row":
        x = torch.nn.functional.normalize(x, dim=-1)
    t = x @ Wd.T + (0 if broken == "no_bd" else bd)
    if broken != "no_tanh":
        t = torch.tanh(t)
    return (t @ Wo.T + (0 if broken == "no_bo" else bo)).double().cpu().numpy()


def pairs(kind, B, S, side="right", seed=0, min_len=8):
    """(ids, mask, tt) [B, S] int64 of B (query, passage) pairs: <s> q </s></s> p </s> with pad 1 (tt None), or [CLS] q [SEP] p [SEP] with pad 0 and token types
    0…0 1…1.  Row 0 has full length; the others between min_len and S tokens; `side`: where the padding goes."""
    rng = np.random.default_rng(seed)
    pad = X.PAD if kind == "xlmr" else B_PAD
    ids = np.full((B, S), pad, np.int64); mask = np.zeros((B, S), np.int64); tt = np.zeros((B, S), np.int64)
    for r in range(B):
        n = S if r == 0 else int(rng.integers(min_len, S + 1))
        extra = 4 if kind == "xlmr" else 3
        nq = int(rng.integers(1, max(2, min(12, n - extra - 1))))
        npass = n - extra - nq
        assert npass >= 1
        q, p = rng.integers(10, VOCAB, nq), rng.integers(10, VOCAB, npass)
        if kind == "xlmr":
            row = [0, *q, 2, 2, *p, 2]; types = [0] * n
        else:
            row = [B_CLS, *q, B_SEP, *p, B_SEP]; types = [0] * (nq + 2) + [1] * (npass + 1)
        sl = slice(0, n) if side == "right" else slice(S - n, S)
        ids[r, sl] = row; mask[r, sl] = 1; tt[r, sl] = types
    return ids, mask, (None if kind == "xlmr" else tt)


def head_bound(x, w):
    """(logit64, bound): the head in float64 on the rows x [B, H], and the a-priori bound of an fp32 evaluation with u = 2^-24, gamma = (H + 2) u (any order of
    an H-term sum plus its bias), A_j = sum_i |Wd_ji x_i| + |bd_j|, e_j = gamma A_j + 4u (tanh's slope is at most 1; 4u for tanhf itself and the rounding of its
    argument), bound_l = sum_j |Wo_lj| e_j + gamma (sum_j |Wo_lj| + |bo_l|) (|t_j| <= 1)."""
    Wd, bd, Wo, bo = (np.asarray(w[k], np.float64) for k in HEAD)
    x = np.asarray(x, np.float64)
    H = x.shape[1]
    u = 2.0 ** -24
    g = (H + 2) * u
    logit = np.tanh(x @ Wd.T + bd) @ Wo.T + bo
    A = np.abs(x) @ np.abs(Wd).T + np.abs(bd)
    e = g * A + 4 * u
    bound = e @ np.abs(Wo).T + g * (np.abs(Wo).sum(1) + np.abs(bo))
    return logit, bound


def _fast(t, **kw):
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast(tokenizer_object=t, **kw)


def xlmr_pair_tokenizer(padding_side="right"):
    """tests/xlmr_util's word-level tokenizer (XLM-R's special ids, 210 entries) with XLM-R's pair template <s> A </s></s> B </s>"""
    from tokenizers.processors import TemplateProcessing
    tok = X.toy_tokenizer(padding_side=padding_side)
    tok._tokenizer.post_processor = TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    assert tok.vocab_size == VOCAB
    return tok


def bert_pair_tokenizer():
    """a WordPiece tokenizer over the same 200 words (+ a few ## pieces) with BERT's pair template and token types"""
    from tokenizers import Tokenizer
    from tokenizers.models import WordPiece
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    vocab = {"[PAD]": B_PAD, "[UNK]": B_UNK, "[CLS]": B_CLS, "[SEP]": B_SEP}
    for extra in ("##s", "##ed", "##ing", ":", ",", "query"):
        vocab.setdefault(extra, len(vocab))
    for wd in X.toy_words():
        vocab.setdefault(wd, len(vocab))
    t = Tokenizer(WordPiece(vocab, unk_token="[UNK]"))
    t.pre_tokenizer = Whitespace()
    t.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1", special_tokens=[("[CLS]", B_CLS), ("[SEP]", B_SEP)])
    tok = _fast(t, unk_token="[UNK]", pad_token="[PAD]", cls_token="[CLS]", sep_token="[SEP]",
                model_input_names=["input_ids", "token_type_ids", "attention_mask"])     # as BertTokenizerFast declares them
    assert tok.pad_token_id == B_PAD and tok.vocab_size == VOCAB
    return tok


def spread_by_value(logits, n=64):
    """n indices into `logits`, in descending order of value, with the largest minimum gap between neighbours that a greedy walk down the sorted pool reaches
    (bisection on the gap): the well-separated subset of a pool of candidates"""
    v = np.asarray(logits, np.float64)
    order = np.argsort(-v, kind="stable")

    def walk(g):
        out = [order[0]]
        for i in order[1:]:
            if v[out[-1]] - v[i] >= g:
                out.append(i)
        return out

    lo, hi = 0.0, (v.max() - v.min()) / (n - 1)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if len(walk(mid)) >= n else (lo, mid)
    return np.array(walk(lo)[:n])


def passages(n, seed=0, lo=3, hi=60):
    """n texts of lo..hi toy words"""
    rng = np.random.default_rng(seed)
    words = X.toy_words()
    return [" ".join(words[i] for i in rng.integers(0, len(words), int(rng.integers(lo, hi + 1)))) for _ in range(n)]
