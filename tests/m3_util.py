"""Shared pieces of the bge-m3 head tests (tests/test_m3_host.py, tests/test_gpu_m3.py): synthetic backbones of both families (oracle.encoder_np's weights,
as tests/xlmr_util.py / tests/reranker_util.py) with seeded ``colbert_linear`` / ``sparse_linear`` tensors, the HF fp32 reference (XLMRobertaModel / BertModel,
eager attention) with the two heads restated in torch fp64 — whole, or with one part broken at a time (the teeth) —, padded batches with right padding, left
padding and holes, and the reference's own lexical weights / MaxSim / hybrid scores for the end-to-end tests."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xlmr_util as X  # noqa: E402

from oracle import encoder_np as E  # noqa: E402

VOCAB = 256
MAX_POS = 200                       # tokens; XLM-R's table has MAX_POS + 2 rows
HEADS = ("colbert_linear.weight", "colbert_linear.bias", "sparse_linear.weight", "sparse_linear.bias")
B_PAD, B_UNK, B_CLS, B_SEP = 0, 1, 2, 3
# (H, layers, heads, FF): 2 heads of 64 on the XLM-R backbone, 4 heads of 32 on the BERT one
SHAPES = {"xlmr": (128, 2, 2, 256), "bert": (128, 1, 4, 256)}
# Bars: twice the worst value measured over the parity cases of tests/test_gpu_m3.py (every family, padding variant, S and P) against the fp32 reference on one
# MI355X, rounded up to two significant digits (profiles/m3/measurements.txt, section 1).  The kernels are deterministic; the factor covers reordering noise
# between runs of the HF side.  Scores: the project's 1e-3 score tolerance.
# measured worst: 1 - cos 1.0604e-07, |element| 1.8116e-04 (the 16-bit store of the product behind the head: half an f16 ulp of an element near 10 over a norm
# near 34), |weight| 9.9722e-06
BARS = {"colbert_cos": 2.2e-7, "colbert_elem": 3.7e-4, "sparse": 2.0e-5}
SCORE_BAR = 1e-3
MUTATIONS = ("no_colbert_bias", "no_norm", "neighbour_row", "no_sparse_bias", "no_relu")


def cfg(kind, H, layers, heads, FF):
    if kind == "xlmr":
        return X.cfg(H, layers, heads, FF, VOCAB, MAX_POS + 2)
    return SimpleNamespace(hidden_size=H, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=FF, vocab_size=VOCAB,
                           max_position_embeddings=MAX_POS, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", model_type="bert", pad_token_id=B_PAD)


def heads(H, P, seed=31, colbert_scale=3.0, colbert_bias=1.0, sparse_scale=0.1, sparse_bias=0.0):
    """The four head tensors, seeded normal.  x (a LayerNorm output) has unit-scale elements.  colbert: W ~ N(0, colbert_scale^2 / H) gives vectors of norm about
    colbert_scale sqrt(P) — far from 1, so a missing normalisation shows — and b ~ N(0, colbert_bias^2) turns every vector visibly.  sparse: w ~ N(0,
    sparse_scale^2 / H) puts the weights at a fraction of 1, where a real checkpoint's lexical weights are; the bias proper comes from heads_for."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s)
    w = {HEADS[0]: f(P, H) * colbert_scale / np.sqrt(H), HEADS[1]: colbert_bias * f(P), HEADS[2]: f(1, H) * sparse_scale / np.sqrt(H),
         HEADS[3]: np.array([sparse_bias])}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def backbone(kind, seed=3):
    H, layers, _, FF = SHAPES[kind]
    if kind == "xlmr":
        return X.weights(H, layers, FF, VOCAB, MAX_POS + 2, seed=seed)
    return dict(E.synth_weights(H, layers, FF, VOCAB, MAX_POS, seed=seed))


def hf_config(kind, c):
    from transformers import BertConfig, XLMRobertaConfig
    kw = dict(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
              vocab_size=c.vocab_size, max_position_embeddings=c.max_position_embeddings, attn_implementation="eager", hidden_dropout_prob=0.0,
              attention_probs_dropout_prob=0.0)
    if kind == "xlmr":
        return XLMRobertaConfig(type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=X.PAD, bos_token_id=0, eos_token_id=2, **kw)
    return BertConfig(type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=B_PAD, **kw)


def hf_backbone(kind, w, device="cpu", cls=None):
    """the HF model in fp32 (eager attention) holding the backbone tensors of `w` (`cls`: another class over the same parameters, e.g. the library's twin)"""
    from transformers import BertModel, XLMRobertaModel
    cls = cls or (XLMRobertaModel if kind == "xlmr" else BertModel)
    m = cls(hf_config(kind, cfg(kind, *SHAPES[kind])), add_pooling_layer=False)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items() if k not in HEADS}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


def batch(kind, B, S, variant="right", seed=0, min_len=4):
    """(ids, mask) [B, S] int64.  Row 0 has full length, the others min_len .. S tokens: <s> w .. </s> with pad 1, or [CLS] w .. [SEP] with pad 0.  variant:
    "right" / "left" = where the padding goes; "holes" = right padding with up to a third of each row's interior columns masked (their ids stay) and, in every
    second row, column 0 masked too."""
    rng = np.random.default_rng(seed)
    pad, first, last = (X.PAD, 0, 2) if kind == "xlmr" else (B_PAD, B_CLS, B_SEP)
    ids = np.full((B, S), pad, np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        n = S if r == 0 else int(rng.integers(min_len, S + 1))
        row = [first, *rng.integers(10, VOCAB, n - 2), last]
        sl = slice(S - n, S) if variant == "left" else slice(0, n)
        ids[r, sl] = row; mask[r, sl] = 1
        if variant == "holes":
            inner = np.arange(1, n - 1)
            mask[r, rng.choice(inner, size=len(inner) // 3, replace=False)] = 0
            if r % 2 == 1:
                mask[r, 0] = 0
    return ids, mask


_CACHE = {}


def heads_for(kind, P):
    """heads(H, P) with the sparse bias moved so that the ReLU cuts through the middle of THIS backbone's tokens: the synthetic rows share a common component,
    which puts w . x of every token on one side of 0.  bias = sparse_bias - median(w . x) over a probe batch of the reference (CPU); tests assert the shares."""
    if (kind, P) not in _CACHE:
        hw = heads(SHAPES[kind][0], P)
        ids, mask = batch(kind, 5, 40, "right", seed=123)
        lh = last_hidden(hf_backbone(kind, backbone(kind)), ids, mask)
        pre = (lh @ torch.from_numpy(hw[HEADS[2]].astype(np.float64)).T).squeeze(-1).numpy()[mask != 0]
        hw[HEADS[3]] = np.array([float(hw[HEADS[3]][0]) - float(np.median(pre))], np.float32)
        _CACHE[(kind, P)] = hw
    return _CACHE[(kind, P)]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@torch.no_grad()
def last_hidden(m, ids, mask):
    dev = next(m.parameters()).device
    return m(input_ids=_t(ids, dev), attention_mask=_t(mask, dev)).last_hidden_state.double().cpu()


def ref_blocks(lh, mask, hw, broken=None):
    """(sparse [B, S], colbert [B, S, P]) float64 from last_hidden_state `lh` [B, S, H] (torch float64): the two heads as the issue states them, masked columns
    zero — whole, or with ONE part broken (MUTATIONS)."""
    Wc, bc, ws, bs = (torch.from_numpy(np.asarray(hw[k], np.float64)) for k in HEADS)
    k = torch.from_numpy(np.asarray(mask)).bool()
    x = lh
    if broken == "neighbour_row":
        x = torch.roll(lh, 1, dims=1)
    v = x @ Wc.T + (0 if broken == "no_colbert_bias" else bc)
    if broken != "no_norm":
        v = torch.nn.functional.normalize(v, dim=-1, eps=1e-12)
    s = (x @ ws.T).squeeze(-1) + (0 if broken == "no_sparse_bias" else bs)
    if broken != "no_relu":
        s = torch.relu(s)
    return (s * k).numpy(), (v * k[..., None]).numpy()


def colbert_errors(got, ref, mask):
    """(worst 1 - cos, worst |element difference|) over the attended tokens"""
    k = np.asarray(mask) != 0
    g, r = np.asarray(got, np.float64)[k], np.asarray(ref, np.float64)[k]
    cos = (g * r).sum(-1) / np.maximum(np.linalg.norm(g, axis=-1) * np.linalg.norm(r, axis=-1), 1e-300)
    return float((1.0 - cos).max()), float(np.abs(g - r).max())


# ---- the reference's own end-to-end arithmetic (restated here, not imported from the package) ----
def ref_encode(m, hw, tok, sentences, max_length=512):
    """per sentence: (dense [H], lexical weights {str(id): max weight}, token vectors [len - 1, P], ids [len], w . x + b BEFORE the ReLU [len]) from the HF model +
    fp64 heads on ONE padded batch"""
    enc = tok(list(sentences), padding=True, truncation=True, max_length=max_length, return_tensors="np")
    ids, mask = enc["input_ids"].astype(np.int64), enc["attention_mask"].astype(np.int64)
    lh = last_hidden(m, ids, mask)
    sparse, colbert = ref_blocks(lh, mask, hw)
    pre = ref_blocks(lh, mask, hw, broken="no_relu")[0]
    dense = torch.nn.functional.normalize(lh[:, 0], dim=-1).numpy()
    skip = {tok.cls_token_id, tok.eos_token_id, tok.pad_token_id, tok.unk_token_id}
    out = []
    for b in range(len(sentences)):
        n = int(mask[b].sum())
        lw = {}
        for i, w in zip(ids[b, :n], sparse[b, :n]):
            if int(i) not in skip and w > 0 and w > lw.get(str(int(i)), 0.0):
                lw[str(int(i))] = float(w)
        out.append((dense[b], lw, colbert[b, 1:n], ids[b, :n], pre[b, :n]))
    return out


def ref_scores(q, p, weights=(1.0, 1.0, 1.0)):
    """the five scores of one (query, passage) pair of ref_encode outputs"""
    wd, ws, wc = weights
    dense = float(q[0] @ p[0])
    sparse = float(sum(w * p[1][k] for k, w in q[1].items() if k in p[1]))
    colbert = float((q[2] @ p[2].T).max(axis=1).mean())
    return {"dense": dense, "sparse": sparse, "colbert": colbert, "sparse+dense": (wd * dense + ws * sparse) / (wd + ws),
            "colbert+sparse+dense": (wd * dense + ws * sparse + wc * colbert) / (wd + ws + wc)}


def texts(n, seed=0, lo=3, hi=40):
    """n texts of lo..hi toy words"""
    rng = np.random.default_rng(seed)
    words = X.toy_words()
    return [" ".join(words[i] for i in rng.integers(0, len(words), int(rng.integers(lo, hi + 1)))) for _ in range(n)]
