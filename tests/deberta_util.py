"""Shared pieces of the DeBERTa-v2 / v3 tests (tests/test_deberta_host.py, tests/test_gpu_deberta.py, tests/test_gpu_deberta_reranker.py): synthetic weights under
DebertaV2Model's state-dict names whose position terms DECIDE the output, the HF fp32 references (transformers.DebertaV2Model /
DebertaV2ForSequenceClassification, eager attention, on the CPU), the bucket rule as HF's tensor code computes it, and the forward restated by hand in float64
with one part of the disentangled attention broken at a time (the teeth of the element-wise bar).

Why the weights are scaled: with init-range weights (N(0, 0.02)) the two position terms move last_hidden_state by about 1e-3 — every mutation below would pass
a 3e-2 bar.  Scaling encoder.rel_embeddings does nothing behind its LayerNorm.  What decides is |PQ|, |PK| against |q|, |k|: encoder.LayerNorm.weight (the
scale of R) and the q / k projections (and their biases, which enter PQ / PK) are multiplied up until the scores are position-dominated, and the value and
attention-output matrices until the attention output stands out against the residual.  With the scales below every mutation of MUTATIONS moves some attended
row of last_hidden_state by 1.2 or more (tests/test_deberta_host.py asserts > 10 x the 3e-2 bar on this restatement, after it agrees with HF).  The q / k
MATRICES carry the smallest factor: they multiply the rounding of the 16-bit operand x into every score.  With x 12 on them (and x 4 on value / output) the
float64 restatement with every operand and stored activation rounded to f16 — no kernel involved — is itself 3.1e-2 away from the exact one, at the bar; with
the scales below it is 3.3e-3, and the position terms get their weight from the projection biases and the table's gamma instead."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import encoder_np as E  # noqa: E402

MODEL_TYPE = "deberta-v2"
SETTINGS = ("config.deberta_position_buckets", "config.deberta_max_relative_positions")
REL_NAME, REL_LN = "encoder.rel_embeddings.weight", ("encoder.LayerNorm.weight", "encoder.LayerNorm.bias")
HEAD = ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias")
EPS = 1e-7
VOCAB = 1000
PAD_ID, CLS_ID, SEP_ID = 0, 1, 2
# the scales of weights(): see the module docstring
QK_SCALE, QK_BIAS_SCALE, REL_GAMMA, VO_SCALE = 4.0, 25.0, 2.0, 6.0

_RENAME = (("attention.self.query.", "attention.self.query_proj."), ("attention.self.key.", "attention.self.key_proj."), ("attention.self.value.", "attention.self.value_proj."))


def cfg(H=128, layers=2, heads=2, FF=256, Bk=256, M=512, max_pos=512, vocab=VOCAB, labels=None, norm="layer_norm"):
    """what HipBertForward reads of a DebertaV2Config (the v3 checkpoints' settings)"""
    c = SimpleNamespace(hidden_size=H, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=FF, vocab_size=vocab, max_position_embeddings=max_pos,
                        type_vocab_size=0, layer_norm_eps=EPS, hidden_act="gelu", model_type=MODEL_TYPE, pad_token_id=PAD_ID, relative_attention=True,
                        position_buckets=Bk, max_relative_positions=M, norm_rel_ebd=norm, share_att_key=True, pos_att_type=["p2c", "c2p"], position_biased_input=False,
                        pooler_hidden_act="gelu", pooler_hidden_size=H)
    if labels is not None:
        c.num_labels = labels
    return c


def hf_config(c):
    from transformers import DebertaV2Config
    kw = dict(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
              vocab_size=c.vocab_size, max_position_embeddings=c.max_position_embeddings, type_vocab_size=0, layer_norm_eps=EPS, hidden_act="gelu",
              relative_attention=True, position_buckets=c.position_buckets, max_relative_positions=c.max_relative_positions, norm_rel_ebd=c.norm_rel_ebd,
              share_att_key=True, pos_att_type=["p2c", "c2p"], position_biased_input=False, pooler_hidden_act="gelu", pooler_hidden_size=c.hidden_size,
              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pooler_dropout=0.0, pad_token_id=PAD_ID)
    if getattr(c, "num_labels", None) is not None:
        kw["num_labels"] = c.num_labels
    return DebertaV2Config(**kw)


def weights(c, seed=3, qk=QK_SCALE, qk_bias=QK_BIAS_SCALE, gamma=REL_GAMMA, vo=VO_SCALE):
    """oracle.encoder_np's synthetic BERT weights under DebertaV2Model's names, without the position and token-type tables, + rel_embeddings N(0, 1) and its norm
    (gamma ~ `gamma` (1 + N(0, 0.1^2)), beta ~ N(0, 0.1^2)); q / k matrices x `qk`, their biases x `qk_bias`; the value and attention-output matrices x `vo`"""
    H, L = c.hidden_size, c.num_hidden_layers
    src = E.synth_weights(H, L, c.intermediate_size, c.vocab_size, 8, seed=seed)
    w = {}
    for k, v in src.items():
        if "position_embeddings" in k or "token_type_embeddings" in k:
            continue
        for a, b in _RENAME:
            k = k.replace(a, b)
        if "query_proj" in k or "key_proj" in k:
            v = v * (qk if k.endswith("weight") else qk_bias)
        if k.endswith("value_proj.weight") or k.endswith("attention.output.dense.weight"):
            v = v * vo
        w[k] = np.ascontiguousarray(v, dtype=np.float32)
    rng = np.random.Generator(np.random.PCG64(seed + 4242))
    w[REL_NAME] = rng.standard_normal((2 * c.position_buckets, H)).astype(np.float32)
    if c.norm_rel_ebd == "layer_norm":
        w[REL_LN[0]] = (gamma * (1.0 + 0.1 * rng.standard_normal(H))).astype(np.float32)
        w[REL_LN[1]] = (0.1 * rng.standard_normal(H)).astype(np.float32)
    return w


def head(H, labels, seed=21, dense_scale=1.0, out_scale=4.0):
    """the four head tensors under the library's names, seeded normal (tests/reranker_util.head: the GELU's argument at unit scale, logits over several units)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s)
    w = {HEAD[0]: f(H, H) * dense_scale / np.sqrt(H), HEAD[1]: 0.5 * f(H), HEAD[2]: f(labels, H) * out_scale / np.sqrt(H), HEAD[3]: f(labels)}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


_HF_HEAD = {HEAD[0]: "pooler.dense.weight", HEAD[1]: "pooler.dense.bias", HEAD[2]: "classifier.weight", HEAD[3]: "classifier.bias"}


def hf_model(c, w):
    """DebertaV2Model in fp32 on the CPU (its attention is eager only)"""
    from transformers import DebertaV2Model
    m = DebertaV2Model(hf_config(c))
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items() if k not in HEAD}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval()


def hf_classifier(c, w):
    """DebertaV2ForSequenceClassification in fp32 on the CPU from library-named tensors (backbone + head)"""
    from transformers import DebertaV2ForSequenceClassification
    m = DebertaV2ForSequenceClassification(hf_config(c))
    sd = {(_HF_HEAD[k] if k in HEAD else "deberta." + k): torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    res = m.load_state_dict(sd, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@torch.no_grad()
def hf_hidden(m, ids, mask):
    """last_hidden_state [B, S, H] as float64 numpy"""
    return m(input_ids=_t(ids), attention_mask=_t(mask)).last_hidden_state.double().numpy()


@torch.no_grad()
def hf_logits(m, ids, mask):
    return m(input_ids=_t(ids), attention_mask=_t(mask)).logits.double().numpy()


def pooled(hidden, mask, pool):
    """the encoders' pooling of a [B, S, H] float64 array: 0 = masked mean, 1 = [:, 0]; L2-normalised"""
    if pool == 0:
        x = (hidden * mask[..., None]).sum(1) / mask.sum(1)[:, None]
    else:
        x = hidden[:, 0]
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def tokens(B, S, side="right", seed=0, min_len=3, holes=False, full=False):
    """ids / mask [B, S]: CLS first, SEP last, lengths uniform in [min_len, S] (the first row full; `full`: all of them), padded on `side`; `holes`: every
    row also loses a few interior columns to the mask (column 0 stays attended)"""
    rng = np.random.Generator(np.random.PCG64(1000 * S + seed))
    lens = np.full(B, S) if full else rng.integers(min(min_len, S), S + 1, B)
    lens[0] = S
    ids = np.zeros((B, S), np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = int(lens[b])
        row = rng.integers(3, VOCAB, n)
        row[0], row[-1] = CLS_ID, SEP_ID
        at = slice(0, n) if side == "right" else slice(S - n, S)
        ids[b, at], mask[b, at] = row, 1
        if holes and n > 4:
            cut = at.start + 1 + rng.choice(n - 2, size=min(1 + n // 5, n - 2), replace=False)
            mask[b, cut] = 0
    return ids, mask


# ---------------------------------------------------------------------------------------------------------
# the bucket rule
# ---------------------------------------------------------------------------------------------------------
def hf_buckets(r, Bk, M):
    """p for the column differences `r` (int array) by HF's own tensor code: make_log_bucket_position in float32 + the clamp of disentangled_attention_bias"""
    from transformers.models.deberta_v2.modeling_deberta_v2 import make_log_bucket_position
    pos = make_log_bucket_position(torch.as_tensor(np.asarray(r), dtype=torch.long), Bk, M).to(torch.long)
    return torch.clamp(pos + Bk, 0, 2 * Bk - 1).numpy()


# ---------------------------------------------------------------------------------------------------------
# the forward by hand, float64
# ---------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_c2p", "no_p2c", "transposed_p", "sqrt_d", "sqrt_2d", "raw_table", "no_pos_bias", "linear_distance", "no_clamp")


def _ln(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + EPS) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / np.sqrt(2.0)))).numpy())


def by_hand(c, w, ids, mask, broken=None):
    """last_hidden_state [B, S, H] in float64 from the library-named weights, by the issue's arithmetic; rows of masked columns are whatever they are (compare
    attended rows only).  `broken`: one of MUTATIONS."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    H, heads, Bk, M = c.hidden_size, c.num_attention_heads, c.position_buckets, c.max_relative_positions
    d = H // heads
    B, S = ids.shape
    col = np.arange(S)
    r = col[:, None] - col[None, :]                                   # query column - key column
    if broken == "transposed_p":
        r = -r
    if broken == "linear_distance":
        p = np.clip(r + Bk, 0, 2 * Bk - 1)
    else:
        p = np.asarray(hf_buckets(r, Bk, M))
        if broken == "no_clamp":
            from transformers.models.deberta_v2.modeling_deberta_v2 import make_log_bucket_position
            p = (make_log_bucket_position(torch.as_tensor(r, dtype=torch.long), Bk, M).to(torch.long).numpy() + Bk) % (2 * Bk)
    R = W[REL_NAME][:2 * Bk]
    if REL_LN[0] in W and broken != "raw_table":
        R = _ln(R, W[REL_LN[0]], W[REL_LN[1]])
    scale = np.sqrt({"sqrt_d": 1.0, "sqrt_2d": 2.0}.get(broken, 3.0) * d)
    x = _ln(W["embeddings.word_embeddings.weight"][ids], W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"])
    keymask = mask.astype(bool)[:, None, None, :]                     # [B, 1, 1, S]
    for li in range(c.num_hidden_layers):
        g = lambda n: W[f"encoder.layer.{li}.{n}"]
        Wq, bq, Wk, bk = g("attention.self.query_proj.weight"), g("attention.self.query_proj.bias"), g("attention.self.key_proj.weight"), g("attention.self.key_proj.bias")
        split = lambda t: t.reshape(t.shape[:-1] + (heads, d))
        q = split(x @ Wq.T + bq).transpose(0, 2, 1, 3)                # [B, h, S, d]
        k = split(x @ Wk.T + bk).transpose(0, 2, 1, 3)
        v = split(x @ g("attention.self.value_proj.weight").T + g("attention.self.value_proj.bias")).transpose(0, 2, 1, 3)
        nb = broken == "no_pos_bias"
        PQ = split(R @ Wq.T + (0 if nb else bq)).transpose(1, 0, 2)   # [h, 2 Bk, d]
        PK = split(R @ Wk.T + (0 if nb else bk)).transpose(1, 0, 2)
        s = q @ k.transpose(0, 1, 3, 2)
        if broken != "no_c2p":
            c2p = q @ PK.transpose(0, 2, 1)[None]                     # [B, h, S, 2 Bk]
            s = s + np.take_along_axis(c2p, np.broadcast_to(p[None, None], (B, heads, S, S)), axis=3)
        if broken != "no_p2c":
            p2c = k @ PQ.transpose(0, 2, 1)[None]                     # [B, h, S(key), 2 Bk]
            s = s + np.take_along_axis(p2c, np.broadcast_to(p.T[None, None], (B, heads, S, S)), axis=3).transpose(0, 1, 3, 2)
        s = np.where(keymask, s / scale, -np.inf)
        s = s - s.max(-1, keepdims=True)
        a = np.exp(s)
        a = a / a.sum(-1, keepdims=True)
        ctx = (a @ v).transpose(0, 2, 1, 3).reshape(B, S, H)
        x = _ln(ctx @ g("attention.output.dense.weight").T + g("attention.output.dense.bias") + x, g("attention.output.LayerNorm.weight"), g("attention.output.LayerNorm.bias"))
        h = _gelu(x @ g("intermediate.dense.weight").T + g("intermediate.dense.bias"))
        x = _ln(h @ g("output.dense.weight").T + g("output.dense.bias") + x, g("output.LayerNorm.weight"), g("output.LayerNorm.bias"))
    return x


HEAD_MUTATIONS = ("tanh", "no_bd", "no_bo", "mean_row", "normalised_row", "neighbour_row")


def head_by_hand(w, hidden, mask, broken=None):
    """logits [B, L] in float64 of ContextPooler + classifier on a [B, S, H] float64 last_hidden_state; `broken`: one of HEAD_MUTATIONS"""
    Wd, bd, Wo, bo = (np.asarray(w[k], np.float64) for k in HEAD)
    x = hidden[:, 0]
    if broken == "mean_row":
        x = (hidden * mask[..., None]).sum(1) / mask.sum(1)[:, None]
    elif broken == "normalised_row":
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    elif broken == "neighbour_row":
        x = hidden[:, 1]
    a = x @ Wd.T + (0 if broken == "no_bd" else bd)
    t = np.tanh(a) if broken == "tanh" else _gelu(a)
    return t @ Wo.T + (0 if broken == "no_bo" else bo)


def head_bound(x, w):
    """The a-priori fp32 bound of tests/reranker_util.head_bound for the erf-GELU variant of k_cls_head: the same sums (gamma = (H + 2) 2^-24 per dot product),
    and for the activation |gelu'| <= 1.13 in place of |tanh'| <= 1, |gelu(a)| <= |a| in place of |tanh| <= 1, erff / the two products within 8 ulp."""
    Wd, bd, Wo, bo = (np.asarray(w[k], np.float64) for k in HEAD)
    x = np.asarray(x, np.float64)
    H = x.shape[1]
    u = 2.0 ** -24
    g = (H + 2) * u
    a = x @ Wd.T + bd
    t = _gelu(a)
    A = np.abs(x) @ np.abs(Wd).T + np.abs(bd)
    e = 1.13 * g * A + 8 * u * (np.abs(a) + 1.0)
    bound = e @ np.abs(Wo).T + g * (np.abs(t) @ np.abs(Wo).T + np.abs(bo))
    return t @ Wo.T + bo, bound


def state_dict_keys(c, classifier=False):
    """every key of the HF model's state dict (parameters and buffers), without building weights twice"""
    from transformers import DebertaV2ForSequenceClassification, DebertaV2Model
    with torch.device("meta"):
        m = (DebertaV2ForSequenceClassification if classifier else DebertaV2Model)(hf_config(c))
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}
