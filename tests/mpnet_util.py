"""Shared pieces of the MPNet tests (tests/test_mpnet_host.py, tests/test_gpu_mpnet.py): MPNet's bucket rule restated in integers, synthetic weights under
MPNet's state-dict names with a relative-attention-bias table, and the HF fp32 reference (transformers.MPNetModel) with the encoders' pooling."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import encoder_np as E

PAD = 1                       # MPNetEmbeddings.padding_idx (a class constant)
BUCKETS = 32
BIAS_NAME = "encoder.relative_attention_bias.weight"
# first |d| of buckets 8 .. 15
BOUNDARIES = (8, 12, 16, 23, 32, 46, 64, 91)

_RENAME = (("attention.self.query.", "attention.attn.q."), ("attention.self.key.", "attention.attn.k."), ("attention.self.value.", "attention.attn.v."),
           ("attention.output.dense.", "attention.attn.o."), ("attention.output.LayerNorm.", "attention.LayerNorm."))


def bucket(d):
    """MPNetEncoder.relative_position_bucket(d) (32 buckets, max_distance 128) for d = col_key - col_query, in integers: n = |d|; n < 8: n, else
    min(15, 8 + max{j >= 0 : 64 * 2^j <= n^2}); + 16 when d > 0."""
    d = np.asarray(d, dtype=np.int64)
    n = np.abs(d)
    b = n.copy()
    large = n >= 8
    j = np.zeros_like(n)
    for t in range(1, 8):
        j = np.where((64 << t) <= n * n, t, j)
    b = np.where(large, np.minimum(15, 8 + j), b)
    return b + 16 * (d > 0)


def delta_table(W, S):
    """tab[h][d + S - 1] = W[bucket(d)][h] for d = -(S-1) .. S-1"""
    d = np.arange(-(S - 1), S)
    return np.ascontiguousarray(np.asarray(W)[bucket(d)].T)


def bias_from_table(tab, S):
    """[heads, S, S]: bias[h, q, k] = tab[h][k - q + S - 1]"""
    q, k = np.arange(S)[:, None], np.arange(S)[None, :]
    return tab[:, k - q + S - 1]


def mirrored(W):
    """the table a sign mistake in d would read: bucket(-d) instead of bucket(d) (d = 0 stays bucket 0; bucket 16 is never hit)"""
    W = np.asarray(W)
    M = W.copy()
    M[1:16], M[17:32] = W[17:32], W[1:16]
    return M


def cfg(H, L, heads, FF, vocab, max_pos=514, buckets=BUCKETS):
    return SimpleNamespace(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=vocab, max_position_embeddings=max_pos,
                           layer_norm_eps=1e-5, hidden_act="gelu", model_type="mpnet", pad_token_id=PAD, relative_attention_num_buckets=buckets)


def to_mpnet_names(w):
    out = {}
    for k, v in w.items():
        if "token_type_embeddings" in k:
            continue
        for a, b in _RENAME:
            k = k.replace(a, b)
        out[k] = v
    return out


def to_bert_names(w):
    """the same weights as a RoBERTa-style state dict: BERT's names, one zero token-type row, no bias table"""
    out = {}
    for k, v in w.items():
        if k == BIAS_NAME:
            continue
        for a, b in _RENAME:
            k = k.replace(b, a)
        out[k] = v
    H = out["embeddings.word_embeddings.weight"].shape[1]
    out["embeddings.token_type_embeddings.weight"] = np.zeros((1, H), np.float32)
    return out


def weights(H, L, heads, FF, vocab, max_pos=514, wname="benign", seed=None, bias_sigma=1.0, bias=None):
    """oracle.encoder_np's synthetic BERT weights under MPNet's names + a bias table N(0, bias_sigma^2) (or `bias`, [32, heads])"""
    if wname == "benign":
        w = E.synth_weights(H, L, FF, vocab, max_pos, seed=3 if seed is None else seed)
    else:
        w = E.synth_weights_outlier(H, L, FF, vocab, max_pos, seed=7 if seed is None else seed, gamma_lo=1.5, gamma_hi=3.0)    # out3 (tests/golden/g10_spec.py)
    w = to_mpnet_names(w)
    if bias is None:
        rng = np.random.Generator(np.random.PCG64(977 if seed is None else seed + 977))
        bias = bias_sigma * rng.standard_normal((BUCKETS, heads))
    w[BIAS_NAME] = np.ascontiguousarray(bias, dtype=np.float32)
    return w


def boundary_table(heads):
    """W[b, h] = 2 (-1)^b for b < 16, -2 (-1)^b for b >= 16: neighbouring buckets and the two signs of d all differ"""
    b = np.arange(BUCKETS)
    col = np.where(b < 16, 2.0, -2.0) * (-1.0) ** b
    return np.ascontiguousarray(np.repeat(col[:, None], heads, 1), dtype=np.float32)


def hf_model(c, w, device="cuda"):
    from transformers import MPNetConfig, MPNetModel
    m = MPNetModel(MPNetConfig(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                               intermediate_size=c.intermediate_size, vocab_size=c.vocab_size, max_position_embeddings=c.max_position_embeddings,
                               layer_norm_eps=1e-5, relative_attention_num_buckets=BUCKETS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0),
                   add_pooling_layer=False)
    missing = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=False).missing_keys
    assert not missing, missing
    return m.float().eval().to(device)


def set_bias(m, W):
    with torch.no_grad():
        m.encoder.relative_attention_bias.weight.copy_(torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)))


@torch.no_grad()
def hf_last_hidden(m, ids, mask, chunk=8):
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev); k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev)
        outs.append(m(input_ids=a, attention_mask=k).last_hidden_state.cpu().numpy())
    return np.concatenate(outs)


def pool_np(lh, mask, pool):
    """masked mean (pool 0) / [:, 0] (pool 1) -> L2 normalise: the encoders' pooling"""
    lh = np.asarray(lh, np.float64); mk = np.asarray(mask) != 0
    v = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None] if pool == 0 else lh[:, 0]
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def hf_encode(m, ids, mask, pool, chunk=8):
    return pool_np(hf_last_hidden(m, ids, mask, chunk), mask, pool)
