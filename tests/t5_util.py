"""Shared pieces of the T5 tests (tests/test_t5_host.py, tests/test_gpu_t5.py): configs, synthetic weights under T5EncoderModel's state-dict names, the HF fp32
reference (transformers.T5EncoderModel, eager attention) with the encoders' pooling and Dense head, and the ways of breaking it that the GPU tests assert as
preconditions."""
import json
import os
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import torch

BIAS_NAME = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
SETTING = "config.t5_feed_forward"
BUCKETS = 32
RELU, GATED = "relu", "gated-gelu"          # T5Config.feed_forward_proj: v1.0, v1.1 / flan
WIDTHS = {64: (768, 12), 32: (384, 12)}     # head width -> (d_model, heads)


def cfg(H, L, heads, FF, vocab, ff=RELU, **extra):
    """the fields of a T5Config the encoders read"""
    d = dict(d_model=H, d_kv=H // heads, num_heads=heads, d_ff=FF, num_layers=L, vocab_size=vocab, feed_forward_proj=ff, layer_norm_epsilon=1e-6,
             relative_attention_num_buckets=32, relative_attention_max_distance=128, model_type="t5", n_positions=512,
             dense_act_fn="relu" if ff == RELU else "gelu_new", is_gated_act=ff != RELU)
    d.update(extra)
    return SimpleNamespace(**d)


def hf_config(c):
    from transformers import T5Config
    hc = T5Config(d_model=c.d_model, d_kv=c.d_kv, num_heads=c.num_heads, d_ff=c.d_ff, num_layers=c.num_layers, vocab_size=c.vocab_size,
                  feed_forward_proj=c.feed_forward_proj, layer_norm_epsilon=c.layer_norm_epsilon, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False,
                  relative_attention_num_buckets=c.relative_attention_num_buckets, relative_attention_max_distance=c.relative_attention_max_distance,
                  pad_token_id=0, eos_token_id=1)
    hc._attn_implementation = "eager"
    return hc


def weights(H, L, heads, FF, vocab, ff=RELU, seed=11, bias_sigma=4.0, bias=None, offset=0.0):
    """shared ~ N(0, 1) (+ offset: a common component of every row that only a mean-subtracting norm removes), norm weights 1 + 0.1 N, the bias table
    N(0, bias_sigma^2) (or `bias`, [32, heads]), q and k N(0, 1 / fan_in) each divided by d_h^(1/4) (unscaled scores q.k of variance ~1), every other matrix
    N(0, 1 / fan_in)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    norm = lambda: (1 + 0.1 * f(H)).astype(np.float32)
    qk = np.float32(1.0 / np.sqrt(H) / (H // heads) ** 0.25)
    w = {"shared.weight": f(vocab, H) + np.float32(offset)}
    for l in range(L):
        a, m = f"encoder.block.{l}.layer.0.", f"encoder.block.{l}.layer.1."
        w[a + "SelfAttention.q.weight"] = f(H, H) * qk
        w[a + "SelfAttention.k.weight"] = f(H, H) * qk
        w[a + "SelfAttention.v.weight"] = f(H, H) * np.float32(1 / np.sqrt(H))
        w[a + "SelfAttention.o.weight"] = f(H, H) * np.float32(1 / np.sqrt(H))
        w[a + "layer_norm.weight"] = norm()
        if ff == RELU:
            w[m + "DenseReluDense.wi.weight"] = f(FF, H) * np.float32(1 / np.sqrt(H))
        else:
            w[m + "DenseReluDense.wi_0.weight"] = f(FF, H) * np.float32(1 / np.sqrt(H))
            w[m + "DenseReluDense.wi_1.weight"] = f(FF, H) * np.float32(1 / np.sqrt(H))
        w[m + "DenseReluDense.wo.weight"] = f(H, FF) * np.float32(1 / np.sqrt(FF))
        w[m + "layer_norm.weight"] = norm()
    w["encoder.final_layer_norm.weight"] = norm()
    w[BIAS_NAME] = np.ascontiguousarray(bias_sigma * f(BUCKETS, heads) if bias is None else bias, dtype=np.float32)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def dense_weight(P, H, seed=5):
    """the Dense head's matrix [P, H] ~ N(0, 1 / H)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.ascontiguousarray(rng.standard_normal((P, H)) / np.sqrt(H), dtype=np.float32)


def hf_model(c, w, device="cuda"):
    from transformers import T5EncoderModel
    m = T5EncoderModel(hf_config(c))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items() if k != "dense.weight"}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    res = m.load_state_dict(sd, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


def set_bias(m, W):
    with torch.no_grad():
        m.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.copy_(torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)))


@contextmanager
def broken(m, how):
    """the reference with one part of the feature broken: "q_scaled" = q divided by sqrt(d_h) (BERT's scores), "erf_gelu" = the relu replaced by erf-GELU,
    "wi_exchanged" = wi_0 and wi_1 exchanged, "layer_norm" = every T5LayerNorm subtracting the mean like nn.LayerNorm"""
    from transformers.models.t5 import modeling_t5 as MT
    blocks = m.encoder.block
    d_h = m.config.d_kv
    keep_fwd = MT.T5LayerNorm.forward

    def scale_q(s):
        with torch.no_grad():
            for b in blocks:
                b.layer[0].SelfAttention.q.weight.mul_(s)

    def swap_wi():
        with torch.no_grad():
            for b in blocks:
                d = b.layer[1].DenseReluDense
                t = d.wi_0.weight.clone(); d.wi_0.weight.copy_(d.wi_1.weight); d.wi_1.weight.copy_(t)

    keep_q = [b.layer[0].SelfAttention.q.weight.clone() for b in blocks]
    keep_act = [b.layer[1].DenseReluDense.act for b in blocks]
    try:
        if how == "q_scaled":
            scale_q(1.0 / np.sqrt(d_h))
        elif how == "erf_gelu":
            for b in blocks:
                b.layer[1].DenseReluDense.act = torch.nn.GELU()
        elif how == "wi_exchanged":
            swap_wi()
        elif how == "layer_norm":
            def mean_subtracting(self, x):
                return torch.nn.functional.layer_norm(x.float(), x.shape[-1:], self.weight.float(), None, self.variance_epsilon)
            MT.T5LayerNorm.forward = mean_subtracting
        else:
            raise ValueError(how)
        yield m
    finally:
        MT.T5LayerNorm.forward = keep_fwd
        with torch.no_grad():
            for b, q, act in zip(blocks, keep_q, keep_act):
                b.layer[0].SelfAttention.q.weight.copy_(q)
                b.layer[1].DenseReluDense.act = act
        if how == "wi_exchanged":
            swap_wi()


@torch.no_grad()
def hf_last_hidden(m, ids, mask, chunk=8):
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev); k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev)
        outs.append(m(input_ids=a, attention_mask=k).last_hidden_state.cpu().numpy())
    return np.concatenate(outs)


def pool_np(lh, mask, pool, W=None):
    """masked mean (pool 0) / [:, 0] (pool 1) -> the Dense head W [P, H] (None: none) -> L2 normalise, in float64: the encoders' head"""
    lh = np.asarray(lh, np.float64); mk = np.asarray(mask) != 0
    v = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None] if pool == 0 else lh[:, 0]
    if W is not None:
        v = v @ np.asarray(W, np.float64).T
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def tokens(B, S, layout, seed, vocab, lo=None):
    """(ids, mask) [B,S] int64: real ids in [2, vocab), id 0 (T5's pad) in every column that is not attended.  R = right-padded ragged lengths (S/2 .. S, one of
    them S), L = left-padded, F = full length."""
    rng = np.random.default_rng(seed)
    real = rng.integers(2, vocab, (B, S))
    lens = rng.integers(max(2, S // 2) if lo is None else lo, S + 1, B)
    lens[0] = S
    if layout == "F":
        lens[:] = S
    ids = np.zeros((B, S), np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        n = int(lens[r])
        if layout == "L":
            ids[r, S - n:] = real[r, :n]; mask[r, S - n:] = 1
        else:
            ids[r, :n] = real[r, :n]; mask[r, :n] = 1
    return ids, mask


def write_st_dense(folder, W, sub="2_Dense", bias=False, activation="torch.nn.modules.linear.Identity", in_features=None, fmt="safetensors"):
    """the files sentence-transformers writes for a Dense module behind a mean pooling: modules.json, <sub>/config.json, <sub>/model.safetensors (or
    pytorch_model.bin)"""
    W = np.asarray(W, np.float32)
    os.makedirs(os.path.join(folder, sub), exist_ok=True)
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": sub, "type": "sentence_transformers.models.Dense"},
               {"idx": 3, "name": "3", "path": "3_Normalize", "type": "sentence_transformers.models.Normalize"}]
    with open(os.path.join(folder, "modules.json"), "w") as f:
        json.dump(modules, f)
    with open(os.path.join(folder, sub, "config.json"), "w") as f:
        json.dump({"in_features": W.shape[1] if in_features is None else in_features, "out_features": W.shape[0], "bias": bias, "activation_function": activation}, f)
    state = {"linear.weight": torch.from_numpy(W.copy())}
    if bias:
        state["linear.bias"] = torch.zeros(W.shape[0])
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(state, os.path.join(folder, sub, "model.safetensors"))
    else:
        torch.save(state, os.path.join(folder, sub, "pytorch_model.bin"))
