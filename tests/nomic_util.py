"""Shared pieces of the NomicBert tests (tests/test_nomic_host.py, tests/test_gpu_nomic.py): the rotary table rule and the row orders of the packed weights
restated in numpy, synthetic weights under NomicBert's state-dict names, and the HF fp32 reference (transformers.NomicBertModel) with the encoders' pooling
and the four ways of breaking it that the GPU tests use as preconditions."""
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import torch

from oracle import encoder_np as E

INV_FREQ_NAME = "config.rotary_inv_freq"

_RENAME = (("attention.self.query.", "self_attn.q_proj."), ("attention.self.key.", "self_attn.k_proj."), ("attention.self.value.", "self_attn.v_proj."),
           ("attention.output.dense.", "self_attn.o_proj."), ("attention.output.LayerNorm.", "post_attention_layernorm."),
           ("intermediate.dense.", "mlp.gate_proj."), ("output.dense.", "mlp.down_proj."), ("output.LayerNorm.", "post_mlp_layernorm."))


def inv_freq(d_h, theta=1000.0):
    """NomicBertRotaryEmbedding.compute_default_rope_parameters: 1 / theta^(2j / d_h), j < d_h / 2, in torch's fp32 arithmetic"""
    return (1.0 / (theta ** (torch.arange(0, d_h, 2, dtype=torch.float) / d_h))).numpy()


def angles(inv, max_pos):
    """the table rule: angle[pos, j] = the fp32 product float(pos) * inv_freq[j] (HF computes it as a matmul with inner dimension 1)"""
    return (np.arange(max_pos, dtype=np.float32)[:, None] * np.asarray(inv, np.float32)[None, :]).astype(np.float32)


def tables(inv, max_pos):
    """(cos, sin) [max_pos, d_h / 2] as the library builds them: the cosine / sine of the fp32 angle, evaluated in double and rounded once"""
    a = angles(inv, max_pos).astype(np.float64)
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def rotate(x, cos, sin):
    """x [..., S, d_h] -> x'[j] = x[j] cos - x[j + d_h/2] sin, x'[j + d_h/2] = x[j + d_h/2] cos + x[j] sin (cos / sin [S, d_h / 2])"""
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    return np.concatenate([a * cos - b * sin, b * cos + a * sin], -1)


def head64_row(r):
    """where row r of q_proj / k_proj lies in the packed copy of a handle with 64-wide heads: the four 16-row blocks of a head in the order 0, 2, 1, 3, so that
    feature j and its rotary partner j + 32 share a 32-column MFMA tile"""
    r = np.asarray(r)
    b = (r >> 4) & 3
    return (r & ~63) + ((((b & 1) << 1) | (b >> 1)) << 4) + (r & 15)


def interleave_gate_up(gate, up):
    """[2 FF, H]: tile t of 32 rows = gate rows 16 t .. 16 t + 15, then the up rows of the same features (the packed intermediate matrix of a NomicBert handle)"""
    FF, H = gate.shape
    return np.concatenate([gate.reshape(FF // 16, 16, H), up.reshape(FF // 16, 16, H)], 1).reshape(2 * FF, H)


def split_gate_up(w):
    F2, H = w.shape
    t = w.reshape(F2 // 32, 2, 16, H)
    return t[:, 0].reshape(F2 // 2, H), t[:, 1].reshape(F2 // 2, H)


def cfg(H, L, heads, FF, vocab, max_pos=8192, **extra):
    d = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=vocab, max_position_embeddings=max_pos,
             layer_norm_eps=1e-12, hidden_act="silu", model_type="nomic_bert", type_vocab_size=2, pad_token_id=0, head_dim=H // heads,
             rope_parameters={"rope_theta": 1000.0, "rope_type": "default"}, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    d.update(extra)
    return SimpleNamespace(**d)


def hf_config(c):
    from transformers import NomicBertConfig
    kw = {k: v for k, v in vars(c).items() if k != "model_type"}
    return NomicBertConfig(**kw)


def to_nomic_names(w, matrix_scale=1.0, seed=0):
    """oracle.encoder_np's BERT-shaped weights under NomicBert's names: no position table, no linear biases, gate_proj = the intermediate matrix and up_proj
    a second draw of the same law; every layer matrix times `matrix_scale`"""
    rng = np.random.Generator(np.random.PCG64(seed + 4242))
    out = {}
    for k, v in w.items():
        if "position_embeddings" in k or (k.endswith(".bias") and "LayerNorm" not in k):
            continue
        layer = k.startswith("encoder.layer.")
        k = k.replace("encoder.layer.", "layers.")
        for a, b in _RENAME:
            k = k.replace(a, b)
        out[k] = np.ascontiguousarray(v * matrix_scale if layer and "proj" in k else v, dtype=np.float32)
        if "mlp.gate_proj." in k:
            out[k.replace("gate_proj", "up_proj")] = np.ascontiguousarray(0.02 * matrix_scale * rng.standard_normal(v.shape), dtype=np.float32)
    return out


def weights(H, L, heads, FF, vocab, wname="benign", seed=None, matrix_scale=1.0):
    if wname == "benign":
        w = E.synth_weights(H, L, FF, vocab, 8, seed=3 if seed is None else seed)
    else:
        w = E.synth_weights_outlier(H, L, FF, vocab, 8, seed=7 if seed is None else seed, gamma_lo=1.5, gamma_hi=3.0)    # out3 (tests/golden/g10_spec.py)
    return to_nomic_names(w, matrix_scale, seed=0 if seed is None else seed)


def hf_model(c, w, device="cuda"):
    from transformers import NomicBertModel
    m = NomicBertModel(hf_config(c), add_pooling_layer=False)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


@contextmanager
def broken(m, how):
    """the reference with one of the feature's parts broken: "no_rotation" (inv_freq zeroed), "mirrored" (inv_freq negated: the sign of the rotation),
    "swapped" (gate_proj and up_proj exchanged), "gelu" (another activation)"""
    from transformers.activations import ACT2FN
    keep = m.rotary_emb.inv_freq.clone()
    acts = [l.mlp.act_fn for l in m.layers]
    def swap():
        with torch.no_grad():
            for l in m.layers:
                g = l.mlp.gate_proj.weight.clone()
                l.mlp.gate_proj.weight.copy_(l.mlp.up_proj.weight); l.mlp.up_proj.weight.copy_(g)
    try:
        if how == "no_rotation":
            m.rotary_emb.inv_freq.zero_()
        elif how == "mirrored":
            m.rotary_emb.inv_freq.neg_()
        elif how == "swapped":
            swap()
        elif how == "gelu":
            for l in m.layers:
                l.mlp.act_fn = ACT2FN["gelu"]
        else:
            raise ValueError(how)
        yield m
    finally:
        m.rotary_emb.inv_freq.copy_(keep)
        if how == "swapped":
            swap()
        for l, a in zip(m.layers, acts):
            l.mlp.act_fn = a


BREAKS = ("no_rotation", "mirrored", "swapped", "gelu")


@torch.no_grad()
def hf_last_hidden(m, ids, mask, tt=None, chunk=8):
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev); k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev)
        t = None if tt is None else torch.from_numpy(np.ascontiguousarray(tt[i:i + chunk])).to(dev)
        outs.append(m(input_ids=a, attention_mask=k, token_type_ids=t).last_hidden_state.cpu().numpy())
    return np.concatenate(outs)


def pool_np(lh, mask, pool):
    """masked mean (pool 0) / [:, 0] (pool 1) -> L2 normalise: the encoders' pooling"""
    lh = np.asarray(lh, np.float64); mk = np.asarray(mask) != 0
    v = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None] if pool == 0 else lh[:, 0]
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def hf_encode(m, ids, mask, pool, tt=None, chunk=8):
    return pool_np(hf_last_hidden(m, ids, mask, tt, chunk), mask, pool)
