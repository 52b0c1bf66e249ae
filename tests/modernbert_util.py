"""Shared pieces of the ModernBERT tests (tests/test_modernbert_host.py, tests/test_gpu_modernbert.py): configs, synthetic weights under ModernBertModel's
state-dict names, the HF fp32 reference (transformers.ModernBertModel, eager attention) with the encoders' pooling, and the six ways of breaking it that the
GPU tests assert as preconditions."""
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import torch

from oracle import encoder_np as E

LOCAL_FREQ_NAME, HALF_WINDOW_NAME, LAYER_FLAGS_NAME = "config.rotary_inv_freq_local", "config.attention_half_window", "config.local_attention_layers"
GLOBAL_FREQ_NAME = "config.rotary_inv_freq"
FULL, SLIDING = "full_attention", "sliding_attention"
THETA = {FULL: 160000.0, SLIDING: 10000.0}


def inv_freq(d_h, theta):
    """ModernBertRotaryEmbedding.compute_default_rope_parameters: 1 / theta^(2j / d_h), j < d_h / 2, in torch's fp32 arithmetic"""
    return (1.0 / (theta ** (torch.arange(0, d_h, 2, dtype=torch.float) / d_h))).numpy()


def layer_types(L, every=3):
    """ModernBertConfig's default: every third layer, from layer 0, is global"""
    return [SLIDING if i % every else FULL for i in range(L)]


def cfg(H, L, heads, FF, vocab, max_pos=8192, types=None, local_attention=128, **extra):
    d = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=vocab, max_position_embeddings=max_pos,
             norm_eps=1e-5, norm_bias=False, attention_bias=False, mlp_bias=False, hidden_activation="gelu", model_type="modernbert", pad_token_id=0,
             bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2, local_attention=local_attention,
             layer_types=list(types) if types is not None else layer_types(L),
             rope_parameters={FULL: {"rope_type": "default", "rope_theta": THETA[FULL]}, SLIDING: {"rope_type": "default", "rope_theta": THETA[SLIDING]}},
             attention_dropout=0.0, embedding_dropout=0.0, mlp_dropout=0.0)
    d.update(extra)
    c = SimpleNamespace(**d)
    c.sliding_window = c.local_attention // 2       # ModernBertConfig's property
    return c


def hf_config(c):
    from transformers import ModernBertConfig
    kw = {k: v for k, v in vars(c).items() if k not in ("model_type", "sliding_window")}
    kw["rope_parameters"] = {k: dict(v) for k, v in kw["rope_parameters"].items()}
    hc = ModernBertConfig(**kw)
    hc._attn_implementation = "eager"
    return hc


def teeth_weights(H, L, FF, vocab, seed=11, sigma=1.57):
    """every layer matrix N(0, (sigma / sqrt(fan_in))^2), LayerNorm weights near 1, token embeddings N(0, 1): scores large enough for the window, the thetas and
    the rotation to decide the attention"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = {"embeddings.tok_embeddings.weight": f(vocab, H), "embeddings.norm.weight": (1 + 0.1 * f(H)).astype(np.float32),
         "final_norm.weight": (1 + 0.1 * f(H)).astype(np.float32)}
    for l in range(L):
        p = f"layers.{l}."
        if l:
            w[p + "attn_norm.weight"] = (1 + 0.1 * f(H)).astype(np.float32)
        w[p + "attn.Wqkv.weight"] = f(3 * H, H) * np.float32(sigma / np.sqrt(H))
        w[p + "attn.Wo.weight"] = f(H, H) * np.float32(sigma / np.sqrt(H))
        w[p + "mlp_norm.weight"] = (1 + 0.1 * f(H)).astype(np.float32)
        w[p + "mlp.Wi.weight"] = f(2 * FF, H) * np.float32(sigma / np.sqrt(H))
        w[p + "mlp.Wo.weight"] = f(H, FF) * np.float32(sigma / np.sqrt(FF))
    return w


def from_bert(w, L, seed=0):
    """oracle.encoder_np's BERT-shaped weights under ModernBert's names: no position table, no biases; Wqkv = q | k | v, mlp.Wi = the intermediate matrix (the
    GELU half) | a second draw of the same law (the gate), the LayerNorm weights in their pre-LN places"""
    rng = np.random.Generator(np.random.PCG64(seed + 777))
    g = lambda k: np.asarray(w[k], np.float32)
    out = {"embeddings.tok_embeddings.weight": g("embeddings.word_embeddings.weight"), "embeddings.norm.weight": g("embeddings.LayerNorm.weight"),
           "final_norm.weight": g(f"encoder.layer.{L - 1}.output.LayerNorm.weight")}
    for l in range(L):
        b, p = f"encoder.layer.{l}.", f"layers.{l}."
        if l:
            out[p + "attn_norm.weight"] = g(f"encoder.layer.{l - 1}.output.LayerNorm.weight")
        out[p + "attn.Wqkv.weight"] = np.concatenate([g(b + "attention.self.query.weight"), g(b + "attention.self.key.weight"), g(b + "attention.self.value.weight")])
        out[p + "attn.Wo.weight"] = g(b + "attention.output.dense.weight")
        out[p + "mlp_norm.weight"] = g(b + "attention.output.LayerNorm.weight")
        wi = g(b + "intermediate.dense.weight")
        out[p + "mlp.Wi.weight"] = np.concatenate([wi, (0.02 * rng.standard_normal(wi.shape)).astype(np.float32)])
        out[p + "mlp.Wo.weight"] = g(b + "output.dense.weight")
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def weights(H, L, FF, vocab, wname="benign", seed=None):
    if wname == "benign":
        w = E.synth_weights(H, L, FF, vocab, 8, seed=3 if seed is None else seed)
    else:
        w = E.synth_weights_outlier(H, L, FF, vocab, 8, seed=7 if seed is None else seed, gamma_lo=1.5, gamma_hi=3.0)    # out3 (tests/golden/g10_spec.py)
    return from_bert(w, L, seed=0 if seed is None else seed)


def hf_model(c, w, device="cuda"):
    from transformers import ModernBertModel
    m = ModernBertModel(hf_config(c))
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


BREAKS = ("all_global", "window_minus_1", "window_plus_1", "thetas_exchanged", "no_rotation", "wi_halves_exchanged")
WINDOW_BREAKS = BREAKS[:3]


@contextmanager
def broken(m, how):
    """the reference with one part of the feature broken: the window removed / one narrower / one wider (config.local_attention, which the mask is built from
    at every forward), the two inv_freq vectors exchanged, the rotation dropped, the halves of every mlp.Wi exchanged"""
    r = m.rotary_emb
    keep_local = m.config.local_attention
    names = [n for n in (FULL + "_inv_freq", SLIDING + "_inv_freq") if hasattr(r, n)]
    keep = {n: getattr(r, n).clone() for n in names}
    def swap_wi():
        with torch.no_grad():
            for l in m.layers:
                a, b = l.mlp.Wi.weight.chunk(2, dim=0)
                l.mlp.Wi.weight.copy_(torch.cat([b, a]).clone())
    try:
        if how == "all_global":
            m.config.local_attention = 1 << 20
        elif how == "window_minus_1":
            m.config.local_attention = keep_local - 2
        elif how == "window_plus_1":
            m.config.local_attention = keep_local + 2
        elif how == "thetas_exchanged":
            getattr(r, names[0]).copy_(keep[names[1]]); getattr(r, names[1]).copy_(keep[names[0]])
        elif how == "no_rotation":
            for n in names:
                getattr(r, n).zero_()
        elif how == "wi_halves_exchanged":
            swap_wi()
        else:
            raise ValueError(how)
        yield m
    finally:
        m.config.local_attention = keep_local
        for n in names:
            getattr(r, n).copy_(keep[n])
        if how == "wi_halves_exchanged":
            swap_wi()


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


def mlp_np(x, wi, wo, bi=None):
    """ModernBertMLP in numpy (float64): Wo . (erf_gelu(input) * gate), input, gate = (Wi . x + bi).chunk(2).  Every sum runs left to right (cumsum), so that
    trailing zero terms leave it unchanged bit for bit (BLAS picks its blocking by the length)"""
    x, wi, wo = np.asarray(x, np.float64), np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    dot = lambda a, b: np.cumsum(a[:, None, :] * b[None, :, :], axis=-1)[..., -1]
    h = dot(x, wi)
    if bi is not None:
        h = h + np.asarray(bi, np.float64)
    a, g = np.split(h, 2, axis=-1)
    return dot(E.gelu_erf(a) * g, wo)
