"""Shared pieces of the jina-embeddings-v3 tests (tests/test_jina3_host.py, tests/test_gpu_jina3.py): tiny JinaEmbeddingsV3Config shapes, synthetic weights under
HF's state-dict names, the HF fp32 eager reference (transformers.JinaEmbeddingsV3Model), numpy pooling, and the ways of breaking the reference that the GPU
tests assert as preconditions.

Weights are drawn as tests/decoder_util.py draws them: embedding rows N(0.4, 1), norm weights in [0.7, 1.5] (norm biases N(0, 0.2^2)), q / k matrices
N(0, 1.2^2 / H), v / o N(0, 0.7^2 / H), fc1 N(0, 1 / H), fc2 N(0, 1 / FF), every linear bias N(0, 0.5^2), rope_theta 100 so that the angles matter a few
tokens apart.  The rows of a post-LN stack leave the last LayerNorm with magnitude ~ 1."""
from contextlib import contextmanager

import numpy as np
import torch

from decoder_util import last_index, tokens  # noqa: F401  (the token layouts are the decoders')

SETTING = "config.rotary_feed_forward"
INV_FREQ_NAME = "config.rotary_inv_freq"
POOL_MEAN, POOL_CLS = 0, 1
SHAPES = {"jina-64": (128, 2), "jina-32": (128, 4)}      # (H, heads): 2 heads of 64, 4 heads of 32
FF, VOCAB, MAX_POS, TYPE_VOCAB = 256, 200, 512, 2


def hf_config(kind, L=2, max_pos=MAX_POS, **extra):
    from transformers import JinaEmbeddingsV3Config
    H, heads = SHAPES[kind]
    kw = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=VOCAB, max_position_embeddings=max_pos,
              type_vocab_size=TYPE_VOCAB, layer_norm_eps=1e-5, hidden_act="gelu", rope_parameters={"rope_theta": 100.0, "rope_type": "default"},
              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pad_token_id=0)
    kw.update(extra)
    cfg = JinaEmbeddingsV3Config(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def weights(cfg, seed=5, pooler=True):
    """HF state-dict name -> fp32 array"""
    rng = np.random.default_rng(seed)
    H, L, ff = cfg.hidden_size, cfg.num_hidden_layers, cfg.intermediate_size
    f = lambda *shape, s=1.0: np.ascontiguousarray(s * rng.standard_normal(shape), dtype=np.float32)
    g = lambda: np.ascontiguousarray(rng.uniform(0.7, 1.5, H), dtype=np.float32)
    w = {"embeddings.word_embeddings.weight": f(cfg.vocab_size, H) + np.float32(0.4), "embeddings.token_type_embeddings.weight": f(cfg.type_vocab_size, H, s=0.3),
         "embeddings.LayerNorm.weight": g(), "embeddings.LayerNorm.bias": f(H, s=0.2)}
    for l in range(L):
        p = f"layers.{l}."
        for x, s in (("q", 1.2), ("k", 1.2), ("v", 0.7), ("o", 0.7)):
            w[p + f"self_attn.{x}_proj.weight"] = f(H, H, s=s / H ** 0.5)
            w[p + f"self_attn.{x}_proj.bias"] = f(H, s=0.5)
        w[p + "post_attention_layernorm.weight"] = g()
        w[p + "post_attention_layernorm.bias"] = f(H, s=0.2)
        w[p + "mlp.fc1.weight"] = f(ff, H, s=1.0 / H ** 0.5)
        w[p + "mlp.fc1.bias"] = f(ff, s=0.5)
        w[p + "mlp.fc2.weight"] = f(H, ff, s=1.0 / ff ** 0.5)
        w[p + "mlp.fc2.bias"] = f(H, s=0.5)
        w[p + "post_mlp_layernorm.weight"] = g()
        w[p + "post_mlp_layernorm.bias"] = f(H, s=0.2)
    if pooler:
        w["pooler.dense.weight"] = f(H, H, s=1.0 / H ** 0.5)
        w["pooler.dense.bias"] = f(H, s=0.1)
    return w


def hf_model(cfg, w, device="cpu"):
    from transformers import JinaEmbeddingsV3Model
    m = JinaEmbeddingsV3Model(cfg)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


@torch.no_grad()
def hf_last_hidden(m, ids, mask, chunk=8):
    """last_hidden_state [B, S, H] fp32 (token types zero, positions = columns: HF's defaults)"""
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev)
        k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev)
        outs.append(m(input_ids=a, attention_mask=k).last_hidden_state.float().cpu().numpy())
    return np.concatenate(outs)


class _Mirrored(torch.nn.Module):
    """the rotary module with the sine's sign exchanged between the halves: rotate_half read as (x2, -x1)"""
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, position_ids):
        cos, sin = self.inner(x, position_ids)
        return cos, -sin


class _SwiGLU(torch.nn.Module):
    """fc1 read as NomicBert's gated projection: rows [0, FF / 2) the gate, the rest up, zero-padded back to FF features for fc2"""
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        h = self.inner.fc1(x)
        gate, up = h.chunk(2, dim=-1)
        return self.inner.fc2(torch.cat([torch.nn.functional.silu(gate) * up, torch.zeros_like(up)], dim=-1))


class _Tanh(torch.nn.Module):
    def forward(self, x):
        return torch.nn.functional.gelu(x, approximate="tanh")


BREAKS = ("no_rotation", "mirrored", "no_q_bias", "no_k_bias", "no_o_bias", "no_fc1_bias", "swiglu")
TANH_BREAK = "tanh_gelu"        # asserted only where it clears the margin with these weights (tests/test_gpu_jina3.py says which)


@contextmanager
def broken(m, how):
    """the reference with one part broken"""
    undo = []

    def setattr_(obj, name, val):
        old = getattr(obj, name)
        setattr(obj, name, val)
        undo.append(lambda: setattr(obj, name, old))

    def zero(p):
        keep = p.detach().clone()
        with torch.no_grad():
            p.zero_()
        undo.append(lambda: p.data.copy_(keep))
    try:
        if how == "no_rotation":
            keep = m.rotary_emb.inv_freq.clone()
            m.rotary_emb.inv_freq.zero_()
            undo.append(lambda: m.rotary_emb.inv_freq.copy_(keep))
        elif how == "mirrored":
            setattr_(m, "rotary_emb", _Mirrored(m.rotary_emb))
        elif how in ("no_q_bias", "no_k_bias", "no_o_bias"):
            for l in m.layers:
                zero(getattr(l.self_attn, how[3] + "_proj").bias)
        elif how == "no_fc1_bias":
            for l in m.layers:
                zero(l.mlp.fc1.bias)
        elif how == "swiglu":
            for l in m.layers:
                setattr_(l, "mlp", _SwiGLU(l.mlp))
        elif how == TANH_BREAK:
            for l in m.layers:
                setattr_(l.mlp, "activation_fn", _Tanh())
        else:
            raise ValueError(how)
        yield m
    finally:
        for u in reversed(undo):
            u()


def pool_np(lh, mask, pool):
    """masked mean (pool 0) / column 0 (pool 1) -> L2 normalise"""
    lh = np.asarray(lh, np.float64); mk = np.asarray(mask) != 0
    v = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None] if pool == POOL_MEAN else lh[:, 0]
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
