"""Shared pieces of the decoder-LLM embedder tests (tests/test_decoder_host.py, tests/test_gpu_decoder.py): tiny Qwen2 / Llama configs, synthetic weights under
HF's state-dict names, the HF fp32 eager reference (transformers.Qwen2Model / LlamaModel) under its own causal mask or under a hand-made 4-D mask, numpy
pooling, and the ways of breaking the reference that the GPU tests assert as preconditions.

Weights.  Embedding rows N(0.4, 1) (a non-zero mean, so that a mean-subtracting norm differs from the RMS norm); norm weights in [0.7, 1.5]; q / k matrices
N(0, 1.2^2 / H) and q / k biases N(0, 0.5^2): scores q.k / sqrt(d_h) have a standard deviation of ~ 1.5 - 2 and stay below ~ 8 over 300 keys, so the 2^-11
relative rounding of f16 q and k moves a score by <= 8e-3 and a probability by < 1 % — a third of the 3e-2 bar on rows of magnitude ~ 1 — while the mask, the
biases and the rotation (rope_theta 100: the angles matter at a distance of a few tokens) still decide rows: measured on the CPU against the HF twins, the
weakest broken reference (no rotation) differs by 1.0, every other by >= 1.8, against the required 0.3.  v / o N(0, 0.7^2 / H), MLP N(0, 1 / fan_in)."""
from contextlib import contextmanager

import numpy as np
import torch

SETTING = "config.decoder_attention"
INV_FREQ_NAME = "config.rotary_inv_freq"
POOL_MEAN, POOL_LAST = 0, 5
# (model_type, H, heads, kv_heads): 4 heads of 32 over 2 KV heads, 2 heads of 64 over 1, and the 6 x 64 case over 2 (tile pairs of q / k rows across 3 KV groups)
SHAPES = {"qwen2-32": ("qwen2", 128, 4, 2), "llama-64": ("llama", 128, 2, 1), "qwen2-384": ("qwen2", 384, 6, 2), "llama-32": ("llama", 128, 4, 2)}
FF, VOCAB, MAX_POS = 256, 200, 512


def hf_config(kind, L=2, max_pos=MAX_POS, **extra):
    from transformers import LlamaConfig, Qwen2Config
    mt, H, heads, kv = SHAPES[kind]
    kw = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, num_key_value_heads=kv, intermediate_size=FF, vocab_size=VOCAB,
              max_position_embeddings=max_pos, rms_norm_eps=1e-6, hidden_act="silu", rope_parameters={"rope_theta": 100.0, "rope_type": "default"},
              attention_dropout=0.0, tie_word_embeddings=False, pad_token_id=0)
    kw.update(extra)
    cfg = (Qwen2Config if mt == "qwen2" else LlamaConfig)(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def weights(cfg, seed=5):
    """HF state-dict name -> fp32 array (q / k / v biases for qwen2 only, as in HF)"""
    rng = np.random.default_rng(seed)
    H, L, heads, kv = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads
    d = H // heads
    f = lambda *shape, s=1.0: np.ascontiguousarray(s * rng.standard_normal(shape), dtype=np.float32)
    g = lambda: np.ascontiguousarray(rng.uniform(0.7, 1.5, H), dtype=np.float32)
    w = {"embed_tokens.weight": f(cfg.vocab_size, H) + np.float32(0.4)}
    for l in range(L):
        p = f"layers.{l}."
        w[p + "input_layernorm.weight"] = g()
        w[p + "self_attn.q_proj.weight"] = f(H, H, s=1.2 / H ** 0.5)
        w[p + "self_attn.k_proj.weight"] = f(kv * d, H, s=1.2 / H ** 0.5)
        w[p + "self_attn.v_proj.weight"] = f(kv * d, H, s=0.7 / H ** 0.5)
        w[p + "self_attn.o_proj.weight"] = f(H, H, s=0.7 / H ** 0.5)
        if cfg.model_type == "qwen2":
            w[p + "self_attn.q_proj.bias"] = f(H, s=0.5)
            w[p + "self_attn.k_proj.bias"] = f(kv * d, s=0.5)
            w[p + "self_attn.v_proj.bias"] = f(kv * d, s=0.5)
        w[p + "post_attention_layernorm.weight"] = g()
        w[p + "mlp.gate_proj.weight"] = f(cfg.intermediate_size, H, s=1.0 / H ** 0.5)
        w[p + "mlp.up_proj.weight"] = f(cfg.intermediate_size, H, s=1.0 / H ** 0.5)
        w[p + "mlp.down_proj.weight"] = f(H, cfg.intermediate_size, s=1.0 / cfg.intermediate_size ** 0.5)
    w["norm.weight"] = g()
    return w


def hf_model(cfg, w, device="cpu"):
    from transformers import LlamaModel, Qwen2Model
    m = (Qwen2Model if cfg.model_type == "qwen2" else LlamaModel)(cfg)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


def expanded_config(cfg):
    """the same model with one KV head per query head"""
    d = cfg.to_dict()
    d["num_key_value_heads"] = cfg.num_attention_heads
    out = type(cfg)(**{k: v for k, v in d.items() if k not in ("model_type", "transformers_version", "architectures")})
    out._attn_implementation = "eager"
    return out


# which key columns a query column admits (besides the padding mask)
RULES = {"causal": lambda q, k: k <= q, "none": lambda q, k: np.ones_like(k <= q), "mirrored": lambda q, k: k >= q, "strict": lambda q, k: k < q}


def mask4d(mask, rule):
    """[B, 1, S, S] additive fp32 mask: 0 where key column k is attended and RULES[rule] admits it for query column q, else the most negative float"""
    mask = np.asarray(mask)
    B, S = mask.shape
    q, k = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    ok = RULES[rule](q, k)[None] & (mask != 0)[:, None, :]
    return torch.from_numpy(np.where(ok, 0.0, np.finfo(np.float32).min).astype(np.float32))[:, None]


@torch.no_grad()
def hf_last_hidden(m, ids, mask, rule=None, chunk=8):
    """last_hidden_state [B, S, H] fp32: rule None = HF's own causal mask from the 2-D attention_mask, else the 4-D mask of RULES[rule]"""
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev)
        k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev) if rule is None else mask4d(mask[i:i + chunk], rule).to(dev)
        outs.append(m(input_ids=a, attention_mask=k).last_hidden_state.float().cpu().numpy())
    return np.concatenate(outs)


class _MeanNorm(torch.nn.Module):
    """the norm with the mean subtracted (LayerNorm without a bias) in the place of an RMS norm"""
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        x = x - x.mean(-1, keepdim=True)
        return self.inner.weight * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.inner.variance_epsilon)


MODEL_BREAKS = ("no_bias", "mean_norm", "no_final_norm", "swapped", "no_rotation")
MASK_BREAKS = ("none", "mirrored", "strict")


@contextmanager
def broken(m, how):
    """the reference with one part broken: q / k / v biases dropped, a mean-subtracting norm, no final norm, gate and up exchanged, no rotation"""
    undo = []
    def setattr_(obj, name, val):
        old = getattr(obj, name)
        setattr(obj, name, val)
        undo.append(lambda: setattr(obj, name, old))
    def swap():
        with torch.no_grad():
            for l in m.layers:
                g = l.mlp.gate_proj.weight.clone()
                l.mlp.gate_proj.weight.copy_(l.mlp.up_proj.weight); l.mlp.up_proj.weight.copy_(g)
    try:
        if how == "no_bias":
            for l in m.layers:
                for p in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj):
                    if p.bias is not None:
                        keep = p.bias.detach().clone()
                        with torch.no_grad():
                            p.bias.zero_()
                        undo.append(lambda p=p, keep=keep: p.bias.data.copy_(keep))
        elif how == "mean_norm":
            for l in m.layers:
                setattr_(l, "input_layernorm", _MeanNorm(l.input_layernorm)); setattr_(l, "post_attention_layernorm", _MeanNorm(l.post_attention_layernorm))
            setattr_(m, "norm", _MeanNorm(m.norm))
        elif how == "no_final_norm":
            setattr_(m, "norm", torch.nn.Identity())
        elif how == "swapped":
            swap(); undo.append(swap)
        elif how == "no_rotation":
            keep = m.rotary_emb.inv_freq.clone()
            m.rotary_emb.inv_freq.zero_()
            undo.append(lambda: m.rotary_emb.inv_freq.copy_(keep))
        else:
            raise ValueError(how)
        yield m
    finally:
        for u in reversed(undo):
            u()


def has_bias(m):
    return m.layers[0].self_attn.q_proj.bias is not None


def last_index(mask):
    """per row the highest attended column (-1: none)"""
    mask = np.asarray(mask) != 0
    S = mask.shape[1]
    return np.where(mask.any(1), S - 1 - np.argmax(mask[:, ::-1], axis=1), -1)


def pool_np(lh, mask, pool):
    """masked mean (pool 0) / the row of the highest attended column (pool 5) -> L2 normalise"""
    lh = np.asarray(lh, np.float64); mk = np.asarray(mask) != 0
    v = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None] if pool == POOL_MEAN else lh[np.arange(len(lh)), last_index(mask)]
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def tokens(B, S, layout, seed, lens=None, holes=0):
    """(ids, mask) [B, S] int64, ids in [3, VOCAB): R = right-padded (ragged lengths in [S / 2, S], row 0 full unless `lens` is given), L = left-padded,
    F = full; `holes` > 0: that many attended columns of every row (never its first or last) are masked out again"""
    rng = np.random.default_rng(seed)
    real = rng.integers(3, VOCAB, (B, S))
    n = rng.integers(max(2, S // 2), S + 1, B) if lens is None else np.asarray(lens)
    if lens is None:
        n[0] = S
    if layout == "F":
        n = np.full(B, S)
    ids = np.zeros((B, S), np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        k = int(n[r])
        sl = slice(S - k, S) if layout == "L" else slice(0, k)
        ids[r, sl] = real[r, :k]; mask[r, sl] = 1
        cols = np.flatnonzero(mask[r])
        if holes and len(cols) > 2:
            drop = rng.choice(cols[1:-1], size=min(holes, len(cols) - 2), replace=False)
            mask[r, drop] = 0; ids[r, drop] = 0
    return ids, mask
