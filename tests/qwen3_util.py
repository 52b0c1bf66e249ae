"""Shared pieces of the Qwen3 tests (tests/test_qwen3_host.py, tests/test_gpu_qwen3.py): tiny Qwen3 configs whose head_dim is a field of its own, synthetic
weights under HF's state-dict names, the HF fp32 eager reference (transformers.Qwen3Model; its masks, pooling and token layouts come from decoder_util) and the
ways of breaking what is new in this family — the q / k norms, the order of norm and rotation, the score scale, the rotary partner — that the GPU tests assert
as preconditions on the CPU.

Shapes (2 layers, FF 256, vocab 200): q3-128 = hidden 128, 2 heads of 128 over 1 KV head (Dq 256, A 128); q3-128g = 4 heads of 128 over 2 (Dq 512, A 256);
q3-64 = 4 heads of 64 over 2 on hidden 128 (Dq 256: decoupled at the old width, the one case that takes k_attn_dma with Dq != hidden).

Weights.  decoder_util's recipe with q_proj [Dq, H], k / v [A, H], o [H, Dq].  The q / k norm weights are random around 1 (uniform in [0.6, 1.6]), not ones,
and q's are multiplied by 2.5: behind an RMS norm q and k have unit RMS whatever the projections are, so q . k / sqrt(d_h) has a standard deviation of about
gamma_q gamma_k ~ 1.2 — the factor brings the scores to the ~ 3 of the other decoder tests, where the mask, the norms and the rotation decide rows.  The rows
of q_proj / k_proj are scaled per head (0.4 .. 2.0): a per-head norm undoes that, a norm over the whole row does not."""
from contextlib import contextmanager

import numpy as np
import torch

import decoder_util as D

HEAD_DIM_NAME = "config.head_dim"
SETTING, INV_FREQ_NAME = D.SETTING, D.INV_FREQ_NAME
POOL_MEAN, POOL_LAST, POOL_CLASSIFY = D.POOL_MEAN, D.POOL_LAST, 2
FF, VOCAB, MAX_POS = D.FF, D.VOCAB, D.MAX_POS
# kind -> (hidden, heads, head_dim, kv_heads)
SHAPES = {"q3-128": (128, 2, 128, 1), "q3-128g": (128, 4, 128, 2), "q3-64": (128, 4, 64, 2)}


def hf_config(kind, L=2, max_pos=MAX_POS, **extra):
    from transformers import Qwen3Config
    H, heads, hd, kv = SHAPES[kind]
    kw = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, num_key_value_heads=kv, head_dim=hd, intermediate_size=FF, vocab_size=VOCAB,
              max_position_embeddings=max_pos, rms_norm_eps=1e-6, hidden_act="silu", rope_parameters={"rope_theta": 100.0, "rope_type": "default"},
              attention_dropout=0.0, attention_bias=False, tie_word_embeddings=False, pad_token_id=0, use_sliding_window=False)
    kw.update(extra)
    cfg = Qwen3Config(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def weights(cfg, seed=5):
    """HF state-dict name -> fp32 array (Qwen3Model's names, without the "model." prefix)"""
    rng = np.random.default_rng(seed)
    H, L, heads, kv, d = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    f = lambda *shape, s=1.0: np.ascontiguousarray(s * rng.standard_normal(shape), dtype=np.float32)
    g = lambda n=H, lo=0.7, hi=1.5, s=1.0: np.ascontiguousarray(s * rng.uniform(lo, hi, n), dtype=np.float32)
    w = {"embed_tokens.weight": f(cfg.vocab_size, H) + np.float32(0.4)}
    for l in range(L):
        p = f"layers.{l}."
        w[p + "input_layernorm.weight"] = g()
        # the rows of head h scaled by 0.4 .. 2.0: the per-head norm undoes it, one norm over the whole row does not
        per_head = lambda n: np.repeat(np.linspace(0.4, 2.0, n) if n > 1 else np.ones(1), d)[:, None].astype(np.float32)
        w[p + "self_attn.q_proj.weight"] = f(heads * d, H, s=1.2 / H ** 0.5) * per_head(heads)
        w[p + "self_attn.k_proj.weight"] = f(kv * d, H, s=1.2 / H ** 0.5) * per_head(kv)
        w[p + "self_attn.v_proj.weight"] = f(kv * d, H, s=0.7 / H ** 0.5)
        w[p + "self_attn.o_proj.weight"] = f(H, heads * d, s=0.7 / (heads * d) ** 0.5)
        w[p + "self_attn.q_norm.weight"] = g(d, 0.6, 1.6, 2.5)
        w[p + "self_attn.k_norm.weight"] = g(d, 0.6, 1.6)
        w[p + "post_attention_layernorm.weight"] = g()
        w[p + "mlp.gate_proj.weight"] = f(cfg.intermediate_size, H, s=1.0 / H ** 0.5)
        w[p + "mlp.up_proj.weight"] = f(cfg.intermediate_size, H, s=1.0 / H ** 0.5)
        w[p + "mlp.down_proj.weight"] = f(H, cfg.intermediate_size, s=1.0 / cfg.intermediate_size ** 0.5)
    w["norm.weight"] = g()
    return w


def hf_model(cfg, w, device="cpu"):
    from transformers import Qwen3Model
    m = Qwen3Model(cfg)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


hf_last_hidden, pool_np, tokens, last_index = D.hf_last_hidden, D.pool_np, D.tokens, D.last_index

BREAKS = ("no_q_norm", "no_k_norm", "swapped_norms", "norm_after_rope", "row_norm", "hidden_scale", "partner_32", "mean_norm")


def _rms(x, weight, eps, mean=False):
    if mean:
        x = x - x.mean(-1, keepdim=True)
    return weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _rot(x, cos, sin, half):
    """x cos + rotate(x) sin with the partner of feature j at j + half (cyclically inside blocks of 2 half)"""
    shape = x.shape
    y = x.reshape(*shape[:-1], -1, 2 * half)
    y = torch.cat((-y[..., half:], y[..., :half]), dim=-1).reshape(shape)
    return x * cos + y * sin


def _attention(att, how):
    """Qwen3Attention.forward (eager, no cache) with one part broken.  None: HF's own arithmetic restated — test_gpu_qwen3 checks it against HF's forward."""
    import transformers.models.qwen3.modeling_qwen3 as MQ

    def forward(hidden_states, position_embeddings, attention_mask, past_key_values=None, **kwargs):
        B, S, _ = hidden_states.shape
        d, eps = att.head_dim, att.q_norm.variance_epsilon
        q = att.q_proj(hidden_states).view(B, S, -1, d)
        k = att.k_proj(hidden_states).view(B, S, -1, d)
        v = att.v_proj(hidden_states).view(B, S, -1, d).transpose(1, 2)
        gq, gk = att.q_norm.weight, att.k_norm.weight
        if how == "swapped_norms":
            gq, gk = gk, gq
        cos, sin = position_embeddings
        cos, sin = cos.unsqueeze(2), sin.unsqueeze(2)              # [B, S, 1, d]
        half = 32 if how == "partner_32" else d // 2

        def norm(x, g, skip):
            if skip:
                return x
            if how == "row_norm":                                  # one norm over the whole heads x d row
                flat = x.reshape(B, S, -1)
                return (g.repeat(x.shape[2]) * (flat * torch.rsqrt(flat.pow(2).mean(-1, keepdim=True) + eps))).view(x.shape)
            return _rms(x, g, eps, mean=how == "mean_norm")
        if how == "norm_after_rope":
            q, k = norm(_rot(q, cos, sin, half), gq, False), norm(_rot(k, cos, sin, half), gk, False)
        else:
            q, k = _rot(norm(q, gq, how == "no_q_norm"), cos, sin, half), _rot(norm(k, gk, how == "no_k_norm"), cos, sin, half)
        scaling = (att.config.hidden_size // att.config.num_attention_heads) ** -0.5 if how == "hidden_scale" else att.scaling
        out, wts = MQ.eager_attention_forward(att, q.transpose(1, 2), k.transpose(1, 2), v, attention_mask, scaling=scaling, dropout=0.0)
        return att.o_proj(out.reshape(B, S, -1).contiguous()), wts
    return forward


@contextmanager
def broken(m, how):
    """the reference with one part of every layer's attention broken (BREAKS), or with how = None restated unbroken"""
    try:
        for l in m.layers:
            l.self_attn.forward = _attention(l.self_attn, how)
        yield m
    finally:
        for l in m.layers:
            del l.self_attn.forward


def library_settings(cfg, w=None):
    """[(reserved name, values)] in the order the Python layer sends them: the head width, HF's own frequencies, the mask"""
    inv = 1.0 / (cfg.rope_parameters["rope_theta"] ** (np.arange(0, cfg.head_dim, 2, dtype=np.float64) / cfg.head_dim))
    return [(HEAD_DIM_NAME, [float(cfg.head_dim)]), (INV_FREQ_NAME, inv.astype(np.float32)), (SETTING, [1.0])]
