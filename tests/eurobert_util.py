"""Shared pieces of the EuroBERT tests (tests/test_eurobert_host.py, tests/test_gpu_eurobert.py): tiny EuroBertConfig shapes, synthetic weights under HF's
state-dict names (tests/decoder_util.py draws them: EuroBertModel's names are LlamaModel's), the HF fp32 eager reference (transformers.EuroBertModel, whose own
mask is bidirectional) and the ways of breaking it that the GPU tests assert as preconditions."""
from contextlib import contextmanager

import numpy as np
import torch

import decoder_util as D
from decoder_util import POOL_LAST, POOL_MEAN, VOCAB, last_index, mask4d, pool_np, tokens  # noqa: F401

# (H, heads, kv_heads): 2 heads of 64 over 1 KV head, 4 heads of 32 over 2 (A = 64: native), and the 6 x 64 case over 2 KV heads at H = 384
SHAPES = {"euro-64": (128, 2, 1), "euro-32": (128, 4, 2), "euro-384": (384, 6, 2)}
FF, MAX_POS = D.FF, D.MAX_POS


def hf_config(kind, L=2, max_pos=MAX_POS, **extra):
    from transformers import EuroBertConfig
    H, heads, kv = SHAPES[kind]
    kw = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, num_key_value_heads=kv, intermediate_size=FF, vocab_size=VOCAB,
              max_position_embeddings=max_pos, rms_norm_eps=1e-5, hidden_act="silu", rope_parameters={"rope_theta": 100.0, "rope_type": "default"},
              attention_dropout=0.0, tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2, mask_token_id=3)
    kw.update(extra)
    cfg = EuroBertConfig(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def weights(cfg, seed=5):
    """HF state-dict name -> fp32 array (no bias anywhere: the model_type is not qwen2)"""
    return D.weights(cfg, seed)


def hf_model(cfg, w, device="cpu"):
    from transformers import EuroBertModel
    m = EuroBertModel(cfg)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


def hf_last_hidden(m, ids, mask, rule=None, chunk=8):
    """rule None: EuroBertModel's own bidirectional mask from the 2-D attention_mask; else the 4-D mask of decoder_util.RULES[rule] ("causal": the broken one)"""
    return D.hf_last_hidden(m, ids, mask, rule, chunk)


BREAKS = ("causal", "no_rotation", "swapped", "mean_norm", "no_final_norm")


@contextmanager
def broken(m, how):
    """the reference with one part broken: gate and up exchanged, a mean-subtracting norm, no final norm, no rotation (decoder_util.broken)"""
    with D.broken(m, how) as b:
        yield b


def break_distances(m, ids, mask, ref):
    """how far each broken reference moves an attended row of `ref`"""
    keep = np.asarray(mask).astype(bool)
    out = {}
    for how in BREAKS:
        if how == "causal":
            other = hf_last_hidden(m, ids, mask, "causal")
        else:
            with broken(m, how):
                other = hf_last_hidden(m, ids, mask)
        out[how] = float(np.abs(ref - other)[keep].max())
    return out
