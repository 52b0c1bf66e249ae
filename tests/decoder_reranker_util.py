"""Shared pieces of the decoder cross-encoder tests (tests/test_decoder_reranker_host.py, tests/test_gpu_decoder_reranker.py): tiny
Qwen2ForSequenceClassification / LlamaForSequenceClassification models over the configs, weights and token batches of tests/decoder_util.py, HF's fp32 eager
logits, and the float64 score head by hand on HF's last_hidden_state — with the ways of reading the wrong row that the GPU tests assert as preconditions.

Shapes: H 128, 2 layers, FF 256; qwen2-32 = 4 heads of 32 over 2 KV heads with q / k / v biases, llama-64 = 2 heads of 64 over 1.  pad_token_id 0 and ids >= 3
with the ids of masked columns (holes included) set to 0, so attention_mask == (input_ids != pad_token_id): HF's last non-pad token and the library's highest
attended column are the same column.

score.weight is N(0, SCORE_SIGMA^2 / H): final-norm rows have elements of magnitude ~ 1, so logits are ~ N(0, 1.2^2) and reading any other row than the last
attended one (or the right row normalised, or before the final norm) moves some logit of a batch by ~ 1, far above ten times the parity bar.

The causal mask.  The last token attends to every earlier one under either mask, so dropping the mask reaches its logit only through the earlier rows that
layer 2 attends to: with decoder_util's v / o scale (0.7) it moves a logit of these batches by 0.2 - 0.3 at most, measured on the CPU against the HF twins.
The v_proj / o_proj matrices are therefore scaled by VO_SCALE = 2 here (attention contributes as much to the residual stream as the MLP does): no causal
mask then moves a logit by 0.9 (llama-64) and 1.6 (qwen2-32), while HF's own bf16 deviation stays where it was (0.03)."""
import numpy as np
import torch

import decoder_util as D

KINDS = ("qwen2-32", "llama-64")
SCORE_NAME = "score.weight"
SCORE_SIGMA = 1.0
VO_SCALE = 2.0
POOL_CLASSIFY = 2
PAD_ID = 0


def hf_config(kind, labels=1, L=2, **extra):
    return D.hf_config(kind, L=L, num_labels=labels, **extra)


def wide_config(H, labels, L=1):
    """a Qwen2 config of another width for the head kernel alone: H / 64 heads of 64 over 2 KV heads (H 896: Qwen2.5-0.5B's 14 over 2), FF 256"""
    from transformers import Qwen2Config
    cfg = Qwen2Config(hidden_size=H, num_hidden_layers=L, num_attention_heads=H // 64, num_key_value_heads=2, intermediate_size=D.FF, vocab_size=D.VOCAB,
                      max_position_embeddings=D.MAX_POS, rms_norm_eps=1e-6, hidden_act="silu", rope_parameters={"rope_theta": 100.0, "rope_type": "default"},
                      attention_dropout=0.0, tie_word_embeddings=False, pad_token_id=PAD_ID, num_labels=labels)
    cfg._attn_implementation = "eager"
    return cfg


def score_weight(H, labels, seed=11):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(SCORE_SIGMA / H ** 0.5 * rng.standard_normal((labels, H)), dtype=np.float32)


def weights(cfg, seed=5):
    """the library's names -> fp32 arrays: the backbone of decoder_util.weights plus score.weight [num_labels, H]"""
    w = D.weights(cfg, seed)
    for k in w:
        if k.endswith(("self_attn.v_proj.weight", "self_attn.o_proj.weight")):
            w[k] = w[k] * np.float32(VO_SCALE)
    w[SCORE_NAME] = score_weight(cfg.hidden_size, cfg.num_labels)
    return w


def hf_state(w):
    """the same tensors under the ...ForSequenceClassification names: the backbone behind `model.`"""
    return {(k if k == SCORE_NAME else "model." + k): torch.from_numpy(np.asarray(v)) for k, v in w.items()}


def hf_classifier(cfg, w, cls=None):
    from transformers import LlamaForSequenceClassification, Qwen2ForSequenceClassification
    cls = cls or (Qwen2ForSequenceClassification if cfg.model_type == "qwen2" else LlamaForSequenceClassification)
    m = cls(cfg)
    res = m.load_state_dict(hf_state(w), strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval()


def pairs(B, S, layout, seed, lens=None, holes=0):
    """decoder_util.tokens: ids in [3, VOCAB) at attended columns, PAD_ID at every other (padding and holes)"""
    ids, mask = D.tokens(B, S, layout, seed, lens=lens, holes=holes)
    assert ((ids != PAD_ID) == (mask != 0)).all()
    return ids, mask


@torch.no_grad()
def hf_logits(m, ids, mask, chunk=8):
    """[B, L] float64: the HF class's own forward (its causal mask from the 2-D attention_mask, its last non-pad token)"""
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])); k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk]))
        outs.append(m(input_ids=a, attention_mask=k).logits.double().numpy())
    return np.concatenate(outs)


def hf_last_non_pad(ids, pad=PAD_ID):
    """GenericForSequenceClassification's column: the rightmost one whose id is not the pad id"""
    ids = torch.from_numpy(np.asarray(ids))
    return ((torch.arange(ids.shape[-1], dtype=torch.int32) * (ids != pad).to(torch.int32)).argmax(-1)).numpy()


def head_by_hand(lh, mask, score, row="last"):
    """[B, L] float64 = score . x on a last_hidden_state [B, S, H]: x the row of the highest attended column ("last": the feature), that row L2-normalised, the
    masked mean, the first attended row, or the NEXT sequence's last row"""
    lh = np.asarray(lh, np.float64); mk = np.asarray(mask) != 0
    B = len(lh)
    last = D.last_index(mask)
    if row == "mean":
        x = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None]
    elif row == "first":
        x = lh[np.arange(B), np.argmax(mk, axis=1)]
    elif row == "neighbour":
        nb = (np.arange(B) + 1) % B
        x = lh[nb, last[nb]]
    else:
        x = lh[np.arange(B), last]
        if row == "normalised":
            x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return x @ np.asarray(score, np.float64).T


def reference_by_hand(m, ids, mask, row="last", rule=None, how=None):
    """the float64 head on the backbone's fp32 last_hidden_state; rule: a 4-D mask of decoder_util.RULES in the place of HF's causal one ("none": every attended
    key); how: one of decoder_util.broken's model breaks ("no_final_norm")"""
    score = m.score.weight.detach().double().numpy()
    if how is None:
        lh = D.hf_last_hidden(m.model, ids, mask, rule)
    else:
        with D.broken(m.model, how):
            lh = D.hf_last_hidden(m.model, ids, mask, rule)
    return head_by_hand(lh, mask, score, row)


# the ways of computing something else that the parity bar must tell from the feature: (row, rule, how)
TEETH = {"normalised row": ("normalised", None, None), "mean row": ("mean", None, None), "first row": ("first", None, None),
         "neighbour's last row": ("neighbour", None, None), "row before the final norm": ("last", None, "no_final_norm"), "no causal mask": ("last", "none", None)}


def gamma(n):
    """the constant of the standard a-priori bound on an fp32 sum of n products: n u / (1 - n u), u = 2^-24"""
    u = 2.0 ** -24
    return n * u / (1 - n * u)
