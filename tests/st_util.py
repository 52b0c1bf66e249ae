"""Shared pieces of the sentence-transformers pipeline tests (tests/test_st_pipeline_host.py, tests/test_gpu_st_pipeline.py, tests/test_gpu_distilbert.py).

sentence-transformers is not installed where these tests run: what its modules compute is RECALLED here, not checked against the package —
  Pooling     cls = column 0; mean = masked mean; max = element-wise max over the attended tokens; mean_sqrt_len = masked sum / sqrt(n); lasttoken = the highest
              attended column
  Dense       activation(linear(x)), activation Identity or Tanh
  Normalize   F.normalize(p=2, dim=1)
— as are the file names and keys of a pipeline folder (modules.json, 1_Pooling/config.json, 2_Dense/config.json + model.safetensors).  The reference of every
parity test is HF's model in fp32 with eager attention followed by `tail_torch`.  Also here: folders written the way sentence-transformers writes them, a tiny
DistilBertModel with synthetic weights, and the ways of breaking the tail that the GPU tests assert as preconditions."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

ST = "sentence_transformers.models."
IDENTITY, TANH = "torch.nn.modules.linear.Identity", "torch.nn.modules.activation.Tanh"
POOL_KEYS = {"cls": "pooling_mode_cls_token", "mean": "pooling_mode_mean_tokens", "max": "pooling_mode_max_tokens", "mean_sqrt_len": "pooling_mode_mean_sqrt_len_tokens",
             "last": "pooling_mode_lasttoken", "weightedmean": "pooling_mode_weightedmean_tokens"}
SETTINGS = ("config.normalize_output", "config.pool_tokens", "config.st_dense_activation")
POOL_TOKENS = {"mean": 0, "max": 1, "mean_sqrt_len": 2}
POOL_MEAN, POOL_CLS, POOL_LAST = 0, 1, 5


def last_index(mask):
    mask = torch.as_tensor(mask) != 0
    cols = torch.arange(mask.shape[1])
    return (mask * (cols + 1)).argmax(dim=1)


def pool_torch(lh, mask, pooling, masked_in_max=False):
    """sentence-transformers' Pooling, one mode, on last_hidden_state [B, S, H] (fp32 or fp64 tensor).  masked_in_max: the broken max that lets masked columns in"""
    lh, mask = torch.as_tensor(lh), torch.as_tensor(mask)
    keep = (mask != 0)[..., None]
    n = (mask != 0).sum(1)[:, None].to(lh.dtype)
    if pooling == "cls":
        return lh[:, 0]
    if pooling == "last":
        return lh[torch.arange(lh.shape[0]), last_index(mask)]
    if pooling == "mean":
        return (lh * keep).sum(1) / n
    if pooling == "mean_sqrt_len":
        return (lh * keep).sum(1) / n.sqrt()
    if pooling == "max":
        return (lh if masked_in_max else lh.masked_fill(~keep, float("-inf"))).max(dim=1).values
    raise ValueError(pooling)


def tail_torch(lh, mask, pooling, W=None, b=None, act="identity", normalize=True, normalize_first=False, masked_in_max=False):
    """Pooling -> Dense(act) -> Normalize in torch, in the precision of `lh`.  normalize_first / masked_in_max: broken variants (Normalize in front of the Dense;
    masked columns inside the max)"""
    x = pool_torch(lh, mask, pooling, masked_in_max)
    if normalize_first:
        x = F.normalize(x, p=2, dim=1)
    if W is not None:
        x = x @ torch.as_tensor(W).to(x.dtype).T
        if b is not None:
            x = x + torch.as_tensor(b).to(x.dtype)
        if act == "tanh":
            x = torch.tanh(x)
    return F.normalize(x, p=2, dim=1) if normalize else x


def write_pipeline(folder, hidden, pooling=("mean",), dense=None, normalize=True, include_prompt=None, extra_modules=(), normalize_before_dense=False,
                   dense_config=None, second_dense=False, torch_bin=False):
    """The pipeline files of a sentence-transformers folder next to whatever model files `folder` holds.  pooling: the modes switched on; dense: None or
    (W [P, hidden], bias [P] or None, IDENTITY / TANH); extra_modules: module types inserted behind the Pooling; dense_config: fields overriding the Dense's
    config.json."""
    os.makedirs(os.path.join(folder, "1_Pooling"), exist_ok=True)
    pc = {"word_embedding_dimension": hidden, **{key: name in pooling for name, key in POOL_KEYS.items()}}
    if include_prompt is not None:
        pc["include_prompt"] = include_prompt
    with open(os.path.join(folder, "1_Pooling", "config.json"), "w") as f:
        json.dump(pc, f)
    mods = [("", ST + "Transformer"), ("1_Pooling", ST + "Pooling")] + [(f"x{i}", t) for i, t in enumerate(extra_modules)]
    if normalize and normalize_before_dense:
        mods.append(("n_Normalize", ST + "Normalize"))
    for d in range(2 if second_dense else 1):
        if dense is None:
            break
        W, b, act = dense
        sub = f"{len(mods)}_Dense"
        os.makedirs(os.path.join(folder, sub), exist_ok=True)
        dc = {"in_features": int(np.asarray(W).shape[1]), "out_features": int(np.asarray(W).shape[0]), "bias": b is not None, "activation_function": act}
        dc.update(dense_config or {})
        with open(os.path.join(folder, sub, "config.json"), "w") as f:
            json.dump(dc, f)
        state = {"linear.weight": torch.as_tensor(np.asarray(W, np.float32)).contiguous()}
        if b is not None:
            state["linear.bias"] = torch.as_tensor(np.asarray(b, np.float32)).contiguous()
        if torch_bin:
            torch.save(state, os.path.join(folder, sub, "pytorch_model.bin"))
        else:
            from safetensors.torch import save_file
            save_file(state, os.path.join(folder, sub, "model.safetensors"))
        mods.append((sub, ST + "Dense"))
    if normalize and not normalize_before_dense:
        mods.append((f"{len(mods)}_Normalize", ST + "Normalize"))
    with open(os.path.join(folder, "modules.json"), "w") as f:
        json.dump([{"idx": i, "name": str(i), "path": p, "type": t} for i, (p, t) in enumerate(mods)], f)


def dense_weights(H, P, seed=11, bias=True, scale=1.0):
    """W ~ N(0, scale^2 / H) [P, H], bias ~ N(0, 0.5^2) [P]: pre-activations of order 1 on rows of order 1, so that tanh bends them and the bias moves them"""
    rng = np.random.default_rng(seed)
    W = np.ascontiguousarray(scale * rng.standard_normal((P, H)) / np.sqrt(H), dtype=np.float32)
    return W, (np.ascontiguousarray(0.5 * rng.standard_normal(P), dtype=np.float32) if bias else None)


# ---- DistilBERT ----
DISTIL_RENAME = (("attention.self.query.", "attention.q_lin."), ("attention.self.key.", "attention.k_lin."), ("attention.self.value.", "attention.v_lin."),
                 ("attention.output.dense.", "attention.out_lin."), ("attention.output.LayerNorm.", "sa_layer_norm."), ("intermediate.dense.", "ffn.lin1."),
                 ("output.dense.", "ffn.lin2."), ("output.LayerNorm.", "output_layer_norm."))


def distil_config(H=128, L=2, heads=2, FF=256, vocab=200, max_pos=160, **extra):
    from transformers import DistilBertConfig
    cfg = DistilBertConfig(dim=H, n_layers=L, n_heads=heads, hidden_dim=FF, vocab_size=vocab, max_position_embeddings=max_pos, dropout=0.0, attention_dropout=0.0,
                           activation="gelu", **extra)
    cfg._attn_implementation = "eager"
    return cfg


def to_distil_names(w):
    """oracle.encoder_np's BERT weights under DistilBertModel's state-dict names (the token-type table dropped)"""
    out = {}
    for k, v in w.items():
        if "token_type_embeddings" in k:
            continue
        k = k.replace("encoder.layer.", "transformer.layer.")
        for a, b in DISTIL_RENAME:
            if a in k:
                k = k.replace(a, b)
                break
        out[k] = v
    return out


def distil_model(cfg, w, device="cpu"):
    from transformers import DistilBertModel
    m = DistilBertModel(cfg)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return m.float().eval().to(device)


@torch.no_grad()
def hf_last_hidden(m, ids, mask, chunk=8, **kw):
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev); k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev)
        extra = {n: torch.from_numpy(np.ascontiguousarray(v[i:i + chunk])).to(dev) for n, v in kw.items()}
        outs.append(m(input_ids=a, attention_mask=k, **extra).last_hidden_state.float().cpu().numpy())
    return np.concatenate(outs)


def tokens(B, S, layout, seed, vocab=200, holes=0, lens=None):
    """(ids, mask) [B, S] int64: R = right-padded (ragged lengths in [S / 2, S], row 0 full unless `lens`), L = left-padded; `holes`: that many attended columns
    of every row (never its first or last) masked out again"""
    rng = np.random.default_rng(seed)
    real = rng.integers(3, vocab, (B, S))
    n = rng.integers(max(2, S // 2), S + 1, B) if lens is None else np.asarray(lens)
    if lens is None:
        n[0] = S
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
