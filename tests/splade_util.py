"""Shared pieces of the SPLADE tests (tests/test_splade_host.py, tests/test_gpu_splade.py): synthetic BERT backbones (oracle.encoder_np's weights) of both head
widths with a seeded MLM head, the reference — ``transformers.BertForMaskedLM`` in fp32 with eager attention, ``log1p(relu(logits))`` max-pooled over the
attended columns in fp64 —, the same head restated by hand in fp64 with ONE part broken at a time (the teeth), and the batches of the parity cases."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import encoder_np as E  # noqa: E402

H, LAYERS, FF = 128, 2, 256
MAX_POS = 320
HEAD_COUNTS = {"h32": 4, "h64": 2}          # 4 heads of 32, 2 heads of 64
VOCABS = (1031, 1280)                       # odd (padded to 1152 inside the library) and an exact multiple of the column granularity
PAD, CLS, SEP = 0, 2, 3
MLM = ("cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias", "cls.predictions.transform.LayerNorm.weight",
       "cls.predictions.transform.LayerNorm.bias", "cls.predictions.decoder.weight", "cls.predictions.decoder.bias")
LN_EPS = 1e-12
# Bar on |w - reference w| over all B x V entries: twice the worst value measured over the parity cases of tests/test_gpu_splade.py against the fp32 reference
# on one MI355X (profiles/splade/measurements.txt, section 1), rounded up to two significant digits.  The kernels are deterministic (max is exact); the
# factor covers reordering noise between runs of the HF side.
# measured worst: 3.4594e-03 (h32, V = 1031, S = 40, right padding) on weights up to 2.2: the transform's rows t are rounded to f16 twice (behind the GELU and
# behind the LayerNorm) before the decoder reads them, and a logit is a sum of 128 such products of standard deviation ~2
BAR = 7.0e-3
MUTATIONS = ("no_layernorm", "no_gelu", "no_bias", "no_log1p", "no_relu", "mean_pool", "masked_columns", "neighbour_row")
ZERO_SHARE = (0.30, 0.90)                   # the reference's own share of exact zeros per parity case: the ReLU is exercised, not everything is clipped


def backbone(V, seed=3):
    return dict(E.synth_weights(H, LAYERS, FF, V, MAX_POS, seed=seed))


def head(V, seed=41, bias=None):
    """The six head tensors, seeded.  t (a LayerNorm output) has unit-scale elements, so a decoder ~ N(0, 4 / H) gives logits of standard deviation about 2.
    The decoder bias is uniform in [-8, -0.5]: the max over a sequence's tokens of such logits lies between about 1 and 6 for 1 .. 300 tokens, so the ReLU cuts a
    different share of the columns at every length (the tests assert the share on the reference)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = lambda *s: rng.standard_normal(s)
    w = {MLM[0]: f(H, H) * 1.5 / np.sqrt(H), MLM[1]: 0.3 * f(H), MLM[2]: 1.0 + 0.1 * f(H), MLM[3]: 0.1 * f(H), MLM[4]: f(V, H) * 2.0 / np.sqrt(H),
         MLM[5]: rng.uniform(-8.0, -0.5, V) if bias is None else np.full(V, bias)}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def lib_cfg(kind, V):
    from types import SimpleNamespace
    return SimpleNamespace(hidden_size=H, num_hidden_layers=LAYERS, num_attention_heads=HEAD_COUNTS[kind], intermediate_size=FF, vocab_size=V,
                           max_position_embeddings=MAX_POS, type_vocab_size=2, layer_norm_eps=LN_EPS, hidden_act="gelu", model_type="bert", pad_token_id=PAD)


def hf_config(kind, V, tie=False):
    from transformers import BertConfig
    return BertConfig(hidden_size=H, num_hidden_layers=LAYERS, num_attention_heads=HEAD_COUNTS[kind], intermediate_size=FF, vocab_size=V,
                      max_position_embeddings=MAX_POS, type_vocab_size=2, layer_norm_eps=LN_EPS, pad_token_id=PAD, attn_implementation="eager",
                      hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, tie_word_embeddings=tie)


def hf_state(w, tie=False):
    """library names -> BertForMaskedLM's state dict (``bert.`` prefix on the backbone; both spellings of the decoder bias)"""
    sd = {(k if k.startswith("cls.") else "bert." + k): torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    sd["cls.predictions.bias"] = sd[MLM[5]]
    if tie:
        sd.pop(MLM[4], None)
    return sd


def hf_mlm(kind, V, w, device="cpu", cls=None, tie=False):
    """``BertForMaskedLM`` (or ``cls``, a subclass: the library's twin) in fp32 with eager attention over the tensors of ``w``.  ``tie``: the decoder's weight IS
    the word table (HF's default for real checkpoints); ``w`` then holds no decoder weight of its own."""
    from transformers import BertForMaskedLM
    m = (cls or BertForMaskedLM)(hf_config(kind, V, tie))
    res = m.load_state_dict(hf_state(w, tie), strict=False)
    assert not res.unexpected_keys and all("position_ids" in k or k == MLM[4] for k in res.missing_keys), res
    if tie:
        assert m.cls.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    return m.float().eval().to(device)


def _t(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)          # a copy: the cached case arrays are read-only


def pool_logits(logits, mask, broken=None):
    """[B, S, V] float64 logits -> [B, V]: max over the attended columns of log1p(relu(.)), 0 for a row without attended columns"""
    k = torch.from_numpy(np.asarray(mask)).bool()
    if broken == "no_relu":
        v = torch.sign(logits) * torch.log1p(logits.abs())          # no clipping at zero: negative logits stay negative
    elif broken == "no_log1p":
        v = torch.relu(logits)
    else:
        v = torch.log1p(torch.relu(logits))
    if broken == "masked_columns":
        k = torch.ones_like(k)
    if broken == "neighbour_row":        # sequence b also sees the first attended row of sequence b + 1
        B = v.shape[0]
        first = torch.stack([v[(b + 1) % B][int(torch.nonzero(k[(b + 1) % B])[0])] if k[(b + 1) % B].any() else torch.zeros_like(v[0, 0]) for b in range(B)])
    if broken == "mean_pool":
        out = (v * k[..., None]).sum(1) / k.sum(1).clamp(min=1)[:, None]
    else:
        out = torch.where(k[..., None], v, torch.full_like(v, -np.inf)).max(dim=1).values
        if broken == "neighbour_row":
            out = torch.maximum(out, first)
        out = torch.where(k.any(1)[:, None], out, torch.zeros_like(out))
    return out.numpy()


@torch.no_grad()
def reference(m, ids, mask):
    """THE reference: ``BertForMaskedLM(...).logits`` in fp32, the formula in fp64 -> [B, V] float64"""
    dev = next(m.parameters()).device
    logits = m(input_ids=_t(ids, dev), attention_mask=_t(mask, dev)).logits.double().cpu()
    return pool_logits(logits, mask)


@torch.no_grad()
def by_hand(m, w, ids, mask, broken=None):
    """the same head restated from the backbone's last_hidden_state in fp64, whole or with ONE part broken (MUTATIONS)"""
    dev = next(m.parameters()).device
    x = m.bert(input_ids=_t(ids, dev), attention_mask=_t(mask, dev)).last_hidden_state.double().cpu()
    Wt, bt, g, b, Wd, bd = (torch.from_numpy(np.asarray(w[k], np.float64)) for k in MLM)
    t = x @ Wt.T + bt
    if broken != "no_gelu":
        t = torch.nn.functional.gelu(t)
    if broken != "no_layernorm":
        t = torch.nn.functional.layer_norm(t, (H,), g, b, LN_EPS)
    logits = t @ Wd.T + (0 if broken == "no_bias" else bd)
    return pool_logits(logits, mask, broken)


def batch(V, lens, S, variant="right", seed=0):
    """(ids, mask) [B, S] int64, one row per entry of ``lens`` (0: an all-masked row): [CLS] w .. [SEP] with pad 0.  variant: "right" / "left" = where the padding
    goes; "holes" = right padding with up to a third of each row's interior columns masked (their ids stay) and, in every second row, column 0 masked too."""
    rng = np.random.default_rng(seed)
    B = len(lens)
    ids = np.full((B, S), PAD, np.int64); mask = np.zeros((B, S), np.int64)
    for r, n in enumerate(lens):
        if n == 0:
            ids[r] = rng.integers(10, V, S)          # ids under a zero mask: they must not matter
            continue
        row = [CLS, *rng.integers(10, V, max(n - 2, 0)), SEP][:n]
        sl = slice(S - n, S) if variant == "left" else slice(0, n)
        ids[r, sl] = row; mask[r, sl] = 1
        if variant == "holes" and n > 4:
            inner = np.arange(1, n - 1)
            mask[r, rng.choice(inner, size=len(inner) // 3, replace=False)] = 0
            if r % 2 == 1:
                mask[r, 0] = 0
    return ids, mask


def random_lens(B, S, seed, min_len=4):
    rng = np.random.default_rng(seed)
    return [S] + [int(rng.integers(min_len, S + 1)) for _ in range(B - 1)]


# the parity cases: name -> (lens, S, variant).  S = 12 / 40 / 150 with right and left padding and holes; "ragged" puts sequence boundaries inside 32-row blocks
# and makes the packed total no multiple of 32; "long" spans more than one 256-row tile; "masked" holds an all-masked row between two others
CASES = {f"s{S}_{v}": (random_lens(5, S, S), S, v) for S in (12, 40, 150) for v in ("right", "left", "holes")}
CASES["ragged"] = ([5, 7, 33, 1, 64], 64, "right")
CASES["long"] = ([300], 300, "right")
CASES["masked"] = ([9, 0, 21], 24, "right")


def case_batch(name, V):
    lens, S, variant = CASES[name]
    return batch(V, lens, S, variant, seed=len(name) + S)


def zero_share(ref):
    return float((np.asarray(ref) == 0).mean())


# ---- end to end (SpladeModel): a tied model, as real checkpoints are ----
def tied_weights(V, seed=3):
    """backbone + head WITHOUT a decoder weight of its own: the word table, scaled so that the tied logits are of order 1"""
    w = backbone(V, seed)
    w["embeddings.word_embeddings.weight"] = np.ascontiguousarray(w["embeddings.word_embeddings.weight"] * 8.0, dtype=np.float32)
    hw = head(V)
    hw.pop(MLM[4])
    return {**w, **hw}


def ref_token_weights(vec, tok, bar, top_k=None):
    """the reference's own dict building, restated: weights > 0 without the pad id, optionally the top_k largest"""
    items = [(i, float(x)) for i, x in enumerate(vec) if x > 0 and i != tok.pad_token_id]
    if top_k is not None:
        items = sorted(items, key=lambda t: (-t[1], t[0]))[:top_k]
    return {tok.convert_ids_to_tokens(i): x for i, x in items}
