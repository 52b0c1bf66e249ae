"""Shared pieces of the token-level tests of the plain BERT path (tests/test_encoder_teeth_host.py, tests/test_gpu_encoder_tokens.py): weights under which
attention decides the output, a planted key that every query attends to, the fp64 forward of oracle.encoder_np with hooks for the ways a kernel could be
wrong (the mutants), and an emulation of 16-bit MFMA operands with fp64 accumulation.  numpy only; the oracle itself stays the restatement of the reference.

Why.  oracle.encoder_np.synth_weights draws every matrix from N(0, 0.02^2): at H = 128 the pre-softmax scores have a standard deviation of about 0.05 and the
softmax is uniform to a few percent, so a wrong score scale, a lost key or a swapped head moves no row of last_hidden_state by more than the 16-bit noise.
sharp_weights scales the layer matrices to sigma sqrt(H) = 1.57 (the rule tests/test_gpu_nomic.py documents), and plant() makes one key win every softmax."""
import math
from functools import lru_cache

import numpy as np

from oracle import encoder_np as E

BAR = 3e-2                  # the project's per-token bar of the default mode (test_g1_last_hidden_state; HIDDEN_BAR of the family tests)
SIGMA_SQRT_H = 1.57         # layer matrices N(0, sigma^2) with sigma sqrt(H) = 1.57: 0.139 at H = 128 (synth_weights x 7)
TOKEN = 4                   # the planted token id; every other id of a planted batch is drawn from [5, vocab)
VOCAB, MAX_POS = 1000, 512
MODES = (("f16", True), ("f16", False), ("bf16", True), ("bf16", False))      # (operand type, residual low half); the first is the default

MUTANTS = ("drop_key", "scale_other_dh", "scale_ln2", "heads_swapped", "no_bv", "pos_rank", "holes_ignored", "type_ignored", "cls_first_attended")


def sharp_weights(H, L, heads, FF, vocab=VOCAB, max_pos=MAX_POS, seed=0, sigma_sqrt_h=SIGMA_SQRT_H):
    """E.synth_weights with every layer matrix scaled to sigma sqrt(H) = `sigma_sqrt_h`, the linear biases x 10 and the position table x 0.25 (so that the
    token, not its column, decides which key a query prefers).  `heads` does not enter the draw; it is an argument so that a call names the whole shape."""
    w = E.synth_weights(H, L, FF, vocab, max_pos, seed=seed)
    scale = sigma_sqrt_h / (0.02 * math.sqrt(H))
    out = {}
    for name, v in w.items():
        v = np.asarray(v, np.float64)
        if name.startswith("encoder.layer.") and "LayerNorm" not in name:
            v = v * (scale if name.endswith(".weight") else 10.0)
        elif name == "embeddings.position_embeddings.weight":
            v = v * 0.25
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def plant(w, heads, c=12.0, token=TOKEN):
    """a copy of `w` whose layer-0 query bias is c * k_h per head, k_h the unit vector along W_k LN_emb(word[token] + type[0]) restricted to head h: every query
    of layer 0 then scores the key that holds `token` about c * 1.57 above the others, wherever it lies"""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    x = E.layer_norm(W["embeddings.word_embeddings.weight"][token] + W["embeddings.token_type_embeddings.weight"][0],
                     W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], 1e-12)
    k = W["encoder.layer.0.attention.self.key.weight"] @ x
    H = k.shape[0]
    kh = k.reshape(heads, H // heads)
    kh = kh / np.linalg.norm(kh, axis=1, keepdims=True)
    out = dict(w)
    out["encoder.layer.0.attention.self.query.bias"] = np.ascontiguousarray(c * kh.reshape(H), dtype=np.float32)
    return out


def planted_batch(S, pairs, layout, seed, vocab=VOCAB, token=TOKEN):
    """One sequence per (n, j): n attended tokens, `token` at attended index j, every other attended id random in [5, vocab), masked columns hold id 0.
    Layouts: R right-padded, L left-padded, H = up to three masked columns ahead of the planted one and the rest of the padding on the right, so that the
    attended index differs from the column (for j = 0 the holes are columns 0.., so column 0 is masked).  A sequence that fills its row (n = S) has no room
    for holes: under H it is made of n - 2 tokens, j clipped to the last.  -> (ids, mask [B,S] int64, j [B] as planted, n [B])"""
    rng = np.random.default_rng(seed)
    B = len(pairs)
    ids = np.zeros((B, S), np.int64); mask = np.zeros((B, S), np.int64)
    js = np.zeros(B, np.int64); ns = np.zeros(B, np.int64)
    for b, (n, j) in enumerate(pairs):
        assert 1 <= n <= S and 0 <= j < n
        if layout == "R":
            cols = np.arange(n)
        elif layout == "L":
            cols = np.arange(S - n, S)
        elif layout == "H":
            if n == S:
                n = n - 2; j = min(j, n - 1)
            g = min(3, S - n)
            holes = np.arange(g) if j == 0 else rng.choice(np.arange(1, j + g), g, replace=False)
            cols = np.setdiff1d(np.arange(S), holes)[:n]
            assert cols[j] == j + g
        else:
            raise ValueError(layout)
        tok = rng.integers(5, vocab, n)
        tok[j] = token
        ids[b, cols] = tok; mask[b, cols] = 1
        js[b] = j; ns[b] = n
    return ids, mask, js, ns


# section 3A of the tests: S -> [(n, j)], the attended length and the planted attended index, at every tile edge of both attention kernels
def _pairs(ns, js):
    out = []
    for n in ns:
        for j in sorted({(n - 1 if j is None else j) for j in js if j is None or j < n}):
            out.append((n, j))
    return out


PLANTED = {32: _pairs((2, 31, 32), (0, None)),
           64: _pairs((33, 63, 64), (0, 31, 32, None)),
           128: _pairs((65, 96, 127, 128), (0, 63, 64, None)),
           300: _pairs((129, 193, 257, 300), (0, 63, 64, 127, 128, 191, 192, 255, 256, None))}
LAYOUTS = ("R", "L", "H")
DH = {64: 2, 32: 4}         # head width -> heads at H = 128
TINY = dict(H=128, L=2, FF=512)


@lru_cache(maxsize=None)
def planted_model(dh, c=12.0):
    heads = DH[dh]
    return plant(sharp_weights(TINY["H"], TINY["L"], heads, TINY["FF"], seed=21), heads, c=c)


@lru_cache(maxsize=None)
def planted_case(S, layout):
    return planted_batch(S, PLANTED[S], layout, seed=100 * S + ord(layout))


# section 3B: generic sharp weights (no plant), four batches of B = 4, token types on half the rows
GENERIC = ((33, "R"), (65, "L"), (129, "H"), (200, "R"))


@lru_cache(maxsize=None)
def generic_model():
    """The token-type table stays as drawn: its second row already moves a typed row by >= 1.0 (type_ignored), and scaling it up blunts the attention of the
    typed tokens (x 2: the score-scale mutants fall from 0.4 to 0.17, x 4 to 0.04) because the type then outweighs the word in the embedding."""
    return sharp_weights(TINY["H"], TINY["L"], 2, TINY["FF"], seed=26)


@lru_cache(maxsize=None)
def generic_case(S, layout, B=4):
    """(ids, mask, token types): ragged lengths in [S / 2, S], row 0 full (minus the holes); H = three masked columns inside every sequence and column 0 masked
    in row 1; half the rows carry token type 1: row 1 from column S / 2 on, row 3 up to it (two segments in either order)"""
    rng = np.random.default_rng(7000 + S)
    ids = np.zeros((B, S), np.int64); mask = np.zeros((B, S), np.int64)
    lens = rng.integers(S // 2, S + 1, B); lens[0] = S
    for b in range(B):
        n = int(lens[b])
        if layout == "L":
            mask[b, S - n:] = 1
        else:
            mask[b, :n] = 1
        if layout == "H":
            mask[b, rng.choice(np.arange(1, n - 1), 3, replace=False)] = 0
    if layout == "H":
        mask[1, 0] = 0
    ids[mask != 0] = rng.integers(5, VOCAB, int(mask.sum()))
    tt = np.zeros((B, S), np.int64)
    tt[1, S // 2:] = 1; tt[3, :S // 2] = 1
    return ids, mask, tt


# section 3C: (H, heads, FF) that no test has run: the LayerNorm / pooling instantiations above 1024, odd multiples of 128 as the intermediate size, 640 / 896
WIDTHS = ((128, 4, 128), (640, 10, 1152), (896, 28, 896), (1280, 40, 1408), (1280, 20, 1280), (2048, 32, 2176))
WIDTH_S = (40, 200)
# sigma sqrt(H) per shape of the sweep; lowered from 1.57 where the f16 emulation left BAR / 3 (test_shape_sweep_emulation_noise asserts every entry)
WIDTH_SCALE = {}


@lru_cache(maxsize=None)
def width_model(H, heads, FF):
    return sharp_weights(H, 1, heads, FF, seed=23, sigma_sqrt_h=WIDTH_SCALE.get((H, heads, FF), SIGMA_SQRT_H))


@lru_cache(maxsize=None)
def width_case(S):
    """B = 3, ragged: row 0 full, row 1 right-padded, row 2 left-padded"""
    rng = np.random.default_rng(9000 + S)
    ids = np.zeros((3, S), np.int64); mask = np.zeros((3, S), np.int64)
    n1, n2 = int(rng.integers(S // 2, S)), int(rng.integers(S // 2, S))
    mask[0] = 1; mask[1, :n1] = 1; mask[2, S - n2:] = 1
    ids[mask != 0] = rng.integers(5, VOCAB, int(mask.sum()))
    return ids, mask


def _round_f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _round_bf16(x):
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)       # round to nearest even (finite inputs)
    return u.view(np.float32).astype(np.float64)


_ROUND = {None: lambda x: x, "f16": _round_f16, "bf16": _round_bf16}


def forward64(w, ids, mask, heads, mutant=None, arg=None, operands=None, token_type_ids=None, residual16=False, eps=1e-12):
    """oracle.encoder_np.bert_forward in fp64, last_hidden_state [B,S,H] of every column, with hooks.

    mutant (each changes the named step and nothing else): "drop_key" (arg = attended index j, one int or one per sequence: that key masked in every layer),
    "scale_other_dh" (scores / sqrt(96 - d_h): the other head width's scale), "scale_ln2" (scores x ln 2: exp2 without the log2(e) fold), "heads_swapped"
    (the context of head h written where head h ^ 1 belongs), "no_bv" (the value bias, which the library folds into the output bias, dropped), "pos_rank"
    (position = rank among the attended tokens instead of the column), "holes_ignored" (every column between the first and the last attended one is a key),
    "type_ignored" (token types all 0), "cls_first_attended" (the row of column 0 = the row of the first attended column).

    operands "f16" / "bf16": every MFMA operand the header of encoder.hip lists (weights, xb, q, k, v, P, ctx, h) rounded to that type, accumulation in fp64;
    residual16 = the residual stream between LayerNorms rounded as well (a handle without the low half; the final LayerNorm always keeps it).  This is the
    reference's own estimate of what 16-bit operands cost on these weights, not a model of the kernels."""
    assert mutant is None or mutant in MUTANTS, mutant
    r = _ROUND[operands]
    W = {k: np.asarray(v, np.float64) for k, v in w.items() if "position_ids" not in k}
    ids = np.asarray(ids); mask = np.asarray(mask)
    B, S = ids.shape
    H = W["embeddings.word_embeddings.weight"].shape[1]
    dh = H // heads
    keep = mask != 0
    tt = np.zeros_like(ids) if token_type_ids is None or mutant == "type_ignored" else np.asarray(token_type_ids)
    pos = np.broadcast_to(np.arange(S), (B, S))
    if mutant == "pos_rank":
        pos = np.maximum(np.cumsum(keep, axis=1) - 1, 0)
    keys = keep.copy()
    if mutant == "holes_ignored":
        first = keep.argmax(1); last = S - 1 - keep[:, ::-1].argmax(1)
        keys = (np.arange(S)[None] >= first[:, None]) & (np.arange(S)[None] <= last[:, None])
    if mutant == "drop_key":
        j = np.broadcast_to(np.asarray(arg), (B,))
        for b in range(B):
            keys[b, np.flatnonzero(keep[b])[j[b]]] = False
    scale = 1.0 / math.sqrt(dh)
    if mutant == "scale_other_dh":
        scale = 1.0 / math.sqrt(96 - dh)
    if mutant == "scale_ln2":
        scale *= math.log(2.0)

    x = W["embeddings.word_embeddings.weight"][ids] + W["embeddings.position_embeddings.weight"][pos] + W["embeddings.token_type_embeddings.weight"][tt]
    x = E.layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    L = 0
    while f"encoder.layer.{L}.attention.self.query.weight" in W:
        L += 1
    for l in range(L):
        p = f"encoder.layer.{l}."
        if residual16:
            x = r(x)

        def lin(t, name, bias=True):
            y = t @ r(W[p + name + ".weight"]).T
            return y + W[p + name + ".bias"] if bias else y

        def split(t):
            return r(t).reshape(B, S, heads, dh).transpose(0, 2, 1, 3)

        xo = r(x)
        q, k, v = split(lin(xo, "attention.self.query")), split(lin(xo, "attention.self.key")), split(lin(xo, "attention.self.value", mutant != "no_bv"))
        s = (q @ k.transpose(0, 1, 3, 2)) * scale
        s = np.where(keys[:, None, None, :], s, -np.inf)
        s = s - s.max(axis=-1, keepdims=True)
        e = np.exp(s)
        pr = r(e / e.sum(axis=-1, keepdims=True))
        ctx = r(pr @ v)
        if mutant == "heads_swapped":
            ctx = ctx[:, np.arange(heads) ^ 1]
        ctx = ctx.transpose(0, 2, 1, 3).reshape(B, S, H)
        x = E.layer_norm(lin(ctx, "attention.output.dense") + x, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        if residual16:
            x = r(x)
        h = r(E.gelu_erf(lin(r(x), "intermediate.dense")))
        x = E.layer_norm(lin(h, "output.dense") + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
    if mutant == "cls_first_attended":
        x = x.copy()
        x[:, 0] = x[np.arange(B), keep.argmax(1)]
    return x


def row_distance(a, b, mask):
    """[B,S]: max over the features of |a - b| on the attended rows, NaN elsewhere"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(-1)
    return np.where(np.asarray(mask) != 0, d, np.nan)


def seq_distance(a, b, mask, cls=False):
    """[B]: max |a - b| over the attended rows of each sequence; with `cls` the row of column 0 counts too (CLS pooling reads it whether attended or not)"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(-1)
    keep = np.asarray(mask) != 0
    if cls:
        keep = keep.copy(); keep[:, 0] = True
    return np.where(keep, d, 0.0).max(1)


def affected(mutant, mask, token_type_ids=None):
    """[B] bool: the sequences a mutant can reach.  pos_rank: an attended token whose column is not its rank (left padding, holes); holes_ignored: a masked
    column between attended ones; type_ignored: an attended token of a non-zero type; cls_first_attended: column 0 masked; the others: every sequence"""
    keep = np.asarray(mask) != 0
    B, S = keep.shape
    rank = np.cumsum(keep, axis=1) - 1
    if mutant == "pos_rank":
        return (keep & (rank != np.arange(S)[None])).any(1)
    if mutant == "holes_ignored":
        first = keep.argmax(1); last = S - 1 - keep[:, ::-1].argmax(1)
        return keep.sum(1) != last - first + 1
    if mutant == "type_ignored":
        return np.zeros(B, bool) if token_type_ids is None else (keep & (np.asarray(token_type_ids) != 0)).any(1)
    if mutant == "cls_first_attended":
        return ~keep[:, 0]
    return np.ones(B, bool)


def pooled64(lh, mask, pool):
    """masked mean (pool 0) / [:, 0] (pool 1) -> L2 normalise, fp64: the encoders' pooling on a last_hidden_state"""
    mk = np.asarray(mask) != 0
    v = (lh * mk[..., None]).sum(1) / mk.sum(1)[:, None] if pool == 0 else lh[:, 0]
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def emulation_error(w, ids, mask, heads, ref, operands, lo, token_type_ids=None):
    """worst |emulated - fp64| on the attended rows for one precision mode"""
    emu = forward64(w, ids, mask, heads, operands=operands, residual16=not lo, token_type_ids=token_type_ids)
    return float(np.nanmax(row_distance(emu, ref, mask)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# references and preconditions of the cases above, computed once per process and shared by every test that needs them (callers must not write into them)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def planted_ref(dh, S, layout):
    ids, mask, _, _ = planted_case(S, layout)
    return forward64(planted_model(dh), ids, mask, DH[dh])


@lru_cache(maxsize=None)
def planted_dropped(dh, S, layout):
    """the reference with each sequence's planted key masked in every layer"""
    ids, mask, js, _ = planted_case(S, layout)
    return forward64(planted_model(dh), ids, mask, DH[dh], "drop_key", js)


@lru_cache(maxsize=None)
def planted_teeth(dh, S, layout):
    """the weakest attended row's distance between the reference and the reference without the planted key"""
    return float(np.nanmin(row_distance(planted_ref(dh, S, layout), planted_dropped(dh, S, layout), planted_case(S, layout)[1])))


@lru_cache(maxsize=None)
def planted_noise(dh, S, layout, mode):
    ids, mask, _, _ = planted_case(S, layout)
    return emulation_error(planted_model(dh), ids, mask, DH[dh], planted_ref(dh, S, layout), mode[0], mode[1])


@lru_cache(maxsize=None)
def generic_ref(S, layout):
    ids, mask, tt = generic_case(S, layout)
    return forward64(generic_model(), ids, mask, 2, token_type_ids=tt)


@lru_cache(maxsize=None)
def generic_teeth(S, layout):
    """{mutant: [B] distance of each sequence from the reference} for every whole-model mutant"""
    ids, mask, tt = generic_case(S, layout)
    ref = generic_ref(S, layout)
    return {m: seq_distance(forward64(generic_model(), ids, mask, 2, m, token_type_ids=tt), ref, mask, cls=m == "cls_first_attended") for m in MUTANTS[1:]}


def generic_weakest(S, layout):
    ids, mask, tt = generic_case(S, layout)
    return min(float(d[affected(m, mask, tt)].min()) for m, d in generic_teeth(S, layout).items() if affected(m, mask, tt).any())


@lru_cache(maxsize=None)
def generic_noise(S, layout, mode):
    ids, mask, tt = generic_case(S, layout)
    return emulation_error(generic_model(), ids, mask, 2, generic_ref(S, layout), mode[0], mode[1], tt)


# The other precision modes (section "Other precision modes" of the GPU tests): per case, the weakest precondition distance of its inputs and, per mode of
# MODES[1:] in that order, the bar = 3 x the worst error of the matching emulation on the same inputs (operands= that type; without the low half the residual
# stream rounded too).  Recorded here, rounded down to two digits, so that the GPU tests need not run twelve emulations per case;
# test_encoder_teeth_host.py::test_recorded_bars_of_the_other_modes recomputes every entry and asserts it.
#   (section, d_h, S, layout): (weakest precondition, bar f16 without lo, bar bf16 + lo, bar bf16 without lo)
MODE_BARS = {
    ("A", 64, 128, "R"): (0.73, 0.01, 0.069, 0.076),
    ("A", 64, 128, "L"): (0.77, 0.01, 0.067, 0.07),
    ("A", 64, 128, "H"): (0.67, 0.0099, 0.067, 0.071),
    ("A", 64, 300, "R"): (0.67, 0.01, 0.068, 0.077),
    ("A", 64, 300, "L"): (0.55, 0.01, 0.073, 0.069),
    ("A", 64, 300, "H"): (0.63, 0.01, 0.07, 0.069),
    ("A", 32, 128, "R"): (0.75, 0.01, 0.066, 0.068),
    ("A", 32, 128, "L"): (0.7, 0.0099, 0.067, 0.069),
    ("A", 32, 128, "H"): (0.79, 0.0094, 0.065, 0.072),
    ("A", 32, 300, "R"): (0.63, 0.0099, 0.072, 0.076),
    ("A", 32, 300, "L"): (0.61, 0.01, 0.072, 0.076),
    ("A", 32, 300, "H"): (0.56, 0.01, 0.071, 0.068),
    ("B", 64, 33, "R"): (0.39, 0.011, 0.083, 0.081),
    ("B", 64, 65, "L"): (0.44, 0.011, 0.088, 0.094),
    ("B", 64, 129, "H"): (0.44, 0.0098, 0.071, 0.079),
    ("B", 64, 200, "R"): (0.41, 0.0095, 0.074, 0.081),
}
