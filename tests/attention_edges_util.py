"""Shared pieces of the attention edge tests (tests/test_attention_edges_host.py, tests/test_gpu_attention_edges.py): the sequence lengths that sit on the
boundaries of k_attn_lds, k_attn_dma and k_pos_scores, derived from the kernels' geometry; the geometry restated in Python (which steps a q-tile visits, where
a q-group's ring ends) so that the host test can say which boundary a length pins; batches that hold a whole list of lengths in one forward; and the
references with one CLASS of keys hidden from every other query (the precondition of the parity tests: the keys at the edges decide rows).

No GPU and no library call here: everything is numpy, HF and the per-family utils (decoder_util, deberta_util, modernbert_util, t5_util)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deberta_util as DB  # noqa: E402
import decoder_util as DC  # noqa: E402

# ---------------------------------------------------------------------------------------------------------
# the kernels' geometry (kirag_amd/csrc/encoder_attn.hpp, encoder_pos.hpp)
# ---------------------------------------------------------------------------------------------------------
Q_TILE = 32          # queries of a wave's tile
KEY_STEP = 64        # keys of one step of the online softmax = one chunk of k_attn_dma's ring
KCHUNK = 128         # keys k_attn_lds stages at a time
Q_GROUP = 256        # queries of one k_attn_dma block: ADMA_QT = 8 tiles, two per wave (w and w + 4)
POS_ROWS = 128       # packed rows of one k_pos_scores block
RING = 3             # stages of k_attn_dma's ring
POS_CHUNK = 64       # buckets k_pos_scores stages at a time
WINDOW = 64          # half-window of the ModernBert handles of these tests (local_attention 128)
LDS_MAX = 4 * Q_TILE  # widest batch the register-staged kernel serves by default; a wider one runs k_attn_dma (a DeBERTa handle: k_attn_lds at every width)

DECODER_KINDS = ("qwen2-32", "llama-64")             # 4 heads of 32 over 2 KV heads, 2 heads of 64 over 1
DEBERTA_SHAPES = ((256, 512), (32, 128))             # (position_buckets, max_relative_positions)
DEBERTA_HEADS = (2, 4)

DECODER_LONG_S = 4 * Q_GROUP
DECODER_LONG = [
    2 * KEY_STEP + Q_TILE,           # 160: the last chunk holds exactly 32 keys (MODE 2), one q-group
    3 * KEY_STEP,                    # 192: no partial chunk, one q-group
    3 * KEY_STEP + 1,                # 193: a last chunk of one key
    Q_GROUP,                         # 256: one q-group, full: every wave has two tiles, none clipped
    Q_GROUP + 1,                     # 257: a second q-group of ONE query whose last chunk holds one key
    Q_GROUP + Q_TILE,                # 288: a second q-group of one tile, last chunk of exactly 32 keys
    Q_GROUP + Q_TILE + 1,            # 289: ... of two tiles, the second of one query
    Q_GROUP + KEY_STEP,              # 320: a second q-group, no partial chunk
    Q_GROUP + KCHUNK,                # 384: q-group 1 with one tile in every wave, none with two
    Q_GROUP + KCHUNK + 1,            # 385: the first length at which a wave of q-group 1 has two tiles
    2 * Q_GROUP - 1,                 # 511: two q-groups, the last query missing
    2 * Q_GROUP,                     # 512: two full q-groups
    2 * Q_GROUP + 1,                 # 513: a third q-group
    2 * Q_GROUP + KEY_STEP,          # 576: a third q-group of two tiles, no partial chunk
    2 * Q_GROUP + KCHUNK,            # 640: a third q-group of four tiles
    4 * Q_GROUP - 24,                # 1000: four q-groups, the ring wrapped several times with a clipped nchunks, a partial last chunk of 40 keys
    4 * Q_GROUP,                     # 1024: four full q-groups, no partial chunk
]

DEBERTA_LONG_S = 512                 # the handles' max_position_embeddings
DEBERTA_LONG = [
    KCHUNK + 1,                      # 129: a second kchunk of one key; T on the far side of a k_pos_scores block
    KCHUNK + Q_TILE,                 # 160: a second kchunk of exactly 32 keys (MODE 2)
    KCHUNK + KEY_STEP,               # 192: a second kchunk of one full step
    KCHUNK + KEY_STEP + 1,           # 193: ... and a step of one key
    KCHUNK + KEY_STEP + Q_TILE,      # 224: ... and a step of 32 keys
    2 * KCHUNK,                      # 256: two whole kchunks (remainder 0)
    2 * KCHUNK + 1,                  # 257: a third kchunk of one key
    2 * KCHUNK + Q_TILE,             # 288: a third kchunk of 32 keys
    2 * KCHUNK + KEY_STEP,           # 320: a third kchunk of one full step
    3 * KCHUNK,                      # 384: three whole kchunks
    4 * KCHUNK - 1,                  # 511: the last key of the fourth kchunk missing
    4 * KCHUNK,                      # 512: four whole kchunks, the widest column difference the table serves
]

# short batches: width S -> lengths.  The width decides the q-tile count and with it HPB (4 / 2 / 1 heads per block) of k_attn_lds
SHORT = {
    Q_TILE: [1, 2, Q_TILE - 1, Q_TILE],                                                              # one q-tile, HPB 4: a single key, MODE 1, MODE 2
    2 * Q_TILE: [Q_TILE + 1, 2 * Q_TILE - 1, 2 * Q_TILE],                                            # two q-tiles, HPB 2: MODE 3 with 1 and 31 keys in the second tile, a full step
    4 * Q_TILE: [2 * Q_TILE + 1, 3 * Q_TILE - 1, 3 * Q_TILE, 3 * Q_TILE + 1, 4 * Q_TILE - 1, 4 * Q_TILE],  # three / four q-tiles, HPB 1: a second step of 1, 31, 32, 33, 63, 64 keys
}

# the decoder entries the bit-identity tests run one by one (part of the list: one forward per length)
DECODER_IDENTITY = [n for n in DECODER_LONG if n <= 2 * Q_GROUP + 1] + [4 * Q_GROUP - 24]
CAUSAL_COLUMNS = (Q_GROUP - 1, Q_GROUP, Q_GROUP + 1, 2 * Q_GROUP - 1, 2 * Q_GROUP, 3 * Q_GROUP - 1, 4 * Q_GROUP - 1)

# packed key indices hidden as a class: the last / first key of a 64-key step, of a 32-key tile
KEY_CLASSES = {"63 mod 64": (KEY_STEP - 1, KEY_STEP), "0 mod 64": (0, KEY_STEP), "31 mod 64": (Q_TILE - 1, KEY_STEP), "32 mod 64": (Q_TILE, KEY_STEP)}
# ... DeBERTa also: of a kchunk, and the last key of every sequence (the clamp of the gathered bias tile)
DEBERTA_KEY_CLASSES = dict(KEY_CLASSES, **{"127 mod 128": (KCHUNK - 1, KCHUNK), "0 mod 128": (0, KCHUNK), "last key": None})


def round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------
# the geometry restated: what a sequence of n keys (nq == nk) makes the kernels do
# ---------------------------------------------------------------------------------------------------------
def band(q0, q1, nk, wl, wr):
    """attn_band without the query-only row: packed keys [lo, hi] of queries [q0, q1] (hi < lo: none)"""
    return max(q0 - wl, 0), (min(q1, nk - 1) + wr if q0 < nk else -1)


def visits(b, kb):
    return kb <= b[1] and kb + KEY_STEP - 1 >= b[0]


def dma_groups(n, wl, wr):
    """per q-group of k_attn_dma under a window (causal: wl = max_pos, wr = 0): dict(c_lo, nchunks, nfull, chunks = ceil(n / 64), two = some wave has two
    tiles, tiles = active q-tiles)"""
    out = []
    chunks = (n + KEY_STEP - 1) // KEY_STEP
    for g in range((n + Q_GROUP - 1) // Q_GROUP):
        lo, hi = band(g * Q_GROUP, g * Q_GROUP + Q_GROUP - 1, n, wl, wr)
        nchunks = min(chunks, hi // KEY_STEP + 1)
        out.append(dict(c_lo=lo // KEY_STEP, nchunks=nchunks, nfull=min(n // KEY_STEP, nchunks), chunks=chunks,
                        two=g * Q_GROUP + 4 * Q_TILE < n, tiles=min((n - g * Q_GROUP + Q_TILE - 1) // Q_TILE, Q_GROUP // Q_TILE)))
    return out


def decoder_classes(n, max_pos=DECODER_LONG_S):
    """the boundary classes of k_attn_dma's causal mode a sequence of n tokens sits on"""
    g = dma_groups(n, max_pos, 0)
    c = set()
    if n % KEY_STEP == Q_TILE:
        c.add("last chunk of exactly 32 keys")
    if n % KEY_STEP == 0:
        c.add("no partial chunk")
    if n % KEY_STEP == 1 and len(g) >= 2 and n - (len(g) - 1) * Q_GROUP == 1:
        c.add("a q-group of one query whose last chunk holds one key")
    if len(g) >= 2 and n % KEY_STEP == Q_TILE:
        c.add("a partial last chunk of 32 keys in a q-group >= 1")
    if len(g) >= 2 and g[1]["two"]:
        c.add("two tiles per wave in a q-group >= 1")
    if n == Q_GROUP + 4 * Q_TILE + 1:
        c.add("first length with two tiles per wave in q-group 1")
    if len(g) >= 3:
        c.add("three q-groups")
    if len(g) >= 4:
        c.add("four q-groups")
    if any(x["nchunks"] < x["chunks"] and x["nchunks"] > RING for x in g):
        c.add("the ring wraps with a clipped nchunks")
    if any(x["nchunks"] < x["chunks"] and x["nfull"] == x["nchunks"] for x in g):
        c.add("the clipped last chunk is full while the sequence goes on")
    if any(x["nchunks"] == x["chunks"] and x["nfull"] < x["nchunks"] and x["nchunks"] > RING for x in g[1:]):
        c.add("a partial last chunk behind a wrapped ring in a q-group >= 1")
    return c


DECODER_CLASSES = ("last chunk of exactly 32 keys", "no partial chunk", "a q-group of one query whose last chunk holds one key",
                   "a partial last chunk of 32 keys in a q-group >= 1", "two tiles per wave in a q-group >= 1", "first length with two tiles per wave in q-group 1",
                   "three q-groups", "four q-groups", "the ring wraps with a clipped nchunks", "the clipped last chunk is full while the sequence goes on",
                   "a partial last chunk behind a wrapped ring in a q-group >= 1")


def lds_classes(n):
    """the boundary classes of k_attn_lds's multi-chunk loop a sequence of n keys sits on (batches wider than KCHUNK: kchunk = 128)"""
    c = set()
    if n > KCHUNK:
        r = n % KCHUNK
        c.add({0: "kchunk remainder 0", 1: "kchunk remainder 1", Q_TILE: "kchunk remainder 32", KEY_STEP: "kchunk remainder 64"}.get(r, "other"))
        if r > KEY_STEP and r % KEY_STEP == 1:
            c.add("a full step and a step of one key in the last kchunk")
        if r > KEY_STEP and r % KEY_STEP == Q_TILE:
            c.add("a full step and a step of 32 keys in the last kchunk")
        if r == KCHUNK - 1:
            c.add("kchunk remainder 127")
    c.discard("other")
    return c


def window_classes(n, w=WINDOW):
    """the boundary classes of k_attn_dma under a symmetric window a sequence of n tokens sits on"""
    c = set()
    for x in dma_groups(n, w, w):
        last = {0: "no partial chunk", 1: "a last chunk of one key", Q_TILE: "a last chunk of 32 keys"}.get(n % KEY_STEP)
        if x["c_lo"] > 0:
            c.add("the ring starts at c_lo > 0")
            if last and x["nchunks"] == x["chunks"]:
                c.add("c_lo > 0, " + last)
        if x["nchunks"] < x["chunks"]:
            c.add("nchunks clipped by the window")
        if x["c_lo"] > 0 and x["nchunks"] - x["c_lo"] > RING:
            c.add("a ring from c_lo > 0 that wraps")
    return c


WINDOW_CLASSES = ("the ring starts at c_lo > 0", "c_lo > 0, no partial chunk", "c_lo > 0, a last chunk of one key", "c_lo > 0, a last chunk of 32 keys",
                  "nchunks clipped by the window", "a ring from c_lo > 0 that wraps")

LDS_CLASSES = ("kchunk remainder 0", "kchunk remainder 1", "kchunk remainder 32", "kchunk remainder 64", "a full step and a step of one key in the last kchunk",
               "a full step and a step of 32 keys in the last kchunk", "kchunk remainder 127")


def hpb(S):
    """heads per block of k_attn_lds for a batch of width S (mean pooling: no query-only row)"""
    nqt = (S + Q_TILE - 1) // Q_TILE
    return 1 if nqt >= 3 else 2 if nqt == 2 else 4


def step_mode(nvalid):
    """MODE of a step with nvalid keys (attn_scores)"""
    return 0 if nvalid == KEY_STEP else 2 if nvalid == Q_TILE else 1 if nvalid < Q_TILE else 3


def last_step_mode(n, chunk=KCHUNK):
    """MODE of the last step k_attn_lds runs on a sequence of n keys staged `chunk` keys at a time"""
    r = (n - 1) % chunk + 1
    return step_mode((r - 1) % KEY_STEP + 1)


def pos_span(S, Bk, M):
    """pos_span of encoder.hip by HF's own bucket rule: (p0, W) of the buckets a batch of width S can reach"""
    lo, hi = (int(x) for x in DB.hf_buckets(np.array([-(S - 1), S - 1]), Bk, M))
    p0 = lo & ~31
    return p0, round_up(hi + 1 - p0, 32)


def widths_with_span(W, Bk, M, max_pos=DEBERTA_LONG_S):
    """every batch width whose pos_span is W buckets wide"""
    S = np.arange(1, max_pos + 1)
    lo, hi = DB.hf_buckets(-(S - 1), Bk, M), DB.hf_buckets(S - 1, Bk, M)
    return [int(s) for s in S[(hi + 1 - (lo & ~31) + 31) // 32 * 32 == W]]


def deberta_extras(Bk, M):
    """(B, S) of the extra full-length DeBERTa batches: B = 3 at S = 1 (W = 32: k_pos_scores leaves its first chunk at the pt break), one sequence of T = 127,
    128 and 129 packed rows (both sides of a k_pos_scores block) and, where the table has one, the first width whose span is W = 96 (ends in a half chunk)"""
    out = [(3, 1)] + [(1, POS_ROWS + d) for d in (-1, 0, 1)]
    w96 = widths_with_span(96, Bk, M)
    if w96:
        out.append((1, w96[0]))
    return out


# ---------------------------------------------------------------------------------------------------------
# batches that hold a list of lengths
# ---------------------------------------------------------------------------------------------------------
def ragged(lens, S, side, seed, lo, hi, first=None, last=None):
    """(ids, mask) [len(lens), S] int64: row r holds lens[r] ids uniform in [lo, hi) (`first` / `last`: the id of its first / last token), padded with id 0 on
    the other `side` ("right" / "left")"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = np.zeros((len(lens), S), np.int64); mask = np.zeros((len(lens), S), np.int64)
    for r, n in enumerate(lens):
        n = int(n)
        row = rng.integers(lo, hi, n)
        if first is not None:
            row[0] = first
        if last is not None and n > 1:
            row[-1] = last
        at = slice(0, n) if side == "right" else slice(S - n, S)
        ids[r, at], mask[r, at] = row, 1
    return ids, mask


def shifted(ids, mask, S=None):
    """the same sequences (no holes) left-padded in a batch of width S"""
    S = ids.shape[1] if S is None else S
    out = np.zeros((len(ids), S), np.int64); om = np.zeros((len(ids), S), np.int64)
    for r in range(len(ids)):
        n = int(mask[r].sum())
        out[r, S - n:], om[r, S - n:] = ids[r, :n], 1
    return out, om


def decoder_batch(lens, S, layout, seed, holes=0):
    """decoder_util.tokens on a list of lengths: R / L padded, `holes` attended columns of every row (never its first or last) masked out again"""
    return DC.tokens(len(lens), S, layout, seed, lens=list(lens), holes=holes)


def deberta_batch(lens, S, side, seed, holes=False):
    """deberta_util.tokens' rows (CLS first, SEP last, ids in [3, VOCAB)) on a list of lengths, with its hole rule: a row of more than 4 tokens loses
    1 + n / 5 interior columns to the mask, column 0 of a right-padded row stays attended"""
    ids, mask = ragged(lens, S, side, 7000 + seed, 3, DB.VOCAB, first=DB.CLS_ID, last=DB.SEP_ID)
    if holes:
        rng = np.random.Generator(np.random.PCG64(9000 + seed))
        for r, n in enumerate(lens):
            n = int(n)
            if n > 4:
                start = 0 if side == "right" else S - n
                cut = start + 1 + rng.choice(n - 2, size=min(1 + n // 5, n - 2), replace=False)
                mask[r, cut] = 0
    return ids, mask


def with_holes(ids, mask, holes, seed):
    """the batch with `holes` attended columns of every row (never its first or last attended one) masked out again, their ids set to 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids, mask = ids.copy(), mask.copy()
    for r in range(len(ids)):
        cols = np.flatnonzero(mask[r])
        if len(cols) > 2:
            drop = rng.choice(cols[1:-1], size=min(holes, len(cols) - 2), replace=False)
            mask[r, drop] = 0; ids[r, drop] = 0
    return ids, mask


def modernbert_model(heads):
    """(config, weights) of the tiny ModernBert of these tests: H 128, layers global / local / local, local_attention 128 (half-window 64), weights under
    which the window decides rows (modernbert_util.teeth_weights)"""
    import modernbert_util as MB
    return MB.cfg(128, 3, heads, 256, 1000, 8192, types=[MB.FULL, MB.SLIDING, MB.SLIDING], local_attention=2 * WINDOW), MB.teeth_weights(128, 3, 256, 1000)


def modernbert_batch(lens, S, side, seed=53):
    """rows of ids in [5, 1000) behind id 2"""
    return ragged(lens, S, side, seed, 5, 1000, first=2)


def one_changed(ids, c, vocab_lo=3, vocab_hi=DC.VOCAB):
    """the batch with the token of row 0, column c replaced by another id"""
    out = ids.copy()
    out[0, c] = vocab_lo + (ids[0, c] - vocab_lo + 17) % (vocab_hi - vocab_lo)
    return out


# ---------------------------------------------------------------------------------------------------------
# references with one class of keys hidden from every other query
# ---------------------------------------------------------------------------------------------------------
def hidden_keys(mask, cls):
    """[B, S] bool: the attended columns whose PACKED index (rank among the row's attended columns) is in the class: (residue, modulus), or None = the last
    attended column of every row"""
    mask = np.asarray(mask) != 0
    rank = np.cumsum(mask, axis=1) - 1
    if cls is None:
        return mask & (rank == mask.sum(1, keepdims=True) - 1)
    return mask & (rank % cls[1] == cls[0])


def visible(mask, rule, hide=None):
    """[B, S, S] bool: query column q sees key column k: k attended, RULES[rule] admits it, and k is not hidden — a key stays visible to itself, so no attended
    row becomes empty"""
    mask = np.asarray(mask) != 0
    S = mask.shape[1]
    q, k = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    ok = DC.RULES[rule](q, k)[None] & mask[:, None, :]
    if hide is not None:
        ok = ok & (~hide[:, None, :] | (q == k)[None])
    return ok


@torch.no_grad()
def decoder_hidden(m, ids, mask, hide=None, chunk=6):
    """HF last_hidden_state [B, S, H] fp32 under a hand-made 4-D additive causal mask (decoder_util.mask4d's values), with the keys `hide` [B, S] hidden from
    every other query"""
    outs = []
    dev = next(m.parameters()).device
    for i in range(0, len(ids), chunk):
        ok = visible(mask[i:i + chunk], "causal", None if hide is None else hide[i:i + chunk])
        add = torch.from_numpy(np.where(ok, 0.0, np.finfo(np.float32).min).astype(np.float32))[:, None].to(dev)
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev)
        outs.append(m(input_ids=a, attention_mask=add).last_hidden_state.float().cpu().numpy())
    return np.concatenate(outs)


@torch.no_grad()
def deberta_hidden(m, ids, mask, hide=None):
    """DebertaV2Model's last_hidden_state [B, S, H] as float64: its embeddings under the 2-D mask, its encoder under a 3-D [B, S, S] mask — the product of the
    2-D mask with itself (what the model builds from a 2-D mask), less the keys `hide` for every other query"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    att = np.asarray(mask) != 0
    ok = visible(mask, "none", hide) & att[:, :, None]
    emb = m.embeddings(input_ids=t(ids), mask=t(mask))
    return m.encoder(emb, t(ok.astype(np.int64)), output_hidden_states=True, return_dict=True).hidden_states[-1].double().numpy()


def class_distances(ref, hidden_fn, mask, classes, rows=None):
    """name -> max |ref - reference with the class hidden| over the attended rows (`rows`: [B, S] bool, a further restriction)"""
    keep = np.asarray(mask) != 0
    if rows is not None:
        keep = keep & rows
    out = {}
    for name, cls in classes.items():
        hide = hidden_keys(mask, cls)
        out[name] = float(np.abs(np.asarray(ref, np.float64) - hidden_fn(hide))[keep].max())
    return out
