"""Data and reference of the attention probe (tests/capi/attn_probe.hip, tests/test_attn_probe_host.py, tests/test_gpu_attn_probe.py).  Everything here is
numpy; the lists of lengths and band / visits come from attention_edges_util, whose own imports (torch, the oracle) need the repository root on the path, as
under pytest.

The probe launches k_attn_lds / k_attn_dma (kirag_amd/csrc/encoder_attn.hpp) on q / k / V^T this file builds, so that every key is decisive at any length:

  needles   most keys are dull (k = 0, score 0).  The SPECIAL keys of every 64-key step sit on its edge classes (index 0, 31, 32 and 63 of the step; index 0
            and 127 of a 128-key kchunk of k_attn_lds are index 0 of an even and 63 of an odd step).  A special key carries three one-hot blocks — step mod
            16 | step div 16 | class, 28 dimensions — and a query carries A = 12 on the three positions of its TARGET: score 3 A with the target, at most
            2 A with any other key, so the target holds > 0.9 of the row's mass.  v_j is a +-2 code of j and of the KV head: the output names the key and the
            head that were read.  In every 32-query tile the (query, head) slots are dealt over the 64-key steps the tile visits (the visit rule of attn_band,
            restated below), so hiding any visited step from any tile moves a row of the tile.
  decoys    (window / causal) an INADMISSIBLE key one column outside a query's window — column col_i + wr + 1 ("right", i + 1 under causal) or
            col_i - wl - 1 ("left") — whose score, 64, beats the target's 36.  Two dimensions per side hold a ramp: the r-th decoy key (in packed order)
            carries (r, 1), the query whose decoy it is (64, -64 (r - 1)): score 64 (r' - r + 1) with decoy key r', i.e. 64 with its own, <= 0 with every
            earlier one (the admissible side), more with the later ones (further outside).  The left ramp runs the other way.  Ranks stay <= 254, so every
            value is exact in bf16.  With holes in the columns the decoys are placed by column, not by packed index.
  diffuse   q, k, v random multiples of 1/8: a few dozen keys share a row's mass (this checks the WEIGHTS, which needles do not); a ramp over the steps on
            one dimension (1/2 per step) makes the running maximum keep rising in a third of the rows (the deferred rescale) and fall after the first step in another third.

Every value is exactly representable in f16 and in bf16 (small integers, powers of two, multiples of 1/8 below 32): the inputs carry no rounding, and all the
scores are exact in fp32 too.  K and V of different KV heads differ: KV head g stores dimension d of the code at (d + 5 g) mod d_h, and v names g.

UNITS: the kernels take scores in log2 units — the loader folds log2(e) / sqrt(d_h) into W_q (enc_load_weight), and build_bias_table multiplies the bias table
by log2(e) on the host; the kernels add the table entry as it is — so the reference is a base-2 softmax of q.k + tab[head][width / 2 + col_j - col_i]:
    ctx[i] = sum_j 2^(s_ij - max_i) v_j / sum_j 2^(s_ij - max_i)     over the keys the mode admits, in float64.
The query-only CLS row (nq = nk + 1, packed last, column 0) follows attn_band's rule: under a window it admits the keys of column <= wr."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attention_edges_util import DEBERTA_LONG, DECODER_LONG, KCHUNK, KEY_STEP, Q_GROUP, Q_TILE, SHORT, WINDOW, band, round_up, visits  # noqa: E402,F401

MODES = ("plain", "bias", "window", "causal")
MAX_POS = 10240                       # the probe's "handle": widest column + 1; causal = window (MAX_POS, 0), as causal_args sets it
BIAS_HALF = MAX_POS + 64              # build_bias_table: width = 2 (max_pos + 64)
A = 12.0                              # weight of one matching block, in log2 units
MAX_TARGETS = 6                       # targets of one (query, head) slot where a tile has fewer slots than visited steps
DECOY = 64.0                          # score of a decoy with the query it belongs to
MAX_DECOYS = 255                      # per sequence and side: ranks 0 .. 254 and 64 * 255 are exact in bf16
VMAX = 2.0                            # max |v| of both data sets
SPECIAL = (0, 31, 32, 63)             # special key positions inside a 64-key step
LONG = [2049, 2080, 4097, 8191, 8192]  # 2080: last chunk of exactly 32 keys in q-group 8; 4097: a q-group of one query
# (heads, kv_heads): groups 1, 2, 2, 3, 7, 16 and (d_h 64 only) 4 with 32 heads; a partial last head block under HPB 4 (6, 14), head blocks that straddle
# two KV groups (6 / 2 and 14 / 2 under HPB 2 and 4)
SHAPES = ((4, 4), (4, 2), (2, 1), (6, 2), (14, 2), (16, 1))
SHAPE_64_ONLY = (32, 8)
FILLS = (1024.0, -512.0)              # what the slack, the alignment rows and the rows between sequences hold (large, finite; two values for the leak test)


def mode_window(mode, wl=WINDOW, wr=WINDOW):
    """(wl, wr) the kernels get, None without a window"""
    return None if mode in ("plain", "bias") else (MAX_POS, 0) if mode == "causal" else (wl, wr)


# ---------------------------------------------------------------------------------------------------------
# one sequence
# ---------------------------------------------------------------------------------------------------------
def seq_columns(n, kind):
    """(col [nq] int32, nk) of a sequence of n attended tokens.  kind: "right" columns 0 .. n - 1; "left": MAX_POS - n .. MAX_POS - 1 (left padding in the widest
    batch); "holes": increasing columns with gaps (about one column in five masked out); "cls" / "cls-holes": column 0 masked, so the keys start at
    column 1 and a query-only row of column 0 is packed last (nq = nk + 1)"""
    if kind == "right":
        return np.arange(n, dtype=np.int32), n
    if kind == "left":
        return np.arange(MAX_POS - n, MAX_POS, dtype=np.int32), n
    rng = np.random.Generator(np.random.PCG64(4000 + n))
    if kind in ("holes", "cls-holes"):
        gaps = 1 + (rng.random(n) < 0.2).astype(np.int64)
        col = np.cumsum(gaps) - gaps[0] + (1 if kind == "cls-holes" else 0)
    elif kind == "cls":
        col = np.arange(1, n + 1)
    else:
        raise ValueError(kind)
    assert col.max() < MAX_POS
    if kind.startswith("cls"):
        return np.concatenate([col, [0]]).astype(np.int32), n
    return col.astype(np.int32), n


def kv_perm(g, dh):
    """where KV head g stores code dimension d"""
    return (np.arange(dh) + 5 * g) % dh


def admits(colq, colk, win):
    """[len(colq), len(colk)] bool"""
    if win is None:
        return np.ones((len(colq), len(colk)), bool)
    d = colk[None, :].astype(np.int64) - colq[:, None].astype(np.int64)
    return (d >= -win[0]) & (d <= win[1])


def tile_steps(t, nk, nq, win):
    """the 64-key steps (first keys kb) the tile of queries [32 t, 32 t + 31] visits: attn_band's rule, query-only row included"""
    allsteps = np.arange(0, nk, KEY_STEP)
    if win is None:
        return allsteps
    q0, q1 = Q_TILE * t, Q_TILE * t + Q_TILE - 1
    b = band(q0, q1, nk, win[0], win[1])
    xhi = win[1] if (nq > nk and q1 >= nk) else -1
    return np.array([kb for kb in allsteps if visits(b, kb) or kb <= xhi], dtype=np.int64)


def value_codes(nk, kv_heads, dh):
    """v [nk, kv_heads, dh] of +-2: bits of j, of the KV head, of a hash of both"""
    j = np.arange(nk, dtype=np.int64)[:, None, None]
    g = np.arange(kv_heads, dtype=np.int64)[None, :, None]
    d = np.arange(dh, dtype=np.int64)[None, None, :]
    hsh = (j * 2654435761 + g * 40503 + 12345) & 0xFFFFFFFF
    bit = np.where(d < 13, (j >> np.minimum(d, 12)) & 1, np.where(d < 16, (g >> np.clip(d - 13, 0, 2)) & 1, (hsh >> ((d - 16) % 24 + 4)) & 1))
    return np.where(bit != 0, VMAX, -VMAX)


class Seq:
    """q [nq, heads, dh], k / v [nk, kv_heads, dh] float64, col [nq] int32; needles also: target [nq, heads] packed key, decoy_r / decoy_l: lists of (query, key)"""
    pass


@functools.lru_cache(maxsize=None)
def make_seq(n, kind, heads, kv_heads, dh, mode, data, wl=WINDOW, wr=WINDOW):
    s = Seq()
    s.col, s.nk = seq_columns(n, kind)
    s.nq = len(s.col)
    s.heads, s.kv_heads, s.dh, s.mode, s.win = heads, kv_heads, dh, mode, mode_window(mode, wl, wr)
    s.group = heads // kv_heads
    s.decoy_r, s.decoy_l = [], []
    if data == "needles":
        _needles(s)
    elif data == "diffuse":
        _diffuse(s, n)
    else:
        raise ValueError(data)
    for a in (s.q, s.k, s.v, s.col):
        a.setflags(write=False)
    return s


def _needles(s):
    nk, nq, heads, dh, win = s.nk, s.nq, s.heads, s.dh, s.win
    colk = s.col[:nk]
    nsteps = (nk + KEY_STEP - 1) // KEY_STEP
    # special keys: sp[step, c] = packed key or -1
    sp = np.arange(nsteps)[:, None] * KEY_STEP + np.array(SPECIAL)[None, :]
    sp = np.where(sp < nk, sp, -1)
    code = np.zeros((nk, 32))
    for c in range(4):
        keys = sp[:, c][sp[:, c] >= 0]
        st = keys // KEY_STEP
        code[keys, st % 16] = 1.0; code[keys, 16 + st // 16] = 1.0; code[keys, 24 + c] = 1.0
    qcode = np.zeros((nq, heads, 32))
    # decoys first: a query that carries a ramp scores every ADMITTED decoy key of that side <= 0, so it must not target one (barred below)
    bar_rows = {}
    if win is not None:
        idx_of = {int(c): i for i, c in enumerate(colk)}
        cand = {}
        for side in "rl":
            cand[side] = {}
            for i in range(nk):
                c = int(s.col[i]) + win[1] + 1 if side == "r" else int(s.col[i]) - win[0] - 1
                j = idx_of.get(c)
                if j is not None and (i % Q_TILE in (0, 1, Q_TILE - 1) or j % KEY_STEP in (0, 1, 31, 32, 33, 63) or i % 7 == 3):
                    cand[side][i] = j
        # one ramp per query: a key can be the right decoy of one query and a left decoy of another, and the left ramp of a query scores the keys to its right
        # (its own right decoy among them) far below zero
        for i in [i for i in cand["r"] if i in cand["l"]]:
            del cand["l" if (i + i // Q_TILE) % 2 == 0 else "r"][i]
        # a tile keeps only as many decoy queries as it can spare: the other queries' slots alone still cover every step the tile visits
        keep = set()
        for t in range((nq + Q_TILE - 1) // Q_TILE):
            lo_q, hi_q = Q_TILE * t, min(Q_TILE * t + Q_TILE, nq)
            spare = (hi_q - lo_q) - -(-len(tile_steps(t, nk, nq, win)) // heads) - 1
            want = sorted((i for i in range(lo_q, hi_q) if i in cand["r"] or i in cand["l"]), key=lambda i: (i % Q_TILE not in (0, Q_TILE - 1), i))
            keep.update(want[:max(spare, 0)])
        for side, lst, base in (("r", s.decoy_r, 28), ("l", s.decoy_l, 30)):
            pairs = [(i, j) for i, j in sorted(cand[side].items()) if i in keep]
            if len(pairs) > MAX_DECOYS:
                pairs = [pairs[i] for i in np.unique(np.linspace(0, len(pairs) - 1, MAX_DECOYS).astype(int))]
            pairs.sort(key=lambda p: p[1])
            dk = np.array([j for _, j in pairs], np.int64)
            for rnk, (i, j) in enumerate(pairs):
                code[j, base], code[j, base + 1] = float(rnk), 1.0
                qcode[i, :, base:base + 2] = (DECOY, -DECOY * (rnk - 1)) if side == "r" else (-DECOY, DECOY * (rnk + 1))
                bar_rows.setdefault(i, []).append(dk)
            lst.extend(pairs)
    blocks = code[:, :28].copy()                                              # the three one-hot blocks of every key, without the ramps
    target = np.full((nq, heads), -1, np.int64)
    multi = []
    for t in range((nq + Q_TILE - 1) // Q_TILE):
        qs = np.arange(Q_TILE * t, min(Q_TILE * t + Q_TILE, nq))
        kbs = tile_steps(t, nk, nq, win)
        m = len(kbs)
        if m == 0:
            continue
        stp = kbs // KEY_STEP
        spk = sp[stp]                                                         # [m, 4]
        ok = admits(s.col[qs], colk[np.maximum(spk, 0).ravel()], win).reshape(len(qs), m, 4) & (spk >= 0)[None]
        for a, i in enumerate(qs):
            for dk in bar_rows.get(int(i), ()):
                ok[a] &= ~np.isin(spk, dk)
        adm = ok.any(2)                                                       # [queries, m]: the query admits a special key of the step
        nslots = heads * len(qs)
        h0 = t % heads
        last = len(qs) - 1
        own = int(np.searchsorted(stp, min(qs[last], nk - 1) // KEY_STEP))
        if m > nslots:
            # fewer (query, head) slots than visited steps (a partial last tile of a long sequence): a slot takes up to MAX_TARGETS steps of ONE group of 16
            # steps, keys of one class: q carries A on each target's step-mod-16 position, on the group and on the class, so exactly the targets score 3 A
            # (a key of another group or class misses a block) and share the row's mass; hiding one of T <= 6 moves the row by about |v - mean of the others| / T
            grp = stp // 16
            groups = [np.nonzero(grp == g)[0] for g in np.unique(grp)]
            T = next((T for T in range(2, MAX_TARGETS + 1) if sum(-(-len(ix) // T) for ix in groups) <= nslots), None)
            if T is None:
                raise ValueError("tile %d of a sequence of %d keys visits %d steps: %d heads cannot cover them" % (t, nk, m, heads))
            chunks = [ix[a:a + T] for ix in groups for a in range(0, len(ix), T)]
            for ci in range(nslots):
                ch = chunks[ci % len(chunks)]
                j, h = ci % len(qs), (ci // len(qs)) % heads
                cnt = ok[j, ch].sum(0)                                        # per class: the steps of the chunk whose key of that class the query admits
                best = np.nonzero(cnt == cnt.max())[0]
                c = int(best[ci % len(best)])
                ts = ch[ok[j, ch, c]]
                if len(ts) == 0:
                    continue
                qcode[qs[j], h, stp[ts] % 16] = A; qcode[qs[j], h, 16 + grp[ts[0]]] = A; qcode[qs[j], h, 24 + c] = A
                multi.append((int(qs[j]), h))
                target[qs[j], h] = -2
            continue
        u = len(qs) * np.arange(heads)[:, None] + np.arange(len(qs))[None, :]  # [heads, queries]: the slots of the tile
        qi = np.broadcast_to(np.arange(len(qs))[None, :], u.shape)
        if adm.all():
            # every query admits a special key of every visited step: slot u takes step (u + r) mod m.  r puts the slot of the tile's last query, head t mod
            # heads, on the query's own step: it targets its own key (the diagonal of the causal mask) where that key is special
            r = (own - (len(qs) * h0 + last)) % m
            chosen = (u + r) % m
        else:
            # a window's edge steps, holes, the query-only row: deal the slots one by one, each to the least-covered step it has an admissible special key in
            chosen = np.full(u.shape, -1, np.int64)
            cover = [0] * m
            lists = [np.nonzero(adm[a])[0].tolist() for a in range(len(qs))]
            free = sorted((a for a in range(len(qs)) if int(qs[a]) not in bar_rows), key=lambda a: len(lists[a]))      # the most constrained first,
            held = [a for a in range(len(qs)) if int(qs[a]) in bar_rows]                                            # the decoy queries last
            order = [(h0, last)] + [(h, a) for a in free + held for h in range(heads) if (h, a) != (h0, last)]
            for n_, (h, a) in enumerate(order):
                if not lists[a]:
                    continue
                c = own if (n_ == 0 and own in lists[a]) else min(lists[a], key=lambda x: (cover[x], (x - a - h) % m))
                chosen[h, a] = c; cover[c] += 1
        has = chosen >= 0
        ok4 = ok[qi, np.maximum(chosen, 0)] & has[..., None]                  # [heads, queries, 4]
        cnt = np.maximum(ok4.sum(2), 1)
        pick = (u + t) % cnt
        sel = (np.cumsum(ok4, 2) - 1 == pick[..., None]) & ok4
        key = np.where(has, spk[np.maximum(chosen, 0), sel.argmax(2)], -1)
        if qs[last] < nk and chosen[h0, last] == own and (spk[own] == qs[last]).any() and ok[last, own][spk[own] == qs[last]].all():
            key[h0, last] = qs[last]                                          # its own key
        target[qs] = key.T
    hq, hh = np.nonzero(target >= 0)
    qcode[hq, hh, :28] = blocks[target[hq, hh]] * A
    s.target, s.multi = target, multi
    _store(s, qcode, code)
    s.v = value_codes(nk, s.kv_heads, dh)


def _store(s, qcode, kcode):
    """codes [.., 32] -> q [nq, heads, dh] / k [nk, kv_heads, dh] in each KV head's own arrangement of the dimensions"""
    s.q = np.zeros((s.nq, s.heads, s.dh)); s.k = np.zeros((s.nk, s.kv_heads, s.dh))
    w = qcode.shape[-1]
    for g in range(s.kv_heads):
        p = kv_perm(g, s.dh)[:w]
        s.k[:, g, p] = kcode
        for h in range(g * s.group, (g + 1) * s.group):
            s.q[:, h, p] = qcode[:, h]


def _diffuse(s, n):
    nk, nq, heads, dh = s.nk, s.nq, s.heads, s.dh
    rng = np.random.Generator(np.random.PCG64(77000 + 131 * n + 7 * heads + dh + len(s.mode)))
    qa = 16 if dh == 32 else 11                                               # q in [-2, 2] / [-1.375, 1.375]: a score spread of about 3.8 log2 units
    qcode = rng.integers(-qa, qa + 1, (nq, heads, dh)) / 8.0
    kcode = rng.integers(-8, 9, (nk, dh)) / 8.0
    # the ramp: dimension 0 of k rises by 1/2 per step (and starts again every 32 steps); a third of the rows climbs it (the maximum keeps rising, 1 per step: past
    # the rescale threshold every 8 steps), a third descends (the maximum falls after the first step)
    kcode[:, 0] = ((np.arange(nk) // KEY_STEP) % 32) / 2.0
    qcode[:, :, 0] = np.where(np.arange(nq) % 3 == 0, 2.0, np.where(np.arange(nq) % 3 == 1, -2.0, 0.0))[:, None]
    s.target = None
    _store(s, qcode, kcode)
    base = rng.integers(-16, 17, (nk, dh)) / 8.0
    s.v = np.stack([np.roll(base, 3 * g + 1, axis=1) * (1.0 if g % 2 == 0 else -1.0) for g in range(s.kv_heads)], axis=1)


@functools.lru_cache(maxsize=None)
def bias_table(heads):
    """[heads, 2 BIAS_HALF] float32 in log2 units: multiples of 1/8 in [-1/2, 0], every head its own (small next to the needles' margins: the targets of a
    slot with several keep comparable shares; an entry off by one column or head still moves the diffuse set's weights by 9 % and more)"""
    rng = np.random.Generator(np.random.PCG64(991 + heads))
    t = (-rng.integers(0, 5, (heads, 2 * BIAS_HALF)) / 8.0).astype(np.float32)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------
def reference(s, win="own", kv_of=None, hide=None, sens=False):
    """ctx [nq, heads, dh] float64 of sequence s.  win: another (wl, wr) than the sequence's own; kv_of [heads]: another KV head per query head;
    hide(t) -> packed keys hidden from tile t.  sens = True: also returns {(tile, kb): max |ctx - ctx with step kb hidden from the tile|} over the visited steps
    (-1.0: no query of the tile admits any key of the step — attn_band's rule is conservative, e.g. the query-only row's step of columns > wr — so hiding it
    is no change at all)"""
    win = s.win if win == "own" else win
    kv_of = np.arange(s.heads) // s.group if kv_of is None else np.asarray(kv_of)
    nk, nq = s.nk, s.nq
    colk = s.col[:nk]
    tab = bias_table(s.heads).astype(np.float64) if s.mode == "bias" else None
    out = np.zeros((nq, s.heads, s.dh))
    moved = {}
    kh = np.ascontiguousarray(s.k.transpose(1, 0, 2))[kv_of]                  # [heads, nk, dh]
    nkp = round_up(nk, KEY_STEP)
    vh = np.zeros((s.heads, nkp, s.dh)); vh[:, :nk] = s.v.transpose(1, 0, 2)[kv_of]
    ntiles = (nq + Q_TILE - 1) // Q_TILE
    per = 1 if (sens or hide is not None) else 8                              # tiles per block (the tile alone where its steps matter)
    for t0 in range(0, ntiles, per):
        qs = np.arange(Q_TILE * t0, min(Q_TILE * (t0 + per), nq))
        # the keys any query of the block can admit, from the columns alone (not from the visit rule): columns increase with the packed index
        if win is None:
            lo, hi = 0, nk
        else:
            cq = s.col[qs].astype(np.int64)
            lo = int(np.searchsorted(colk, cq.min() - win[0], "left")) // KEY_STEP * KEY_STEP
            hi = int(np.searchsorted(colk, cq.max() + win[1], "right"))
        if hi <= lo:
            continue
        kbs = tile_steps(t0, nk, nq, win) if sens else None
        ok = None if (win is None and hide is None) else admits(s.col[qs], colk[lo:hi], win)
        if hide is not None:
            hid = hide(t0)
            ok[:, hid[(hid >= lo) & (hid < hi)] - lo] = False
        d = (colk[None, lo:hi].astype(np.int64) - s.col[qs][:, None] + BIAS_HALF) if tab is not None else None
        for h in range(s.heads):
            sc = s.q[qs, h] @ kh[h, lo:hi].T
            if tab is not None:
                sc += tab[h][d]
            if ok is not None:
                mx = np.where(ok, sc, -np.inf).max(1)
                mx[~np.isfinite(mx)] = 0.0                                    # a row without a key: all weights zero
            else:
                mx = sc.max(1)
            sc -= mx[:, None]
            if ok is not None:
                sc[~ok] = 0.0                                                 # (exp2 of -inf takes libm's slow path: the weight is set to zero below instead)
            w = np.exp2(sc, out=sc)
            if ok is not None:
                w[~ok] = 0.0
            den = w.sum(1)
            num = w @ vh[h, lo:hi]
            ctx = np.where(den[:, None] > 0, num / np.where(den > 0, den, 1.0)[:, None], 0.0)
            out[qs, h] = ctx
            if sens:
                S = (round_up(hi, KEY_STEP) - lo) // KEY_STEP
                w3 = np.zeros((len(qs), S * KEY_STEP)); w3[:, :hi - lo] = w
                w3 = w3.reshape(len(qs), S, KEY_STEP)
                den_s = w3.sum(2)                                             # [q, S]
                num_s = np.matmul(w3.transpose(1, 0, 2), vh[h, lo:lo + S * KEY_STEP].reshape(S, KEY_STEP, s.dh)).transpose(1, 0, 2)   # [q, S, dh]
                smax = w3.max(2)
                top = np.sort(smax, 1)[:, ::-1]
                second = top[:, 1] if S > 1 else np.zeros(len(qs))
                other = np.where(smax == top[:, :1], second[:, None], top[:, :1])      # the largest weight outside the step (exact: no cancellation)
                live = other > 0
                alt = np.where(live[..., None], (num[:, None] - num_s) / np.where(live, den[:, None] - den_s, 1.0)[..., None], 0.0)
                mv = np.abs(alt - ctx[:, None]).max((0, 2))                   # [S]
                held = den_s.max(0) > 0                                       # some query of the tile admits a key of the step
                for si in np.nonzero(held)[0]:
                    if lo + KEY_STEP * int(si) not in kbs:
                        moved[("unvisited", t0, lo + KEY_STEP * int(si))] = float(den_s[:, si].max())      # the visit rule would lose an admitted key
                for kb in kbs:
                    if not lo <= kb < hi:
                        moved.setdefault((t0, int(kb)), -1.0)
                        continue
                    key, si = (t0, int(kb)), (int(kb) - lo) // KEY_STEP
                    moved[key] = max(moved.get(key, 0.0 if held[si] else -1.0), float(mv[si]) if held[si] else -1.0)
    return (out, moved) if sens else out


@functools.lru_cache(maxsize=None)
def seq_reference(*key):
    r = reference(make_seq(*key))
    r.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------------------
# a batch: the probe's host arrays, laid out as ensure_ws allocates them
# ---------------------------------------------------------------------------------------------------------
def to_bits(x, dtype):
    """float64 -> the 16-bit patterns of the operand type; raises when a value does not survive"""
    x = np.asarray(x, np.float64)
    if dtype == "f16":
        b = x.astype(np.float16)
        back = b.astype(np.float64)
        bits = b.view(np.uint16)
    else:
        f = x.astype(np.float32).view(np.uint32)
        bits = (f >> 16).astype(np.uint16)
        back = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if not np.array_equal(back, x):
        raise ValueError("a value is not exact in " + dtype)
    return bits


def from_bits(b, dtype):
    b = np.asarray(b, np.uint16)
    return b.view(np.float16).astype(np.float64) if dtype == "f16" else (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


SENTINEL = {"f16": 0x7BFF, "bf16": 0x7F7F}      # the largest finite value of the type: no context row can hold it (|ctx| <= 2)


class Batch:
    pass


def make_batch(seqs, align, dtype, fill=FILLS[0]):
    """The host arrays of one launch: q / ctx [capT, H], k [capT + 64, ldk], vT [ldk, capT + 64], col [capT + 64] (ensure_ws: 64 rows, columns, entries of
    slack), offsets = exclusive scan of round_up(nq, align).  Everything outside the sequences' own rows — slack, alignment rows, the K / V^T row of a
    query-only CLS row — holds +-fill; ctx holds the sentinel"""
    b = Batch()
    s0 = seqs[0]
    H, ldk = s0.heads * s0.dh, s0.kv_heads * s0.dh
    offs, T = [], 0
    for s in seqs:
        offs.append(T); T += round_up(s.nq, align)
    capT = round_up(max(T, 1), 256)
    sign = np.where((np.arange(capT + 64) % 2) == 0, 1.0, -1.0)
    q = np.repeat((fill * sign[:capT])[:, None], H, 1)
    k = np.repeat((fill * sign)[:, None], ldk, 1)
    vT = np.repeat((-fill * sign)[None, :], ldk, 0)
    col = np.full(capT + 64, 12345, np.int32)
    for s, o in zip(seqs, offs):
        q[o:o + s.nq] = s.q.reshape(s.nq, H)
        k[o:o + s.nk] = s.k.reshape(s.nk, ldk)
        vT[:, o:o + s.nk] = s.v.reshape(s.nk, ldk).T
        col[o:o + s.nq] = s.col
    b.seqs, b.dtype, b.capT, b.H, b.ldk = seqs, dtype, capT, H, ldk
    b.q, b.k, b.vT, b.col = to_bits(q, dtype), to_bits(k, dtype), np.ascontiguousarray(to_bits(vT, dtype)), col
    b.off = np.array(offs, np.int32); b.nk = np.array([s.nk for s in seqs], np.int32); b.nq = np.array([s.nq for s in seqs], np.int32)
    b.ctx = np.full((capT, H), SENTINEL[dtype], np.uint16)
    b.rows = np.zeros(capT, bool)
    for s, o in zip(seqs, offs):
        b.rows[o:o + s.nq] = True
    return b


# ---------------------------------------------------------------------------------------------------------
# the error bound of a context element, derived from the kernels' rounding points (attn_softmax_pv, attn_store_tile)
# ---------------------------------------------------------------------------------------------------------
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}      # relative error of one rounding to nearest: 11 and 8 significand bits


def error_bound(dtype, nkeys):
    """max |ctx - ref| of any element of a row that admits at most nkeys keys, given |v| <= VMAX and inputs / scores that carry no rounding:
         ctx = fl16( fl32(sum_j P~_j v_j) / fl32(sum_j P_j) ),  P_j = exp2(s_j - mref) by v_exp_f32,  P~_j = P_j rounded to the operand type.
       The scores are exact (products of 16-bit values, sums of multiples of 1/64 below 2^10, in fp32) and so is s - mref.  mref never exceeds the running maximum,
       so the largest P is >= 1 and l = sum_j P_j >= 1; the deferred rescale keeps every P <= 2^8.
         (1) P to the operand type: |P~ - P| <= u P, the denominator sums the UNROUNDED P: |sum (P~ - P) v| / l <= u VMAX.  f16 only: a P below 2^-14 is
             subnormal, absolute error <= 2^-25 each: <= nkeys 2^-25 VMAX (l >= 1)
         (2) ctx to the operand type: <= u |ctx| <= u VMAX
         (3) v_exp_f32: 1 ulp, relative 2^-23 on P in numerator and denominator: <= 2 x 2^-23 VMAX
         (4) the fp32 sums.  Numerator: one rounding per key at the worst (the MFMA's internal order is not specified), each <= 2^-24 of a partial sum <= VMAX l.
             Denominator: 34 additions per 64-key step (32 in a lane, the half-wave exchange, l +=), each <= 2^-24 l.  Each of at most 8 rescales (scores
             span < 64 log2 units, one rescale per 8) rounds o and l once more; 1 / l and o * inv add 3 x 2^-24.  Together (nkeys + 34 nkeys / 64 + 34 + 16 + 3) 2^-24 VMAX
       The sum is the bound; (1) and (2) dominate: about 2^-10 VMAX for f16 and 2^-7 VMAX for bf16 (at 8192 keys the worst-case fp32 term adds 0.75 x 2^-10)"""
    u = UNIT[dtype]
    sub = nkeys * 2.0 ** -25 if dtype == "f16" else 0.0
    fp32 = (nkeys + 34.0 * nkeys / KEY_STEP + 34 + 16 + 3) * 2.0 ** -24
    return VMAX * (u + sub + u + 2 * 2.0 ** -23 + fp32)


# ---------------------------------------------------------------------------------------------------------
# what the tests run: lists of lengths per kernel, shapes per list
# ---------------------------------------------------------------------------------------------------------
GQA_LONG = [KCHUNK + 1, 3 * KEY_STEP + 1, Q_GROUP + Q_TILE + 1]      # 129, 193, 289: the many-headed shapes beyond one kchunk / one q-group
LONG_A = [2080, 8191, 8192]                                          # the long list, split by the heads its sparsest tile needs (_needles): 4 heads serve these,
LONG_B = [2049, 4097]                                                # a last tile of ONE query that visits 33 / 65 steps needs 7 / 11 heads x 6 targets
ALL_SHAPES = tuple((h, kv, dh) for dh in (32, 64) for h, kv in SHAPES) + ((SHAPE_64_ONLY[0], SHAPE_64_ONLY[1], 64),)
FULL_SHAPES = ((4, 4, 32), (4, 2, 32), (2, 1, 64), (6, 2, 64))       # these also run the whole DECODER_LONG (k_attn_dma) and DEBERTA_LONG (k_attn_lds) lists
LONG_CASES = (                                                       # (lengths, shape, modes)
    (LONG_A, (4, 2, 32), MODES), (LONG_A, (4, 4, 64), MODES),
    (LONG_B, (16, 1, 32), MODES), (LONG_B, (14, 2, 64), ("window", "causal")),
    (LONG, (16, 1, 32), ("window",)), (LONG, (14, 2, 64), ("window",)),      # the whole list as ONE batch, groups 16 and 7 at 8192 tokens: under the window the reference is cheap
)


def long_data(shape, mode):
    """the data sets a long case runs: the needles everywhere; the diffuse set under a window and causally (a cheap reference) and, on the 4 x 2 shape of d_h 32, in
    the plain mode too (every key of 8192 weighs in)"""
    return ("needles",) + (("diffuse",) if mode in ("window", "causal") or (mode == "plain" and shape == (4, 2, 32)) else ())


KINDS = ("right", "left", "holes", "cls", "cls-holes")               # dealt over the sequences of a list in turn (causal: the first three)


def list_kinds(lens, mode, shift=0):
    """[(n, kind)]: the lengths of a list with the column layouts dealt over them"""
    kinds = KINDS[:3] if mode == "causal" else KINDS
    return [(n, kinds[(i + shift) % len(kinds)]) for i, n in enumerate(lens)]


def edge_lists(shape):
    """name -> (kernel, lengths) of the lists a shape runs below the long ones.  kernel: "dma", or the heads per block of k_attn_lds the width selects"""
    out = {"short-%d" % w: (4 if w == 32 else 2 if w == 64 else 1, v) for w, v in SHORT.items()}
    out["gqa-long-lds"] = (1, GQA_LONG); out["gqa-long-dma"] = ("dma", GQA_LONG)
    if shape in FULL_SHAPES:
        out["deberta-long"] = (1, DEBERTA_LONG); out["decoder-long"] = ("dma", DECODER_LONG)
    return out
