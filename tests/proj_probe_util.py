"""Inputs, float64 reference, mutants and the derived error bound of the projection probe (tests/capi/proj_probe.hip, tests/test_proj_probe_host.py,
tests/test_gpu_proj_probe.py).  numpy only: importable without a GPU.

A case is described in CHECKPOINT order (q | k | v rows with the features of a head in their natural order; gate rows then up rows) and handed to the probe in
the PACKED order the loader gives the library (tile_pair_row of encoder_rows.hpp, restated here); the reference stays in checkpoint order.

Two data sets:
  exact    W dense in {-1, +1}; X has exactly one +-1 per (row, K-tile), at a column that depends on (row, tile).  An accumulator is then a sum of nk <= 152
           signs: every fp32 partial sum is an exact integer in any order, every K-tile moves every output element by exactly +-1.  Biases are integers in
           [-8, 8]; the rotary tables take only (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1)}, varying with position and pair index.  |value| <= 160 <= 256:
           exact in bf16 and in f16, so the linear epilogues have ONE correct bit pattern per element.
  diffuse  dense Gaussians rounded to 8 significant bits at each value's own exponent (round_sig8: exact in both operand types, and the fp32 partial sums
           really round, so a loop that summed K in another order would show in the bits): X of unit variance (|x| < 4), W with sigma sqrt(K) = 1.3
           (sharp_util.SIGMA_SQRT_H is 1.57), real RoPE tables (fp32).  One channel of X per K-tile is an outlier (x 32, like the massive activations of real
           transformer layers): it gives one K-tile enough weight at K = 9728 to stand above the worst-case fp32 summation bound (test_proj_probe_host.py), and
           it lifts the accumulators' standard deviation from 1.3 to about 5.3, so the set is NOT at the output scale of a plain layer.  The comparison is
           against float64 of the 16-bit operands."""
from functools import lru_cache

import numpy as np

UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}      # relative error of one rounding to nearest: 11 and 8 significand bits


def round_up(n, m):
    return (n + m - 1) // m * m


def to_bits(x, dtype):
    """float64 -> the 16-bit patterns of the operand type; raises when a value does not survive (as attn_probe_util.to_bits)"""
    x = np.asarray(x, np.float64)
    if dtype == "f16":
        b = x.astype(np.float16)
        back, bits = b.astype(np.float64), b.view(np.uint16)
    else:
        bits = (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        back = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if not np.array_equal(back, x):
        raise ValueError("a value is not exact in " + dtype)
    return bits


def from_bits(b, dtype):
    b = np.asarray(b, np.uint16)
    return b.view(np.float16).astype(np.float64) if dtype == "f16" else (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


EPI_QKV, EPI_DENSE, EPI_GELU, EPI_QKV_ROT, EPI_SWIGLU, EPI_GEGLU, EPI_QKV_ROTB, EPI_RELU, EPI_GEGLU_TANH, EPI_SPLADE = range(10)      # encoder_proj.hpp
EPI_NAMES = ("qkv", "dense", "gelu", "qkv_rot", "swiglu", "geglu", "qkv_rotb", "relu", "geglu_tanh", "splade")
ROTATES = (EPI_QKV_ROT, EPI_QKV_ROTB)
QKV_LIKE = (EPI_QKV,) + ROTATES
GATED = (EPI_SWIGLU, EPI_GEGLU, EPI_GEGLU_TANH)
HAS_BIAS = (EPI_QKV, EPI_GELU, EPI_GEGLU, EPI_QKV_ROTB, EPI_SPLADE)
LOOPS = (256, 128, 130, 64, 32)          # KIRAG_AMD_PROJ_TILE: ping-pong, streaming, producer / consumer, skinny 64 x 64, skinny 32 x 32
PERSISTENT = (256, 128, 130)
TILE_ROWS = {256: 256, 128: 128, 130: 128, 64: 64, 32: 32}
GUARD_ROWS, GUARD_T_ROWS, GUARD_T_COLS = 256, 32, 256      # proj_probe.hip
SENTINEL = {"f16": 0x7BFF, "bf16": 0x7F7F}                # the largest finite value of the type: no output of either data set reaches it
ROWS_HEAD64, ROWS_GATE, ROWS_UP = 0, 1, 2
SIGMA_SQRT_K = 1.3
OUTLIER = 32.0
FILLS = (3.0, -2.5)                      # what the rows >= T of X hold (finite, exact in both types; two values for the leak test)


def loops_of(epi):
    """the main loops the library builds for an epilogue"""
    return tuple(l for l in LOOPS if not (epi == EPI_QKV_ROTB and l == 256))


# ---------------------------------------------------------------------------------------------------------
# row orders
# ---------------------------------------------------------------------------------------------------------
def tile_pair_row(r, mode):
    """encoder_rows.hpp: the packed row of checkpoint row r"""
    r = np.asarray(r, np.int64)
    if mode == ROWS_HEAD64:
        b = (r >> 4) & 3
        return (r & ~np.int64(63)) + ((((b & 1) << 1) | (b >> 1)) << 4) + (r & 15)
    return ((r >> 4) << 5) + (16 if mode == ROWS_UP else 0) + (r & 15)


def tile_pair_row_inv(p, mode):
    """the checkpoint row of packed row p (ROWS_GATE / ROWS_UP: -1 where p holds a row of the other half)"""
    p = np.asarray(p, np.int64)
    if mode == ROWS_HEAD64:
        return tile_pair_row(p, ROWS_HEAD64)      # the block order 0, 2, 1, 3 is its own inverse
    mine = ((p >> 4) & 1) == (1 if mode == ROWS_UP else 0)
    return np.where(mine, ((p >> 5) << 4) + (p & 15), -1)


def packed_index(c):
    """perm [F]: packed row i holds checkpoint row perm[i] of the case's W (and bias)"""
    F = c.F
    ck_of = np.arange(F, dtype=np.int64)
    if c.epi in ROTATES and c.dh == 64:
        qk = c.H + c.A
        ck_of[:qk] = tile_pair_row_inv(np.arange(qk), ROWS_HEAD64)      # H % 64 == 0: q's and k's heads are permuted in place
    elif c.epi in GATED:
        FF = F // 2
        p = np.arange(F)
        g, u = tile_pair_row_inv(p, ROWS_GATE), tile_pair_row_inv(p, ROWS_UP)
        ck_of = np.where(g >= 0, g, FF + u)
    return ck_of


def stored_column(c, width):
    """[width]: the stored column of q / k that holds checkpoint feature i (the rotating epilogues store 64-wide heads in the rows' order)"""
    i = np.arange(width, dtype=np.int64)
    return tile_pair_row(i, ROWS_HEAD64) if (c.epi in ROTATES and c.dh == 64) else i


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
class Case:
    pass


def _hash(*xs):
    """a cheap integer hash of broadcast integer arrays (deterministic, no generator state)"""
    h = np.uint64(0x9E3779B97F4A7C15)
    for x in xs:
        with np.errstate(over="ignore"):
            h = (h ^ np.asarray(x).astype(np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            h ^= h >> np.uint64(29)
    return h


def _sign(*xs):
    return np.where(_hash(*xs) & np.uint64(1 << 20), 1.0, -1.0)


def round_sig8(v):
    """v rounded to 8 significant bits AT ITS OWN EXPONENT (a floating significand: exact in bf16; exponents below -17 share the quantum 2^-24, so exact in f16
    down to its subnormals).  Products of two such values are exact in fp32 but lie on different grids, so fp32 partial sums of them really round, and the
    order of a sum shows in its bits (test_proj_probe_host.py checks that it does)"""
    with np.errstate(divide="ignore"):
        e = np.maximum(np.floor(np.log2(np.abs(v))), -17.0)
    q = 2.0 ** (e - 7)
    return np.round(v / q) * q


def rope_tables(max_pos, dh, data):
    j = np.arange(dh // 2)
    p = np.arange(max_pos)[:, None]
    if data == "exact":
        q = (p + 3 * j[None, :] + (j[None, :] >> 4) + (p >> 2)) & 3      # quarter turns, varying with the position AND the pair index (and between j and j - 16)
        return np.array([1, 0, -1, 0], np.float32)[q], np.array([0, 1, 0, -1], np.float32)[q]
    ang = p * (10000.0 ** (-2.0 * j / dh))[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


MAX_POS = 99


def splade_rows(T):
    """row_seq of the splade shapes: sequences whose boundaries fall inside, on and 4 rows past a 32-row block, alignment rows (-1) behind each, -1 from T on"""
    ends = [4, 20, 64, 100, 132, 196, 230]   # row 0 alone; 20: inside a block; 64: on one; 100 = 96 + 4; 132 = 128 + 4; 196: inside; then whole blocks of one sequence
    rs = np.full(round_up(T, 256), -1, np.int32)
    start, seq = 0, 0
    for e in ends:
        if e >= T:
            break
        rs[start:e - 3] = seq      # three alignment rows before every boundary
        start, seq = e, seq + 1
    rs[start:T] = seq
    return rs, seq + 1


@lru_cache(maxsize=24)
def make_case(epi, data, T, F, K, H=0, A=0, dh=0, V=0, fill=FILLS[0]):
    c = Case()
    c.epi, c.data, c.T, c.F, c.K, c.H, c.A, c.dh, c.V = epi, data, T, F, K, H, A, dh, V
    c.capT = round_up(T, 256)
    c.ldT = c.capT + 64                       # ensure_ws: 64 columns behind V^T
    c.nk = K // 64
    c.max_pos = MAX_POS
    t, f, k = np.arange(c.capT)[:, None], np.arange(F)[:, None], np.arange(K)[None, :]
    if data == "exact":
        W = _sign(f, k, 1)
        kt = np.arange(c.nk)[None, :]
        col = (_hash(t, kt, 2) % np.uint64(64)).astype(np.int64)
        X = np.zeros((c.capT, K))
        np.put_along_axis(X, 64 * kt + col, _sign(t, kt, 3), 1)
        bias = (_hash(f[:, 0], 4) % np.uint64(17)).astype(np.float64) - 8.0
    else:
        rng = np.random.default_rng(1000 * epi + K + 7 * F + T)
        X = np.clip(rng.standard_normal((c.capT, K)), -3.96875, 3.96875)
        oc = 64 * np.arange(c.nk) + (np.arange(c.nk) * 37 + 11) % 64            # the outlier channel of every K-tile
        X[:, oc] *= OUTLIER
        X = round_sig8(X)
        W = round_sig8(rng.standard_normal((F, K)) * (SIGMA_SQRT_K / np.sqrt(K)))
        bias = np.clip(np.round(rng.standard_normal(F) * 32) / 64, -2, 2)
    X[T:] = fill * _sign(t[T:], k, 5)
    c.X, c.W, c.bias = X, W, bias.astype(np.float32)
    if epi in ROTATES:
        c.cos, c.sin = rope_tables(c.max_pos, dh, data)
        tp = ((np.arange(c.capT) * 7) % (c.max_pos - 2) + 1).astype(np.int32)
        for i, v in enumerate((6, c.max_pos - 1, -1, c.max_pos, 0)):      # the edges of the table and both sides beyond it, among the first rows
            tp[i] = v                                                      # (row 0: a position that turns every pair, for the shapes of one row)
        c.tpos = tp
    if epi == EPI_SPLADE:
        c.row_seq, c.nseq = splade_rows(T)
        b = c.bias.copy()
        b[5::11] = -400.0                     # all-negative columns: they stay 0
        b[V:] = 300.0                         # the padded columns behind V would be large if one were written
        if V > 70:
            b[70] = np.nan                    # a planted NaN: it survives in every sequence
        c.bias = b
    return c


def probe_arrays(c, dtype):
    """the packed host arrays of a case: X bits [capT, K], W bits [F, K] and bias [F] in the rows' packed order"""
    perm = packed_index(c)
    return to_bits(c.X, dtype), np.ascontiguousarray(to_bits(c.W, dtype)[perm]), np.ascontiguousarray(c.bias[perm])


def check_case(c, loop=256, blocks=0, nt=0, ant=0, epi_prio=0, pw=8):
    """the argument checks of proj_probe.hip (check_args), mirrored: a message, or None when the probe accepts the case"""
    if c.epi not in range(10) or loop not in LOOPS:
        return "epilogue / loop"
    if c.capT < 256 or c.capT % 256 or not 1 <= c.T <= c.capT:
        return "T / capT"
    if c.K < 64 or c.K % 64 or c.F < 64 or c.F % 64 or c.K > 65536 or c.F > 65536:
        return "K / F"
    if c.epi in QKV_LIKE:
        if c.H < 64 or c.H % 64 or c.A < 64 or c.A % 64 or c.H + 2 * c.A != c.F or (c.epi == EPI_QKV and c.A != c.H):
            return "F = H + 2 A"
        if c.ldT < c.capT or c.ldT % 8:
            return "ldT"
    if c.epi in ROTATES and (c.dh not in (32, 64) or c.max_pos < 1 or c.cos.shape != (c.max_pos, c.dh // 2) or c.sin.shape != c.cos.shape or len(c.tpos) != c.capT):
        return "rotary tables"
    if c.epi == EPI_SPLADE and (c.nseq < 1 or not 1 <= c.V <= c.F or len(c.row_seq) != c.capT or int(c.row_seq.max()) >= c.nseq or nt):
        return "splade"
    if c.epi == EPI_QKV_ROTB and loop == 256:
        return "EPI_QKV_ROTB on the 256 x 256 tile"
    if blocks and (loop not in PERSISTENT or blocks < 8 or blocks % 8 or blocks > 4096):
        return "blocks"
    if nt not in (0, 1) or (nt and loop not in (256, 128)) or ant not in (0, 1) or (ant and (loop != 256 or c.epi != EPI_DENSE)):
        return "nt / ant"
    if epi_prio not in (0, 1, 2) or not 1 <= pw <= 64:
        return "epi_prio / pw"
    if loop not in PERSISTENT and -(-c.T // loop) > 65535:
        return "token tiles"
    return None


# ---------------------------------------------------------------------------------------------------------
# the float64 reference, in checkpoint order; the mutants of test_proj_probe_host.py are switches of the same code
# ---------------------------------------------------------------------------------------------------------
try:      # as oracle/encoder_np.py: scipy where the image has it, math.erf vectorised otherwise
    from scipy.special import erf as _erf
except ImportError:
    import math
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu_erf(x):
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def gelu_new(x):
    """HF gelu_new, 0.5 x (1 + tanh(t)), as x / (1 + exp(-2 t)): the same function without the cancellation of 1 + tanh(t) at t << 0 (in float64 the tanh form
    is 0 from x = -6 on, where the true value — 6e-21 at x = -8 — is still a normal bf16 / fp32 number the kernel returns)"""
    t = np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-2.0 * t))


def silu(x):
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


@lru_cache(maxsize=6)
def accumulators(c):
    """(acc, absacc) [capT, F]: X . W^T and |X| . |W|^T in float64; the rows >= T are those of the source row T - 1 (what the streaming, producer / consumer and
    skinny loops compute there, which clamp the row; the ping-pong loop reads such rows as zeros through its buffer resource.  No test looks at them)"""
    Xc = c.X.copy()
    Xc[c.T:] = c.X[c.T - 1]
    return Xc @ c.W.T, np.abs(Xc) @ np.abs(c.W).T


def affected_tile(c):
    """the 32 x 32 block the accumulator mutants act on: the last 32-row block that holds a row < T, feature columns 32 .. 63 (q's, gate's)"""
    # (the last block is the partial one: its rows >= T come from the clamped source row)
    return (0 if c.epi == EPI_SPLADE else (c.T - 1) // 32 * 32), 32      # EPI_SPLADE: the block of the short sequences (a long one's max hides a block)


def swapped_rows(c):
    """token_rows_swapped: the last two rows < T that share a 32-row block"""
    if c.epi == EPI_SPLADE:
        return 1, 0
    hi = c.T - 1 if (c.T - 1) % 32 >= 1 else c.T - 2
    return hi, hi - 1


MUTANTS = ("ktile_hidden_first", "ktile_hidden_middle", "ktile_hidden_last", "ktile_twice", "token_rows_swapped", "feature_rows_swapped", "clamp_leak",
           "vT_untransposed", "k_pitch_H", "boundary_shifted", "rot_jbase0", "rot_sign", "next_position", "tpos_unmapped", "gate_up_exchanged",
           "geglu_biases_exchanged", "neighbour_quad_bias", "splade_alignment_row", "splade_neighbour_row", "column_past_V")


def applies(mut, c):
    """the cases a mutant can show in (elsewhere the mutated kernel computes the same function)"""
    if mut == "ktile_twice":
        return c.nk >= 2
    if mut == "token_rows_swapped":      # two rows < T of one 32-row block; EPI_SPLADE: row 0 (a sequence of its own) and the alignment row behind it
        return c.T >= 5 if c.epi == EPI_SPLADE else swapped_rows(c)[0] >= 1
    if mut == "clamp_leak":              # EPI_SPLADE: a row >= T is an alignment row (splade_alignment_row); it holds row T - 1's accumulators, which are in the max already
        return c.T < c.capT and c.epi != EPI_SPLADE
    if mut == "vT_untransposed":
        return c.epi in QKV_LIKE
    if mut == "k_pitch_H":
        return c.epi in ROTATES and c.A != c.H and c.T >= 2
    if mut == "boundary_shifted":
        return c.epi in QKV_LIKE
    if mut == "rot_jbase0":
        return c.epi in ROTATES and c.dh == 64
    if mut in ("rot_sign", "next_position"):
        return c.epi in ROTATES
    if mut == "tpos_unmapped":
        return c.epi in ROTATES and c.T >= 3
    if mut == "gate_up_exchanged":
        return c.epi in GATED
    if mut == "geglu_biases_exchanged":
        return c.epi == EPI_GEGLU
    if mut == "neighbour_quad_bias":
        return c.epi in HAS_BIAS
    if mut == "splade_alignment_row":
        return c.epi == EPI_SPLADE and bool((c.row_seq[:c.T] < 0).any())
    if mut == "splade_neighbour_row":
        return c.epi == EPI_SPLADE and c.nseq >= 2
    if mut == "column_past_V":
        return c.epi == EPI_SPLADE and c.V < c.F
    return True


def _rotate(c, x, width, mut, with_err=None):
    """x [T, width] (heads of dh) rotated by every row's position; with_err = (e [T, width]) returns the propagated error bound as well"""
    T, dh, half = c.T, c.dh, c.dh // 2
    tp = c.tpos[:T].astype(np.int64)
    if mut == "next_position":
        tp = c.tpos[1:T + 1].astype(np.int64) if T < c.capT else np.roll(tp, -1)
    if mut == "tpos_unmapped":
        pos = np.where(tp < 0, c.max_pos - 1, np.minimum(tp, c.max_pos - 1))      # what the table's neighbourhood would give: the row before / the last row
    else:
        pos = np.where((tp >= 0) & (tp < c.max_pos), tp, 0)
    j = np.arange(half)
    if mut == "rot_jbase0":
        j = j % 16                                                               # the odd tile of a 64-wide head reads the even tile's table entries
    cs, sn = c.cos[pos][:, j].astype(np.float64), c.sin[pos][:, j].astype(np.float64)
    if mut == "rot_sign":
        sn = -sn
    xh = x.reshape(T, width // dh, 2, half)
    a, b = xh[:, :, 0], xh[:, :, 1]
    out = np.stack([a * cs[:, None] - b * sn[:, None], b * cs[:, None] + a * sn[:, None]], 2).reshape(T, width)
    if with_err is None:
        return out
    eh = with_err.reshape(T, width // dh, 2, half)
    ea, eb = eh[:, :, 0], eh[:, :, 1]
    ac, asn = np.abs(cs)[:, None], np.abs(sn)[:, None]
    # two products and a sum in fp32: each product rounds once, the sum once more (of a value <= |a c| + |b s|)
    e1 = ac * ea + asn * eb + 2.0 ** -23 * (np.abs(a) * ac + np.abs(b) * asn)
    e2 = ac * eb + asn * ea + 2.0 ** -23 * (np.abs(b) * ac + np.abs(a) * asn)
    return out, np.stack([e1, e2], 2).reshape(T, width)


def reference(c, mut=None, dtype=None):
    """{"out0": [T, w0], "out1": [T, A], "outT": [A, T], "smax": [nseq (+ 1 guard row), V]} of the case in float64, checkpoint order.
    With dtype: (outputs, bounds), bounds = error_bound of every element, derived from the kernel's rounding points (see error_bound)."""
    T, F, K, H, A, epi = c.T, c.F, c.K, c.H, c.A, c.epi
    acc, absacc = accumulators(c)
    if mut is not None:
        acc = acc.copy()
    r0, c0 = affected_tile(c)
    rows, cols = slice(r0, r0 + 32), slice(c0, c0 + 32)
    if mut and mut.startswith("ktile"):
        kt = {"ktile_hidden_first": 0, "ktile_hidden_middle": c.nk // 2, "ktile_hidden_last": c.nk - 1, "ktile_twice": c.nk // 2 - 1 if c.nk > 2 else 0}[mut]
        Xc = np.where((np.arange(c.capT) < T)[:, None], c.X, c.X[T - 1])[rows]
        part = lambda t: Xc[:, 64 * t:64 * t + 64] @ c.W[cols, 64 * t:64 * t + 64].T
        acc[rows, cols] += (part(kt) - part(kt + 1)) if mut == "ktile_twice" else -part(kt)
    if mut == "token_rows_swapped":
        hi, lo = swapped_rows(c)
        acc[[hi, lo], cols] = acc[[lo, hi], cols]
    if mut == "feature_rows_swapped":          # every feature of the tile with its neighbour (one pair alone can tie on the exact set at nk = 1)
        acc[rows, cols] = acc[rows, c0 + (np.arange(32) ^ 1)]
    if mut == "clamp_leak":
        acc[T - 1, cols] = c.X[min(T, c.capT - 1)] @ c.W[cols].T      # the clamp one row late: row T - 1 is computed from the row behind it
    bias = c.bias.astype(np.float64)
    if mut == "neighbour_quad_bias":
        bias = bias[np.arange(F) ^ 4]
    a = acc[:T]
    u16 = UNIT[dtype] if dtype else 0.0
    # fp32 accumulation over K in an order the MFMA does not specify: at most one rounding per product, gamma_K sum |x w|; zero on the exact set
    e_acc = (K * 2.0 ** -24 / (1 - K * 2.0 ** -24)) * absacc[:T] if c.data == "diffuse" else np.zeros_like(a)
    tiny = 2.0 ** -25 if dtype == "f16" else 2.0 ** -125      # half the smallest subnormal of f16; bf16 / fp32: what a flush to zero loses

    def stored(v, e):      # the output rounded to the operand type: half an ulp of a value within e of v
        return e + u16 * (np.abs(v) + e) + tiny

    def add32(v, e):       # one fp32 addition (of the bias): a rounding of the sum
        return e + 2.0 ** -24 * (np.abs(v) + e)

    out, err = {}, {}
    if epi in (EPI_DENSE, EPI_RELU):
        v = a if epi == EPI_DENSE else np.maximum(a, 0.0)
        out["out0"], err["out0"] = v, stored(v, e_acc)
    elif epi == EPI_GELU:
        x = a + bias
        v = gelu_erf(x)
        # |gelu'| <= 1.13; gelu_erf_fast2: 9.4e-7 absolute in fp32 arithmetic (its comment)
        out["out0"], err["out0"] = v, stored(v, 1.13 * add32(x, e_acc) + 9.4e-7)
    elif epi in GATED:
        FF = F // 2
        g, u, eg, eu = a[:, :FF], a[:, FF:], e_acc[:, :FF], e_acc[:, FF:]
        if mut == "gate_up_exchanged":
            g, u, eg, eu = u, g, eu, eg
        if epi == EPI_GEGLU:
            bi, bg = bias[:FF], bias[FF:]
            if mut == "geglu_biases_exchanged":
                bi, bg = bg, bi
            g, u = g + bi, u + bg
            eg, eu = add32(g, eg), add32(u, eu)
            act, eact, rel = gelu_erf(g), 1.13 * eg + 9.4e-7, 2.0 ** -24                      # one product
        else:
            # x rcp(1 + exp2(z)) u with z = -x log2(e) (silu_mul: a rounded constant and a product = 2 roundings of z) or z = -2 log2(e) sqrt(2 / pi)
            # (x + 0.044715 x^3) (gelu_tanh_mul, built with -ffp-contract=off: 9 roundings — x x, x x x, the constant 0.044715f, its product, the sum, the constant sqrt(2 / pi),
            # its product, the constant -2 log2(e), its product —, all terms of one sign).  A relative error d of z is an absolute error |z| d in log2 units, i.e.
            # a relative error ln2 |z| d of exp2; v_exp_f32 adds 1 ulp (2^-23); |z| counts up to 128, beyond it exp2 is 0 or inf and the quotient
            # is x or -0 (absolute error < |x u| 2^-125: the last term of eact).  The sigmoid's relative error is at most that of exp2; then 1 + (2^-24), v_rcp_f32 (1 ulp,
            # 2^-23) and two products (2^-24 each).  |silu'|, |gelu_new'| <= 1.13
            if epi == EPI_SWIGLU:
                z, nround, act = g * 1.4426950408889634, 2, silu(g)
            else:
                z, nround, act = 2.8853900817779268 * 0.7978845608028654 * (g + 0.044715 * g ** 3), 9, gelu_new(g)
            rel_act = np.log(2.0) * np.minimum(np.abs(z), 128.0) * nround * 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -24
            eact, rel = 1.13 * eg + rel_act * np.abs(act) + np.abs(g) * 2.0 ** -125, 2.0 ** -24
        v = act * u
        e = np.abs(u) * eact + np.abs(act) * eu + eact * eu
        out["out0"], err["out0"] = v, stored(v, e + rel * (np.abs(v) + e))
    elif epi in QKV_LIKE:
        kq, kk, kv = slice(0, H), slice(H, H + A), slice(H + A, F)
        if mut == "boundary_shifted":
            kk = slice(H - 64, H - 64 + A)      # k's columns begin 64 features early
        q, k, v = a[:, kq], a[:, kk], a[:, kv]
        eq, ek, ev = e_acc[:, kq], e_acc[:, kk], e_acc[:, kv]
        if epi != EPI_QKV_ROT:
            q, k = q + bias[kq], k + bias[kk]
            eq, ek = add32(q, eq), add32(k, ek)
        if epi in ROTATES:
            q, eq = _rotate(c, q, H, mut, eq)
            k, ek = _rotate(c, k, A, mut, ek)
        vT, evT = v.T.copy(), ev.T
        if mut == "vT_untransposed":
            full = acc[:, H + A:]               # rows >= T: the clamped row's values
            blk = full[r0:r0 + 32, 0:32]        # [token, feature] of the tile at V^T rows 0 .. 31
            n = min(32, T - r0)
            vT[0:32, r0:r0 + n] = blk[:, :n]     # stored as it lies in the accumulators: [token][feature]
        if mut == "k_pitch_H":
            flat = np.zeros(c.capT * A)
            idx = (np.arange(T)[:, None] * H + np.arange(A)[None, :]).ravel()
            ok = idx < flat.size
            flat[idx[ok]] = k.ravel()[ok]
            k = flat.reshape(c.capT, A)[:T]
        out.update(out0=q, out1=k, outT=vT)
        err.update(out0=stored(q, eq), out1=stored(k, ek), outT=stored(vT, evT))
    else:
        V, ns = c.V, c.nseq
        x = a + bias
        ex = add32(x, e_acc)
        rs = c.row_seq[:T].astype(np.int64).copy()
        if mut == "splade_alignment_row":
            for i in np.flatnonzero(rs < 0):      # an alignment row is taken for a row of the sequence in front of it
                rs[i] = rs[i - 1] if i > 0 else 0
        if mut == "splade_neighbour_row":
            for s in range(1, ns):                # the first row of a sequence enters the max of the one before
                rs[int(np.flatnonzero(rs == s)[0])] = s - 1
        sm, es = np.zeros((ns + 1, F)), np.zeros((ns + 1, F))
        for s in range(ns):
            m = rs == s
            if m.any():
                with np.errstate(invalid="ignore"):
                    sm[s] = np.maximum(0.0, np.fmax.reduce(np.where(np.isnan(x[m]), np.inf, x[m]), 0))
                    sm[s] = np.where(np.isnan(x[m]).any(0), np.nan, sm[s])
                es[s] = np.nan_to_num(ex[m], nan=0.0).max(0)
        res = sm[:, :V].copy()
        if mut == "column_past_V":
            flat = res.ravel()
            for s in range(ns):
                flat[s * V + V] = np.fmax(flat[s * V + V], sm[s, V])      # column V of sequence s is column 0 of the row behind it (the last: the guard row)
        out["smax"], err["smax"] = res, es[:, :V]
    return (out, err) if dtype else out


def error_bound(c, dtype):
    """The bound of every output element of a case, derived from the kernel's rounding points (reference() computes it next to the values it bounds):
         fp32 accumulation over K:  gamma_K sum |x w| (one rounding per product at the worst; zero on the exact set, whose partial sums are integers)
         the bias:                  one fp32 addition
         the activation:            gelu_erf_fast2 9.4e-7 absolute (its comment), through |gelu'| <= 1.13; silu_mul / gelu_tanh_mul: the roundings of exp2's
                                    argument, v_exp_f32 and v_rcp_f32 at 1 ulp each, 1 + e and the two products, propagated through the product
         the rotation:              two products and a sum in fp32
         the output:                half an ulp of the operand type (EPI_SPLADE keeps fp32: none)
       Never tuned to a measurement."""
    return reference(c, dtype=dtype)[1]


def expected_bits(c, dtype):
    """the exact set's one correct bit pattern per element (the linear epilogues; EPI_SPLADE: the fp32 pattern)"""
    assert c.data == "exact"
    ref = reference(c)
    if c.epi == EPI_SPLADE:
        return {"smax": ref["smax"].astype(np.float32).view(np.uint32)}
    return {k: no_minus_zero(to_bits(v, dtype)) for k, v in ref.items()}      # to_bits raises when a value is not exact in the type


def no_minus_zero(bits):
    """-0 == +0: a rotation by a quarter turn multiplies a zero accumulator by -1"""
    return np.where(bits == 0x8000, 0, bits).astype(np.uint16)


EXACT_BITS = (EPI_DENSE, EPI_RELU, EPI_QKV, EPI_QKV_ROT, EPI_QKV_ROTB, EPI_SPLADE)      # bit patterns; the others: exact accumulators under an activation


def unpack_outputs(c, dtype, raw):
    """raw = the probe's guarded arrays -> {name: the bits of the rows < T in checkpoint order} (smax: the nseq rows and the guard row behind them)"""
    out = {}
    G = GUARD_ROWS
    if c.epi == EPI_SPLADE:
        return {"smax": raw["smax"][1:c.nseq + 2]}
    out["out0"] = raw["out0"][G:G + c.T]
    if c.epi in QKV_LIKE:
        out["out0"] = out["out0"][:, stored_column(c, c.H)]
        out["out1"] = raw["out1"][G:G + c.T][:, stored_column(c, c.A)]
        out["outT"] = raw["outT"][GUARD_T_ROWS:GUARD_T_ROWS + c.A, GUARD_T_COLS:GUARD_T_COLS + c.T]
    return out


# ---------------------------------------------------------------------------------------------------------
# what the tests run (tests/test_gpu_proj_probe.py launches these; tests/test_proj_probe_host.py shows on the same inputs that every mutant is seen)
# ---------------------------------------------------------------------------------------------------------
WALK = (1300, 768, 192)                                   # T, F, K: 6 token tiles of 256 (the last partial), odd nk; 18 tiles of 256^2, 66 of 128^2
EDGE_T = (1, 31, 32, 33, 127, 129, 255, 257)
EDGE_F, EDGE_K = 320, (64, 128)                           # 64 past a 128- and a 256-tile; nk = 1 and 2
LONG_K = (2560, 9728)
LONG_T, LONG_F = 300, 256
REGIONS = ((128, 128, 64), (128, 128, 32), (256, 64, 64), (256, 64, 32), (192, 64, 32))      # (H, A, dh) of the QKV epilogues
REGION_T, REGION_K = 300, 128
SPLADE_T = 237                                            # not a multiple of 32


def shape_kwargs(epi, F, region=None):
    """the epilogue's own arguments at F GEMM columns: QKV epilogues take F = H + 2 A (thirds unless a region says otherwise), EPI_SPLADE V = F - 37"""
    if epi in QKV_LIKE:
        if region is None:
            third = F // 3 // 64 * 64
            region = (F - 2 * third, third, 64) if epi in ROTATES else (F // 3, F // 3, 64)
        H, A, dh = region
        return dict(H=H, A=A, dh=dh if epi in ROTATES else 0)
    if epi == EPI_SPLADE:
        return dict(V=F - 37)
    return {}


def cases_of(epi, data):
    """every (name, case) the GPU test launches for an epilogue and data set"""
    out = []
    T, F, K = WALK
    out.append(("walk", make_case(epi, data, T, F, K, **shape_kwargs(epi, F))))
    for t in EDGE_T:
        for k in EDGE_K:
            F = 576 if epi == EPI_QKV else EDGE_F           # EPI_QKV splits F into thirds of whole 64s: 576 is 64 past a 128- and a 256-tile as well
            out.append(("edge-T%d-K%d" % (t, k), make_case(epi, data, t, F, k, **shape_kwargs(epi, F))))
    for k in LONG_K:
        F = 384 if epi == EPI_QKV else LONG_F
        out.append(("long-K%d" % k, make_case(epi, data, LONG_T, F, k, **shape_kwargs(epi, F))))
    if epi in QKV_LIKE:
        for H, A, dh in REGIONS:
            if epi == EPI_QKV and (A != H or dh != 64):     # thirds only, and the head width does not enter
                continue
            out.append(("region-%d-%d-%d" % (H, A, dh), make_case(epi, data, REGION_T, H + 2 * A, REGION_K, H=H, A=A, dh=dh if epi in ROTATES else 0)))
    if epi == EPI_SPLADE:
        for V in (EDGE_F, EDGE_F - 37):
            out.append(("splade-V%d" % V, make_case(epi, data, SPLADE_T, EDGE_F, 192, V=V)))
    return out
