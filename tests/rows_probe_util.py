"""Cases, numpy models, float64 references, the codec specification, the derived error bound and the mutants of the row-kernel probe (tests/capi/rows_probe.hip,
tests/test_rows_probe_host.py, tests/test_gpu_rows_probe.py).  numpy only: importable without a GPU.

The kernels (kirag_amd/csrc/encoder_rows.hpp): k_ln16 ("post"), k_ln16_pre ("pre"), k_ln16_head ("head"), k_embed_ln, k_embed_rms, k_qk_norm_rope ("qk"),
k_rot_pos, k_gather_cls, and through them lo_encode / lo_decode / lo_decode_final, whose specification (to_hi, encode, decode) lives here.

Every launch is held to one of two kinds of data:
  exact    constructions in which every fp32 operation of the kernel is exact in ANY order, so each output element has ONE correct bit pattern:
             signs  v = (y + bias) + decode(r) is +-1, in equal numbers per row (RMS: 3 : 1, so that a subtracted mean would show); y, the bias and BOTH halves of
                    the residual carry a part of it.  eps = 0, beta = 0: mu = 0, the variance is 1, rstd = 1 and o = +-g bit for bit — the output row is any
                    fp32 vector the test chooses (codec_sweep), xb must be its rounding and the low byte the specification's encode()
             mean   v = m +- D with m a per-row constant of 12 fractional bits, D = 1/2, integer beta, g on a 2^-10 grid: mu = m and rstd = 2 exactly, o = +-g + beta
             fixed  (pre-LN store) y = 0, bias = 0: v = decode(r) and the stored residual is the input (hi, byte) pair again, for every byte and both signs
           k_qk_norm_rope: x = +-a with a power of two a per (token, head), eps = 0, quarter-turn tables: every output is +-gq[f] or +-gk[f] of one feature
  diffuse  Gaussian rows with a few outlier channels (x 32) and small-variance rows (so that eps matters), real eps, g around 1, small beta, real RoPE tables:
           compared with float64 of the same 16-bit inputs and bytes within norm_bound / qk_bound, which are derived from the kernels' rounding points"""
import numpy as np

import proj_probe_util as P

UNIT, OUTLIER, SENTINEL = P.UNIT, P.OUTLIER, P.SENTINEL
MANT = {"f16": 10, "bf16": 7}           # stored significand bits
LO_SH = {"f16": 5, "bf16": 8}           # encoder_rows.hpp: 23 - MANT - 8
TINY = {"f16": 2.0 ** -25, "bf16": 2.0 ** -134}      # half the smallest subnormal of the type
MIN_NORMAL = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}
U32 = 2.0 ** -24                       # relative error of one fp32 rounding
GUARD = 8                               # rows_probe.hip
OPS = {"post": 0, "pre": 1, "head": 2, "embed_ln": 3, "embed_rms": 4, "qk": 5, "rot_pos": 6, "gather": 7}
ALIAS_RB_XB, ALIAS_RB, ALIAS_LO = 1, 2, 4
F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------
# the low byte's specification (lo_encode / lo_decode / lo_decode_final)
# ---------------------------------------------------------------------------------------------------------
def to_hi(x, kind):
    if kind == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) >> 16 << 16          # bf16: round to nearest even on the bit pattern
    return b.astype(np.uint32).view(np.float32)


def encode(x, hi, sh):
    d = (x.view(np.uint32).astype(np.int64) - hi.view(np.uint32).astype(np.int64) + 2**31) % 2**32 - 2**31      # int32 wrap
    return (np.clip(d + (1 << (sh - 1)) + (128 << sh), 0, (256 << sh) - 1) >> sh).astype(np.uint8)


def decode(byte, hi, sh, keep_inf=True):
    """lo_decode_final: what the readers of the final hidden state and the pre-LN residual use (a non-finite hi decodes to itself, round 5); for finite hi
    identical to the 3-instruction lo_decode of the post-LN residual path (keep_inf=False)"""
    x = ((hi.view(np.uint32).astype(np.int64) + (byte.astype(np.int64) << sh) - (128 << sh)) % 2**32).astype(np.uint32).view(np.float32)
    return np.where((hi.view(np.uint32) & 0x7f800000) == 0x7f800000, hi, x) if keep_inf else x


def bits16(hi, dtype):
    """fp32 values that ARE 16-bit operands -> their patterns"""
    hi = np.ascontiguousarray(hi, F32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return hi.astype(np.float16).view(np.uint16)
    return (hi.view(np.uint32) >> 16).astype(np.uint16)


def exact16(x, dtype):
    """bits16 of an INPUT: refuses a value that is no 16-bit operand (non-finite values pass as they are)"""
    b = bits16(x, dtype)
    assert np.array_equal(from16(b, dtype), np.asarray(x, F32), equal_nan=True), "a value is not exact in " + dtype
    return b


def from16(b, dtype):
    b = np.ascontiguousarray(b, np.uint16)
    return b.view(np.float16).astype(F32) if dtype == "f16" else (b.astype(np.uint32) << 16).view(F32)


def codec(x, dtype):
    """fp32 -> (the 16-bit pattern, the low byte) as the kernels store a value"""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(invalid="ignore"):
        hi = to_hi(x, dtype)
    return bits16(hi, dtype), encode(x, hi, LO_SH[dtype])


def codec_sweep(H, dtype, seed):
    """H positive fp32 values that sweep the codec: binade edges, the clamped tie (byte 255) and the tie that rounds up (byte 0), |x| < 2^-25, the f16
    subnormal range, values beyond 65504 (f16: hi = inf, byte 0), then the specification's own distribution (Gaussian x exp(U(-6, 3)))"""
    rng = np.random.default_rng(seed)
    t = 2.0 ** -(MANT[dtype] + 1)
    special = [1.0, 2.0, 1.9999999, 0.5, 1 + t, 1 + 3 * t, 1 + t * (1 - 2.0 ** -10), 1 + t * (1 + 2.0 ** -10), 2 - t, 2.0 ** -26, 1e-8, 2.0 ** -25, 2.0 ** -24, 5.9e-8,
               6.1e-8, 3.0e-5, 3.1e-5 * 1.37, 6.09e-5, 6.11e-5, 65504.0, 65519.0, 65520.0, 7.0e4, 1.0e5]
    x = np.abs(rng.standard_normal(H) * np.exp(rng.uniform(-6, 3, H))).astype(F32)
    x[x == 0] = 1.0
    x[rng.permutation(H)[:len(special)]] = np.float32(special)
    return x


# ---------------------------------------------------------------------------------------------------------
# the norm family: k_ln16, k_ln16_pre, k_ln16_head, k_embed_ln, k_embed_rms
# ---------------------------------------------------------------------------------------------------------
class Case:
    pass


_hash = P._hash
N_WORD, N_POS, N_TYPE = 8, 6, 2
EMBED_IDS = (7, 2, 7, 4, 0, 5, 3, 7, 1)      # repeated ids, the last row of every table (word 7, position (4 + 1) % 6 = 5, type 7 % 2 = 1)


def pos_of(w):
    return (np.asarray(w) + 1) % N_POS


def type_of(w):
    return np.asarray(w) % N_TYPE


def _signs(T, H, seed, share):
    rng = np.random.default_rng(seed)
    s = -np.ones((T, H))
    for t in range(T):
        s[t, rng.permutation(H)[:int(H * share)]] = 1.0
    return s


def _pick(vals, *xs):
    return np.asarray(vals, F64)[(_hash(*xs) >> np.uint64(7)) % np.uint64(len(vals))]


def _outlier_cols(H, seed):
    return np.random.default_rng(seed + 99).permutation(H)[:max(2, H // 128)]


def make_norm_case(op, kind, dtype, H, T, rms=False, eps=None, seed=0, has_lo=True):
    """op: post / pre / head / embed_ln / embed_rms; kind: signs / mean / fixed / diffuse (see the module's header)"""
    assert op in ("post", "pre", "head", "embed_ln", "embed_rms") and kind in ("signs", "mean", "fixed", "diffuse")
    assert not (rms and op in ("post", "head", "embed_ln")) and (op != "embed_rms" or rms) and not (rms and kind == "mean")
    assert kind != "fixed" or op in ("pre", "embed_rms")
    c = Case()
    c.op, c.kind, c.dtype, c.H, c.T, c.capT, c.rms, c.has_lo, c.seed = op, kind, dtype, H, T, T + 3, rms, has_lo, seed
    c.NS = 1 if H <= 512 else 2 if H <= 1024 else 4
    rng = np.random.default_rng(1000 * seed + H + 7 * T)
    sh, capT = LO_SH[dtype], c.capT
    col, row = np.arange(H)[None, :], np.arange(capT)[:, None]
    exact = kind in ("signs", "mean")
    c.eps = 0.0 if exact else (1e-5 if eps is None else eps)
    c.exact_keys = {"signs": ("xb", "xlo", "rb", "rlo"), "mean": ("xb", "xlo", "rb", "rlo"), "fixed": ("rb", "rlo"), "diffuse": ()}[kind]
    # gamma, beta: the output row of the exact sets
    if kind == "signs":
        c.g, c.beta = codec_sweep(H, dtype, seed + H), np.zeros(H, F32)
    elif kind == "mean":
        c.g = (_pick(np.arange(1, 4096), col[0], seed) * 2.0 ** -10 * np.where(_hash(col[0], 5) & np.uint64(4), 1, -1)).astype(F32)
        c.beta = _pick(np.arange(-8, 9), col[0], seed, 3).astype(F32)
    else:
        c.g, c.beta = (1 + 0.1 * rng.standard_normal(H)).astype(F32), (0.05 * rng.standard_normal(H)).astype(F32)
    if rms:
        c.beta = (1.5 + np.abs(c.beta)).astype(F32) if not exact else np.full(H, 3.0, F32)      # never read under RMS: a kernel that read it would show
    # the target v of the exact sets
    s = _signs(capT, H, seed + 1, 0.75 if rms else 0.5)
    D = 0.5
    m = (2 * (512 + (_hash(row[:, 0], seed, 11) % np.uint64(512)).astype(F64)) + 1) / 4096      # [0.25, 0.5), 12 fractional bits, never a 16-bit tie
    if op == "head":
        m = 0.25 + (_hash(row[:, 0], seed, 11) % np.uint64(4)).astype(F64) / 16                 # y itself carries it: exact in bf16
    V = s if kind == "signs" else m[:, None] + D * s
    c.y = c.ybias = c.r_hi = c.r_lo = None
    if op in ("post", "pre"):
        c.y, c.ybias = np.zeros((capT, H)), np.zeros(H)
        if kind == "signs":
            cc = _pick([-0.75, -0.25, 0.25, 0.75], col[0], seed, 1)
            sg = np.where(_hash(col[0], seed, 2) & np.uint64(8), 1.0, -1.0)
            R = (sg[None, :] * _pick([1.25, 1.5], row, col, seed)).astype(F32)            # never a binade's first value: the byte's unit is one size on both sides
            mm = (1 + _hash(col[0], seed, 3) % np.uint64(127)).astype(np.int64) * np.where(_hash(col[0], seed, 4) & np.uint64(16), 1, -1)
            mm = mm * int(has_lo)                                                        # without a low half the kernel has to see byte 128: no part there
            c.r_hi, c.r_lo = R, np.broadcast_to((128 + mm).astype(np.uint8), (capT, H)).copy()
            rho = decode(c.r_lo, R, sh).astype(F64)
            phi = rho[0] - R[0]                                                          # the byte's part: a function of the column alone
            assert np.array_equal(rho - R, np.broadcast_to(phi, (capT, H))) and ((phi != 0).all() or not has_lo)
            c.ybias, c.y = cc - phi, s - cc[None, :] - R
        elif kind == "mean":
            cc = _pick([-0.75, -0.25, 0.25, 0.75], col[0], seed, 1)
            c.ybias, c.y = cc, D * s - cc[None, :]
            hb, c.r_lo = codec(np.broadcast_to(m[:, None], (capT, H)), dtype)
            c.r_hi = from16(hb, dtype)
            assert np.array_equal(decode(c.r_lo, c.r_hi, sh).astype(F64), np.broadcast_to(m[:, None], (capT, H)))
        elif kind == "fixed":
            # every byte value on both signs; hi with a non-zero stored significand (below a binade's first value the unit halves and the pair is re-rounded),
            # byte 0 (hi - ulp / 2, a tie) only on an even hi (the tie rounds back to it)
            man = 1 + (_hash(row, col, seed) % np.uint64((1 << MANT[dtype]) - 1)).astype(np.int64)
            byte = ((col + 37 * row) % 256).astype(np.uint8)
            man = np.where((byte == 0) & (man % 2 == 1), man + 1 if MANT[dtype] > 1 else man, man)
            man = np.where(man >= (1 << MANT[dtype]), 2, man)
            ex = -6 + (_hash(row, col, seed, 9) % np.uint64(10)).astype(np.int64)
            sg = np.where(_hash(row, col, seed, 8) & np.uint64(2), 1.0, -1.0)
            c.r_hi, c.r_lo = (sg * (1 + man * 2.0 ** -MANT[dtype]) * 2.0 ** ex).astype(F32), byte
        else:
            scale = np.where(row % 3 == 1, 2.0 ** -7, 1.0)                                # small-variance rows: eps of 1e-5 / 1e-6 matters there
            out = np.ones(H)
            out[_outlier_cols(H, seed)] = OUTLIER
            c.y = P.round_sig8(rng.standard_normal((capT, H)) * scale * out)
            c.ybias = (0.1 * rng.standard_normal(H) * 2.0 ** -7).astype(F32).astype(F64)
            hb, c.r_lo = codec((rng.standard_normal((capT, H)) * scale * out).astype(F32), dtype)
            c.r_hi = from16(hb, dtype)
        c.y, c.ybias, c.r_hi = np.ascontiguousarray(c.y, F32), np.ascontiguousarray(c.ybias, F32), np.ascontiguousarray(c.r_hi, F32)
    elif op == "head":
        if exact:
            c.y = np.ascontiguousarray(V, F32)
        else:
            out = np.ones(H)
            out[_outlier_cols(H, seed)] = OUTLIER
            c.y = P.round_sig8(rng.standard_normal((capT, H)) * np.where(row % 3 == 1, 2.0 ** -10, 1.0) * out).astype(F32)      # (only xb is compared: eps has to show in 16 bits)
        c.row_seq = np.where(np.arange(capT) % 4 == 3, -1, np.arange(capT) // 4).astype(np.int32)
    else:
        c.tok_id = np.resize(np.int32(EMBED_IDS), capT).astype(np.int32)
        c.tok_pos, c.tok_type = pos_of(c.tok_id).astype(np.int32), type_of(c.tok_id).astype(np.int32)
        w = np.arange(N_WORD)[:, None]
        if op == "embed_ln":
            if exact:
                Pt = _pick(np.arange(-8, 9) * 0.25, np.arange(N_POS)[:, None], col, seed, 21)
                Qt = _pick([-1.5, -0.5, 0.5, 1.5], np.arange(N_TYPE)[:, None], col, seed, 22)
                sw = _signs(N_WORD, H, seed + 2, 0.5)
                mw = (2 * (512 + (_hash(w[:, 0], seed, 12) % np.uint64(512)).astype(F64)) + 1) / 4096
                Vw = sw if kind == "signs" else mw[:, None] + D * sw
                Wt = Vw - Pt[pos_of(w[:, 0])] - Qt[type_of(w[:, 0])]      # each word completes ITS position and type row to the target: any other row shows
            else:
                out = np.ones(H)
                out[_outlier_cols(H, seed)] = OUTLIER
                Wt = rng.standard_normal((N_WORD, H)) * out * np.where(w % 3 == 1, 2.0 ** -7, 1.0)
                Pt, Qt = 0.3 * rng.standard_normal((N_POS, H)) * np.where(np.arange(N_POS)[:, None] % 3 == 2, 2.0 ** -7, 1.0), 0.1 * rng.standard_normal((N_TYPE, H)) * 2.0 ** -7
            c.word, c.pos, c.type = np.ascontiguousarray(Wt, F32), np.ascontiguousarray(Pt, F32), np.ascontiguousarray(Qt, F32)
        else:
            if kind == "signs":
                Wt = _signs(N_WORD, H, seed + 2, 0.75)
            elif kind == "fixed":      # the stored residual is the codec of any fp32 row: the sweep with signs
                Wt = np.stack([codec_sweep(H, dtype, seed + 31 * k) * np.where(_hash(col[0], k, seed) & np.uint64(4), 1, -1) for k in range(N_WORD)])
            else:
                out = np.ones(H)
                out[_outlier_cols(H, seed)] = OUTLIER
                Wt = rng.standard_normal((N_WORD, H)) * out * np.where(w % 3 == 1, 2.0 ** -10, 1.0)      # (only xb is normalised: eps has to show in 16 bits)
            c.word = np.ascontiguousarray(Wt, F32)
    return c


def _rowsum(x, order):
    """row sums of x [T, H] in x's type.  fp32 orders: seq (left to right), rev, lane (Ln16: a lane owns 8 consecutive elements of every 512-element step,
    adds them step by step, then the xor butterfly 32, 16, .., 1 over the 64 lanes)"""
    if x.dtype == F64:
        return x.sum(1)
    T, H = x.shape
    if order == "seq":
        return np.cumsum(x, axis=1, dtype=F32)[:, -1]
    if order == "rev":
        return np.cumsum(x[:, ::-1], axis=1, dtype=F32)[:, -1]
    ns = (H + 511) // 512
    pad = np.zeros((T, ns * 512), F32)
    pad[:, :H] = x
    lane = np.cumsum(pad.reshape(T, ns, 64, 8).transpose(0, 2, 1, 3).reshape(T, 64, ns * 8), axis=2, dtype=F32)[:, :, -1]
    for mth in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, np.arange(64) ^ mth]
    return lane[:, 0]


NORM_MUTANTS = ("lo_ignored", "lo_pair_swapped", "lo_word0", "lo_step_dropped", "no_ybias", "no_beta", "no_eps", "padded_mean", "rms_subtracts_mean", "rms_reads_beta",
                "res_after_norm", "res_no_lo", "keep_inf_off", "pos_at_id", "type_at_0")


def norm_applies(mut, c):
    """the cases a mutant of the norm family acts on (and on which set it can be seen at all)"""
    res = c.op in ("post", "pre")
    if mut in ("lo_ignored", "lo_pair_swapped", "lo_word0", "lo_step_dropped"):
        return res and c.has_lo and c.kind != "mean"      # the mean set's bytes are one constant per row, which the mean removes: the other sets catch these
    if mut == "no_ybias":
        return res and c.kind != "fixed"
    if mut == "no_beta":
        return not c.rms and c.kind in ("mean", "diffuse")                  # the signs set has beta = 0: the mean set and the diffuse set catch it
    if mut == "no_eps":
        return c.kind == "diffuse" and c.eps >= 1e-6                        # the exact sets have eps = 0: the diffuse set's small-variance rows catch it
    if mut == "padded_mean":
        return c.H != 512 * c.NS
    if mut in ("rms_subtracts_mean", "rms_reads_beta"):
        return c.rms
    if mut in ("res_after_norm", "res_no_lo"):
        return c.op in ("pre", "embed_rms") and (mut == "res_after_norm" or (c.has_lo and c.kind in ("mean", "fixed", "diffuse")))
    if mut == "keep_inf_off":
        return False                                                        # seen only with a planted non-finite element: keep_inf_case
    if mut in ("pos_at_id", "type_at_0"):
        return c.op == "embed_ln"
    raise KeyError(mut)


def _combine(c, ft, mut):
    T, H, sh = c.T, c.H, LO_SH[c.dtype]
    if c.op in ("post", "pre"):
        byte = c.r_lo[:T].copy() if c.has_lo else np.full((T, H), 128, np.uint8)
        if mut == "lo_ignored":
            byte[:] = 128
        elif mut == "lo_pair_swapped":
            byte = byte.reshape(T, H // 2, 2)[:, :, ::-1].reshape(T, H)
        elif mut == "lo_word0":
            byte = byte.reshape(T, H // 8, 8).copy()
            byte[:, :, 4:] = byte[:, :, :4]
            byte = byte.reshape(T, H)
        elif mut == "lo_step_dropped":
            byte[:, 512 * ((H - 1) // 512):] = 128
        with np.errstate(invalid="ignore", over="ignore"):
            r = decode(byte, c.r_hi[:T], sh, keep_inf=c.op == "pre" and mut != "keep_inf_off").astype(ft)
            b = np.zeros(H, ft) if mut == "no_ybias" else c.ybias.astype(ft)
            return (c.y[:T].astype(ft) + b[None, :]) + r
    if c.op == "head":
        return c.y[:T].astype(ft)
    ids = c.tok_id[:T]
    if c.op == "embed_rms":
        return c.word[ids].astype(ft)
    p = ids % N_POS if mut == "pos_at_id" else c.tok_pos[:T]
    ty = np.zeros(T, np.int64) if mut == "type_at_0" else c.tok_type[:T]
    return (c.word[ids].astype(ft) + c.pos[p].astype(ft)) + c.type[ty].astype(ft)


def norm_forward(c, ft=F32, order="seq", mut=None):
    """the kernel's arithmetic in `ft` (fp32: every operation rounded once, no contraction, the row sums in `order`): (o, v) = the normalised row before its
    rounding to 16 bits, the residual sum"""
    H = c.H
    v = _combine(c, ft, mut)
    n = ft(512 * c.NS if mut == "padded_mean" else H)
    eps = ft(0.0 if mut == "no_eps" else c.eps)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mean = (not c.rms) or mut == "rms_subtracts_mean"
        mu = (_rowsum(v, order) / n) if mean else np.zeros(c.T, ft)
        d = v - mu[:, None]
        q = _rowsum(d * d, order)
        rstd = ft(1.0) / np.sqrt(q / n + eps)
        o = d * rstd[:, None] * c.g.astype(ft)[None, :]
        if (not c.rms and mut != "no_beta") or mut == "rms_reads_beta":
            o = o + c.beta.astype(ft)[None, :]
    return o, v


def norm_outputs(c, o, v, mut=None):
    """the stored patterns of fp32 (o, v): xb / xlo of the normalised row, rb / rlo of the residual (k_ln16_pre, k_embed_rms)"""
    xb, xlo = codec(o, c.dtype)
    out = {"xb": xb, "xlo": xlo}
    if c.op in ("pre", "embed_rms"):
        out["rb"], out["rlo"] = codec(o if mut == "res_after_norm" else v, c.dtype)
        if mut == "res_no_lo":
            out["rlo"] = np.full_like(out["rlo"], 128)
    return out


def norm_keys(c):
    return {"post": ("xb", "xlo"), "pre": ("xb", "xlo", "rb", "rlo"), "head": ("xb",), "embed_ln": ("xb", "xlo"), "embed_rms": ("xb", "rb", "rlo")}[c.op]


def norm_expected(c, mut=None):
    """the exact set's one correct pattern per element (keys: c.exact_keys that the op has)"""
    o, v = norm_forward(c, F32, "seq", mut)
    out = norm_outputs(c, o, v, mut)
    return {k: out[k] for k in norm_keys(c) if k in c.exact_keys}


def _depth(c):
    """additions on the longest path of a row sum: Ln16 8 NS - 1 in the lane + 6 in the butterfly; ln_row_store (k_embed_ln) 4 per 256-element step + 6"""
    return 4 * ((c.H + 255) // 256) + 6 if c.op == "embed_ln" else 8 * c.NS + 5


def norm_bound(c):
    """float64 reference (o, v) and the derived bound (do, dv) on |fp32 kernel value - reference| BEFORE the final rounding, from the kernel's rounding points:
    the two fp32 adds of the combine; the two row sums (gamma_d of the lane order's depth d); the divides by H, the add of eps, one sqrt, one divide (HIP's
    correctly rounded forms); the subtraction of the mean, two multiplies and the add of beta per element"""
    o, v = norm_forward(c, F64)
    u, H = U32, c.H
    if c.op in ("post", "pre"):
        a = np.abs(c.y[:c.T].astype(F64) + c.ybias.astype(F64)[None, :])
    elif c.op == "embed_ln":
        a = np.abs(c.word[c.tok_id[:c.T]].astype(F64) + c.pos[c.tok_pos[:c.T]].astype(F64))
    else:
        a = None                                                             # v is an input: no rounding
    dv = u * (a + np.abs(v)) * (1 + 2 * u) if a is not None else np.zeros_like(v)
    d_ = _depth(c)
    gam = d_ * u / (1 - d_ * u)
    if c.rms:
        mu, dmu = np.zeros(c.T), np.zeros(c.T)
    else:
        mu = v.sum(1) / H
        dmu = (gam * np.abs(v).sum(1) + dv.sum(1)) / H * (1 + u) + u * np.abs(mu)
    d = v - mu[:, None]
    dd = dv + dmu[:, None] + (0 if c.rms else u) * np.abs(d)
    q = (d * d).sum(1)
    dq = (2 * np.abs(d) * dd + dd * dd).sum(1) * (1 + gam) + (u + gam) * (1 + u) * q
    w = q / H + c.eps
    dw = dq / H * (1 + 2 * u) + 2 * u * w
    rel = 0.5 * (dw / w) / (1 - dw / w) ** 1.5 + 2 * u * (1 + u)
    rstd = 1 / np.sqrt(w)
    do = np.abs(c.g.astype(F64))[None, :] * rstd[:, None] * (dd + np.abs(d) * (rel[:, None] + 2 * u)) * (1 + 4 * u) + (0 if c.rms else u) * np.abs(o)
    return o, v, do, dv


def bound16(ref, dref, dtype):
    """|stored 16-bit value - reference|: the fp32 error, then one rounding to the operand type"""
    return dref + UNIT[dtype] * (np.abs(ref) + dref) + TINY[dtype]


def bound_lo(dref, hi_bits, byte, dtype):
    """|decode(byte, hi) - reference|: the fp32 error, then half a unit of the codec, ulp(hi) / 256 (one whole unit at the clamped tie, byte 255); hi = 0
    or subnormal in the operand type (its values are 2^-24 apart in f16, more than 256 units of the byte): never worse than the 16-bit operand alone, half
    that spacing (the specification: tests/test_lo_codec_spec.py)"""
    hi = np.abs(from16(hi_bits, dtype).astype(F64))
    normal = hi > MIN_NORMAL[dtype]      # (the smallest normal value too: below it the spacing does not halve, and half of it is 256 of the halved units)
    unit = np.exp2(np.floor(np.log2(np.where(normal, hi, 1.0))) - MANT[dtype] - 8)
    return dref + np.where(normal, unit * np.where(np.asarray(byte) == 255, 1.0, 0.5), TINY[dtype])


def decoded(hi_bits, byte, dtype):
    return decode(np.asarray(byte, np.uint8), from16(hi_bits, dtype), LO_SH[dtype]).astype(F64)


def keep_inf_case(c, what, t=1, i=5):
    """a copy of a pre-LN case with ONE non-finite residual element: hi = +-inf with byte 0 (what the encoder stores for an overflow: on the bit patterns
    alone it would decode to a finite 3.4e38) or a NaN"""
    d = Case()
    d.__dict__.update(c.__dict__)
    d.r_hi, d.r_lo = c.r_hi.copy(), c.r_lo.copy()
    d.r_hi[t, i] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[what]
    d.r_lo[t, i] = 0
    d.planted = (t, i)
    return d


# ---------------------------------------------------------------------------------------------------------
# k_qk_norm_rope
# ---------------------------------------------------------------------------------------------------------
QK_MUTANTS = ("partner_plain64", "gk_for_q", "epsq_for_k", "k_rows_by_heads", "rot_before_norm", "rot_sign", "pos_not_clamped")
QK_MAX_POS = 11


def make_qk_case(kind, dtype, dh, heads, kv_heads, T, seed=0):
    c = Case()
    c.op, c.kind, c.dtype, c.dh, c.heads, c.kv_heads, c.T, c.capT, c.max_pos = "qk", kind, dtype, dh, heads, kv_heads, T, T + 3, QK_MAX_POS
    rng = np.random.default_rng(seed + 13 * dh + heads + 100 * T)
    f = np.arange(dh)
    shape = (c.capT, heads + kv_heads, dh)
    t_, h_, f_ = np.arange(shape[0])[:, None, None], np.arange(shape[1])[None, :, None], f[None, None, :]
    c.tpos = np.resize(np.int32([3, -1, QK_MAX_POS, 7, 0, 10, 1 << 30, -(1 << 31)]), c.capT).astype(np.int32)
    if kind == "exact":
        a = 2.0 ** ((_hash(t_, h_, seed) % np.uint64(7)).astype(F64) - 3)
        x = a * np.where(_hash(t_, h_, f_, seed, 1) & np.uint64(32), 1.0, -1.0)
        c.gq, c.gk = ((64 + f) / 64).astype(F32), (-(64 + (5 * f + 3) % 128) / 256).astype(F32)      # 8 significant bits, distinct per feature and between q and k
        c.eps_q = c.eps_k = 0.0
        c.cos, c.sin = P.rope_tables(c.max_pos, dh, "exact")
    else:
        out = np.ones(dh)
        out[[3, dh // 2 + 1]] = OUTLIER
        small = ((t_ + h_) % 3 == 1) | ((h_ >= heads) & ((t_ + h_) % 2 == 0))      # heads whose mean square is below eps: there eps_q != eps_k shows
        x = P.round_sig8(rng.standard_normal(shape) * np.where(small, 2.0 ** -14, 1.0) * out)
        c.gq, c.gk = (2.5 * rng.uniform(0.6, 1.6, dh)).astype(F32), rng.uniform(0.6, 1.6, dh).astype(F32)
        c.eps_q, c.eps_k = float(F32(1e-6 / 16)), float(F32(1e-6))          # eps_q = s^2 eps of a folded score scale s = 1 / 4
        c.cos, c.sin = P.rope_tables(c.max_pos, dh, "diffuse")
    c.cos, c.sin = np.ascontiguousarray(c.cos, F32), np.ascontiguousarray(c.sin, F32)
    c.x = np.ascontiguousarray(x, F32)              # [capT, heads + kv_heads, dh]: q's heads, then k's, features in their natural order
    return c


def stored_order(dh):
    """where feature j of a head lies in a stored row: tile-pair order for 64-wide heads (ROWS_HEAD64), plain otherwise"""
    j = np.arange(dh)
    return P.tile_pair_row(j, P.ROWS_HEAD64) if dh == 64 else j


def qk_arrays(c):
    """(q [capT, heads dh], k [capT, kv_heads dh]) as stored rows (fp32 values that are 16-bit operands)"""
    p = stored_order(c.dh)
    st = np.empty_like(c.x)
    st[:, :, p] = c.x
    return st[:, :c.heads].reshape(c.capT, -1), st[:, c.heads:].reshape(c.capT, -1)


def qk_applies(mut, c):
    if mut == "partner_plain64":
        return c.dh == 64
    if mut == "epsq_for_k":
        return c.kind == "diffuse"          # eps_q = eps_k = 0 on the exact set: the diffuse set's small heads catch it
    if mut == "k_rows_by_heads":
        return c.kv_heads != c.heads and c.T > 1
    if mut == "pos_not_clamped":
        return c.T > 1                      # the first row's position is in range
    return True


def qk_forward(c, ft=F32, mut=None):
    """(q', k') [T, heads, dh], [T, kv_heads, dh] in `ft`, natural feature order, before the rounding to 16 bits"""
    T, dh, half, nh = c.T, c.dh, c.dh // 2, c.heads + c.kv_heads
    x = c.x[:T].astype(ft)
    if mut == "partner_plain64":          # the stored row read as if it were in plain order
        p = stored_order(dh)
        st = np.empty_like(x)
        st[:, :, p] = x
        x = st
    if mut == "k_rows_by_heads":          # unit (t, j) of k works on k's row t heads + j: the rows past T kv_heads are not its own
        kx = x[:, c.heads:].reshape(T * c.kv_heads, dh)
        idx = (np.arange(T)[:, None] * c.heads + np.arange(c.kv_heads)[None, :]).ravel()
        live = idx < T * c.kv_heads
    isq = (np.arange(nh) < c.heads)[None, :, None]
    g = np.where(isq, c.gq.astype(ft)[None, None, :], c.gk.astype(ft)[None, None, :])
    if mut == "gk_for_q":
        g = np.broadcast_to(c.gk.astype(ft)[None, None, :], x.shape)
    eps = np.where(isq, ft(c.eps_q), ft(c.eps_q if mut == "epsq_for_k" else c.eps_k))
    p = c.tpos[:T].astype(np.int64)
    ok = (p >= 0) & (p < c.max_pos)
    prow = np.where(ok, p, np.where(p < 0, (p % c.max_pos + c.max_pos - 1) % c.max_pos, (p + 1) % c.max_pos)) if mut == "pos_not_clamped" else np.where(ok, p, 0)
    cs, sn = c.cos[prow].astype(ft)[:, None, :], c.sin[prow].astype(ft)[:, None, :]
    if mut == "rot_sign":
        sn = -sn

    def rot(z):
        a, b = z[:, :, :half], z[:, :, half:]
        return np.concatenate([a * cs - b * sn, b * cs + a * sn], 2)

    def norm(z):
        ss = np.cumsum(z * z, axis=2, dtype=ft)[:, :, -1:] if ft == F32 else (z * z).sum(2, keepdims=True)
        return z * (ft(1.0) / np.sqrt(ss * ft(1.0 / dh) + eps)) * g
    out = norm(rot(x)) if mut == "rot_before_norm" else rot(norm(x))
    if mut == "partner_plain64":
        out = out[:, :, stored_order(dh)]
    q, k = out[:, :c.heads], out[:, c.heads:]
    if mut == "k_rows_by_heads":
        k2 = kx.copy()
        full = out[:, c.heads:].reshape(T * c.kv_heads, dh)      # what the norm makes of k's rows, each in place
        k2[idx[live]] = full[idx[live]]
        k = k2.reshape(T, c.kv_heads, dh)
    return q, k


def qk_expected(c, mut=None):
    q, k = qk_forward(c, F32, mut)
    return {"q": _store_heads(c, q), "k": _store_heads(c, k)}


def _store_heads(c, z):
    """natural-order fp32 [T, n, dh] -> the stored 16-bit rows [T, n dh]"""
    st = np.empty_like(z)
    st[:, :, stored_order(c.dh)] = z
    return bits16(to_hi(np.ascontiguousarray(st, F32), c.dtype), c.dtype).reshape(c.T, -1)


def natural_heads(c, rows, n):
    """stored rows [T, n dh] (any dtype) -> [T, n, dh] in natural feature order"""
    return np.asarray(rows).reshape(c.T, n, c.dh)[:, :, stored_order(c.dh)]


def qk_bound(c):
    """float64 reference (q, k) and the bound on |stored 16-bit value - reference|: 8 exact-operand squares and their sum per lane plus log2(dh / 8) butterfly
    adds (gamma_d, one rounding per square), the scaling by the power of two 1 / dh (exact), the add of eps, the reciprocal square root (HIP's rsqrtf: 1 ulp = 2
    half-ulps), two multiplies per element, then two products and one add of the rotation, then one rounding to the operand type"""
    q, k = qk_forward(c, F64)
    u, dh, half = U32, c.dh, c.dh // 2
    d_ = 8 + int(np.log2(dh // 8))
    gam = d_ * u / (1 - d_ * u)
    x = c.x[:c.T].astype(F64)
    isq = (np.arange(c.heads + c.kv_heads) < c.heads)[None, :, None]
    eps = np.where(isq, c.eps_q, c.eps_k)
    ss = (x * x).sum(2, keepdims=True)
    w = ss / dh + eps
    dw = (u + gam) * (1 + u) * ss / dh + u * w
    rel = 0.5 * (dw / w) / (1 - dw / w) ** 1.5 + 2 * u
    g = np.where(isq, c.gq.astype(F64)[None, None, :], c.gk.astype(F64)[None, None, :])
    n = np.abs(x / np.sqrt(w) * g)                                    # |normalised element|
    dn = n * (rel + 2 * u) * (1 + 4 * u)
    prow = np.where((c.tpos[:c.T] >= 0) & (c.tpos[:c.T] < c.max_pos), c.tpos[:c.T], 0)
    cs, sn = np.abs(c.cos[prow].astype(F64))[:, None, :], np.abs(c.sin[prow].astype(F64))[:, None, :]
    a, b, da, db = n[:, :, :half], n[:, :, half:], dn[:, :, :half], dn[:, :, half:]
    ref = np.concatenate([q, k], 1)
    mag = np.concatenate([a * cs + b * sn, b * cs + a * sn], 2)
    dr = np.concatenate([da * cs + db * sn, db * cs + da * sn], 2) + u * mag * (1 + 4 * u) + u * np.abs(ref)
    bound = bound16(ref, dr, c.dtype)
    return q, k, bound[:, :c.heads], bound[:, c.heads:]


# ---------------------------------------------------------------------------------------------------------
# k_rot_pos, k_gather_cls: integers and copies
# ---------------------------------------------------------------------------------------------------------
ROT_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 130)
ROT_LAYOUTS = ("right", "left", "holes", "cls_last")
INT_MUTANTS = ("first_row_only", "cls_under_last_row", "ctx_H_cols")


def make_rot_case(align, seed=0):
    """every length under every layout, packed with `align`; the alignment rows of tok_pos hold 777, the ints behind the last sequence are not the kernel's"""
    rng = np.random.default_rng(seed + align)
    c = Case()
    c.op, c.align = "rot_pos", align
    off, nq, cols, o = [], [], [], 0
    for layout in ROT_LAYOUTS:
        for n in ROT_LENGTHS:
            S = n + 9
            if layout == "right" or n == 0:
                col = np.arange(n)
            elif layout == "left":
                col = np.arange(S - n, S)
            elif layout == "holes":
                col = np.sort(rng.permutation(np.arange(2, S + n))[:n])
            else:                                  # the query-only CLS row of a masked column 0 sits last, with column 0
                col = np.concatenate([np.sort(rng.permutation(np.arange(3, S + n))[:n - 1]), [0]])
            padded = (n + align - 1) // align * align
            off.append(o); nq.append(n)
            cols.append(np.concatenate([col, np.full(padded - n, 777)]))
            o += padded
    c.seq_off, c.seq_nq = np.int32(off), np.int32(nq)
    c.total, c.capT = o, o + 5
    c.tok_pos = np.concatenate(cols + [np.full(5, 555)]).astype(np.int32)
    c.nseq = len(off)
    return c


def rot_expected(c, sentinel32, mut=None):
    out = np.full(c.capT, sentinel32, np.int32)
    for o, n in zip(c.seq_off, c.seq_nq):
        if n <= 0:
            continue
        first = c.tok_pos[o] if mut == "first_row_only" else min(c.tok_pos[o], c.tok_pos[o + n - 1])
        padded = (n + c.align - 1) // c.align * c.align
        out[o:o + padded] = 0
        out[o:o + n] = c.tok_pos[o:o + n] - first
    return out


def make_gather_case(H, Dq, last_row, has_lo, seed=0):
    rng = np.random.default_rng(seed + H + Dq)
    c = Case()
    c.op, c.H, c.Dq, c.last_row, c.has_lo = "gather", H, Dq, last_row, has_lo
    c.seq_off, c.seq_nk, c.seq_cls = np.int32([0, 8, 12, 20]), np.int32([5, 3, 0, 7]), np.int32([0, 2, 1, 6])      # one sequence without attended rows
    c.nseq, c.T, c.capT = 4, 4, 28
    c.ctx = rng.integers(0, 1 << 16, (c.capT, Dq), dtype=np.uint16)
    c.xb = rng.integers(0, 1 << 16, (c.capT, H), dtype=np.uint16)
    c.xlo = rng.integers(0, 256, (c.capT, H), dtype=np.uint8)
    return c


def gather_expected(c, sentinel, mut=None):
    src = c.seq_off + (np.where(c.seq_nk > 0, c.seq_nk - 1, 0) if (c.last_row and mut != "cls_under_last_row") else c.seq_cls)
    out = {"c_ctx": c.ctx[src].copy(), "c_xb": c.xb[src], "c_off": np.arange(c.nseq, dtype=np.int32), "c_nk": (c.seq_nk > 0).astype(np.int32),
           "c_cls": np.zeros(c.nseq, np.int32), "d_B": np.int32(c.nseq)}
    if mut == "ctx_H_cols":
        out["c_ctx"][:, c.H:] = sentinel
    if c.has_lo:
        out["c_xlo"] = c.xlo[src]
    return out


def int_applies(mut, c):
    return {"first_row_only": c.op == "rot_pos", "cls_under_last_row": c.op == "gather" and bool(c.last_row), "ctx_H_cols": c.op == "gather" and c.Dq != c.H}[mut]


# ---------------------------------------------------------------------------------------------------------
# the shapes of the GPU test, shared with the host test
# ---------------------------------------------------------------------------------------------------------
WIDTHS = (128, 384, 512, 640, 1024, 1152, 2048)      # NS = 1, 2, 4, each with a full and a partial last step; 1152 leaves step 3 of 4 empty
ROWS = (1, 4, 5, 9)                                   # 9 rows on one block: three passes of the stride loop, the last with one wave
GRIDS = (1, 2, 0)
EPS = (1e-12, 1e-5, 1e-6)
QK_SHAPES = ((4, 4), (4, 2), (6, 1))
QK_ROWS = (1, 3, 5)
GATHER_SHAPES = ((128, 128), (128, 256), (128, 4096), (2048, 2048), (2048, 4096))      # (H, Dq): Dq in {H, 2H, 4096 where that is >= H}


def norm_kinds(op, rms):
    if rms:                                            # (the mean set needs a subtracted mean)
        return ("signs", "fixed", "diffuse")
    return ("signs", "mean", "fixed", "diffuse") if op == "pre" else ("signs", "mean", "diffuse")


def check_norm_launch(c, grid=0, alias=0, outs=None):
    """what rows_probe.hip's check_args refuses, said on the host (None = accepted)"""
    if c.H < 128 or c.H % 128 or c.H > 2048:
        return "H"
    if c.T < 1 or c.T > c.capT:
        return "T"
    if grid < 0 or (c.op in ("post", "pre", "head") and grid > c.T):
        return "grid"
    if alias and c.op not in ("post", "pre"):
        return "alias"
    if c.op in ("embed_ln", "embed_rms"):
        ids = c.tok_id[:c.T]
        if (ids < 0).any() or (ids >= N_WORD).any():
            return "tok_id"
        if c.op == "embed_ln" and ((c.tok_pos[:c.T] < 0).any() or (c.tok_pos[:c.T] >= N_POS).any() or (c.tok_type[:c.T] < 0).any() or (c.tok_type[:c.T] >= N_TYPE).any()):
            return "tok_pos / tok_type"
    return None
