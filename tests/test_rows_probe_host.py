"""The inputs of the row-kernel probe have teeth (tests/rows_probe_util.py) — checked on numpy models alone, no GPU, on the SAME cases
tests/test_gpu_rows_probe.py launches:
  - every construction of the exact set is exact: the kernel's arithmetic evaluated in fp32 in three summation orders (left to right, right to left, Ln16's
    lane order) and in float64 gives identical bits, so each output element has one correct pattern;
  - every listed mutant of the kernels changes at least one expected bit of the exact set, and moves the diffuse set's reference by >= 10 derived bounds on at
    least one element — or is invisible to one set BY CONSTRUCTION, in which case *_applies says so and the other set catches it;
  - the fp32 model itself stays within the derived bound of the float64 reference (the bound is not too tight for a correct kernel)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_probe_util as U  # noqa: E402

MOVE = 10.0          # x the derived bound: the ratio tests/test_proj_probe_host.py uses
DTYPES = ("f16", "bf16")
NORM_OPS = (("post", False), ("pre", False), ("pre", True), ("head", False), ("embed_ln", False), ("embed_rms", True))
F32, F64 = np.float32, np.float64


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _cases(op, rms, dtype, widths=U.WIDTHS, T=5):
    for H in widths:
        for kind in U.norm_kinds(op, rms):
            if op == "head" and kind == "fixed":
                continue
            yield U.make_norm_case(op, kind, dtype, H, T, rms=rms, eps=U.EPS[(H // 128) % 3], seed=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op,rms", NORM_OPS)
def test_exact_constructions_are_exact_in_every_order(op, rms, dtype):
    n = 0
    for c in _cases(op, rms, dtype):
        if c.kind == "diffuse":
            continue
        runs = [U.norm_forward(c, F32, order) for order in ("seq", "rev", "lane")]
        o64, v64 = U.norm_forward(c, F64)
        if c.kind == "fixed":      # only the residual sum is exact: v = decode(r), or the embedding row itself
            for o, v in runs:
                assert np.array_equal(_bits(v), _bits(v64)) and np.array_equal(v64.astype(F32).astype(F64), v64), (op, c.H)
            if op == "pre":        # and the stored pair is the input pair, for every byte value and both signs
                out = U.norm_outputs(c, *runs[0])
                assert np.array_equal(out["rb"], U.bits16(c.r_hi[:c.T], dtype)) and np.array_equal(out["rlo"], c.r_lo[:c.T]), (op, c.H)
                assert len(np.unique(c.r_lo[:c.T])) == 256 and (c.r_hi[:c.T] > 0).any() and (c.r_hi[:c.T] < 0).any()
            n += 1
            continue
        assert np.array_equal(o64.astype(F32).astype(F64), o64) and np.array_equal(v64.astype(F32).astype(F64), v64), (op, c.kind, c.H, "float64 result is no fp32 number")
        for o, v in runs:
            assert np.array_equal(_bits(o), _bits(o64)) and np.array_equal(_bits(v), _bits(v64)), (op, c.kind, c.H)
        s = np.sign(v64)
        if c.kind == "signs":
            assert set(np.unique(v64)) == {-1.0, 1.0} and np.array_equal(o64, s * c.g.astype(F64)[None, :]), (op, c.H)      # the output row IS +-g
            if not rms:
                assert (v64.sum(1) == 0).all()
        else:
            assert (np.abs(v64 - v64.mean(1, keepdims=True)) == 0.5).all() and (v64.mean(1) != 0).all()
            assert np.array_equal(o64, np.sign(v64 - v64.mean(1, keepdims=True)) * c.g.astype(F64)[None, :] + c.beta.astype(F64)[None, :]), (op, c.H)
        n += 1
    assert n >= len(U.WIDTHS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_signs_set_sweeps_the_codec(dtype):
    """the g of the signs set reaches every region of the codec the specification names, and the expected bytes come from the specification alone"""
    g = U.codec_sweep(2048, dtype, 5)
    hb, byte = U.codec(g, dtype)
    hi = U.from16(hb, dtype)
    assert (byte == 255).any() and (byte == 0).any() and (byte == 128).any() and len(np.unique(byte)) > 200
    assert (g < 2.0 ** -25).any()
    if dtype == "f16":
        assert (hi == 0).any() and (g[hi == 0] < 2.0 ** -25 * 1.0001).all()                                      # |x| < 2^-25: hi = 0
        assert np.isinf(hi).any() and (byte[np.isinf(hi)] == 0).all() and ((hi > 0) & (hi < 6.1e-5)).any()      # beyond 65504; the subnormal range
    c = U.make_norm_case("post", "signs", dtype, 2048, 4, seed=3)
    exp = U.norm_expected(c)
    o, _ = U.norm_forward(c, F64)
    want_hb, want_lo = U.codec(o.astype(F32), dtype)
    assert np.array_equal(exp["xb"], want_hb) and np.array_equal(exp["xlo"], want_lo)


def _stored(c, o, v, mut):
    """the compared quantities of the diffuse set as numbers: the normalised row, the stored residual"""
    out = {"o": np.asarray(o, F64)}
    if c.op in ("pre", "embed_rms"):
        vs = o if mut == "res_after_norm" else v
        out["v"] = U.to_hi(np.ascontiguousarray(vs, F32), c.dtype).astype(F64) if mut == "res_no_lo" else np.asarray(vs, F64)
    return out


def _norm_moves(c, mut):
    o, v, do, dv = U.norm_bound(c)
    hb, byte = U.codec(o.astype(F32), c.dtype)
    bounds = {"o": U.bound_lo(do, hb, byte, c.dtype) if c.op != "embed_rms" and c.op != "head" else U.bound16(o, do, c.dtype)}
    if c.op in ("pre", "embed_rms"):
        vb, vbyte = U.codec(v.astype(F32), c.dtype)
        bounds["v"] = U.bound_lo(dv, vb, vbyte, c.dtype)
    ref, alt = _stored(c, o, v, None), _stored(c, *U.norm_forward(c, F64, mut=mut), mut)
    with np.errstate(invalid="ignore"):
        return max(float(np.nanmax(np.abs(alt[k] - ref[k]) / bounds[k])) for k in ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op,rms", NORM_OPS)
def test_every_norm_mutant_is_seen(op, rms, dtype):
    seen = {m: 0 for m in U.NORM_MUTANTS}
    for c in _cases(op, rms, dtype, widths=(128, 640, 1152, 2048)):
        ref = U.norm_expected(c)
        for m in U.NORM_MUTANTS:
            if not U.norm_applies(m, c):
                continue
            seen[m] += 1
            alt = U.norm_expected(c, m)
            changed = any(not np.array_equal(ref[k], alt[k]) for k in ref)
            if c.kind in ("signs", "mean"):
                assert changed, (op, c.kind, c.H, m)
            elif not changed:      # fixed / diffuse: what is compared within the bound has to move by 10 bounds
                moved = _norm_moves(c, m)
                assert moved >= MOVE, (op, c.kind, c.H, m, moved)
    want = {"post": ("lo_ignored", "lo_pair_swapped", "lo_word0", "lo_step_dropped", "no_ybias", "no_beta", "no_eps", "padded_mean"),
            "pre": ("res_after_norm", "res_no_lo", "lo_ignored") + (("rms_subtracts_mean", "rms_reads_beta") if rms else ("no_beta",)),
            "head": ("no_beta", "padded_mean", "no_eps"), "embed_ln": ("pos_at_id", "type_at_0", "no_beta", "padded_mean"),
            "embed_rms": ("rms_subtracts_mean", "rms_reads_beta", "res_after_norm", "res_no_lo")}[op]
    for m in want:
        assert seen[m] >= 2, (op, m)


@pytest.mark.parametrize("dtype", DTYPES)
def test_diffuse_mutants_move_the_reference_too(dtype):
    """on the diffuse set ALONE every mutant that acts on it moves a compared quantity by >= 10 bounds (the exact set is not needed to see it)"""
    for op, rms in NORM_OPS:
        for H in (384, 2048):
            c = U.make_norm_case(op, "diffuse", dtype, H, 5, rms=rms, eps=1e-5, seed=4)
            for m in U.NORM_MUTANTS:
                if U.norm_applies(m, c):
                    moved = _norm_moves(c, m)
                    assert moved >= MOVE, (op, H, m, moved)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_model_stays_within_the_derived_bound(dtype):
    """a correct kernel passes: the fp32 evaluation in the kernel's own summation order, stored through the codec, lies within the bound of every comparison"""
    for op, rms in NORM_OPS:
        for H in U.WIDTHS:
            for eps in U.EPS:
                c = U.make_norm_case(op, "diffuse", dtype, H, 5, rms=rms, eps=eps, seed=4)
                o, v, do, dv = U.norm_bound(c)
                o32, v32 = U.norm_forward(c, F32, "lane")
                assert (np.abs(o32 - o) <= do).all() and (np.abs(v32 - v) <= dv).all(), (op, H, eps, float((np.abs(o32 - o) / do).max()))
                out = U.norm_outputs(c, o32, v32)
                assert (np.abs(U.from16(out["xb"], dtype) - o) <= U.bound16(o, do, dtype)).all()
                assert (np.abs(U.decoded(out["xb"], out["xlo"], dtype) - o) <= U.bound_lo(do, out["xb"], out["xlo"], dtype)).all()
                if "rb" in out:
                    assert (np.abs(U.decoded(out["rb"], out["rlo"], dtype) - v) <= U.bound_lo(dv, out["rb"], out["rlo"], dtype)).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["+inf", "-inf", "nan"])
def test_keep_inf_is_seen(what, dtype):
    """a non-finite pre-LN residual element (hi = inf with the byte 0 an overflow is stored with) keeps the row non-finite; decoded on the bit patterns alone
    (KEEP_INF off) it would be a finite 3.4e38 and the row would normalise"""
    c = U.keep_inf_case(U.make_norm_case("pre", "diffuse", dtype, 640, 4, seed=2), what)
    t, i = c.planted
    o, v = U.norm_forward(c, F32, "lane")
    out = U.norm_outputs(c, o, v)
    assert np.isnan(o[t]).all() and not np.isfinite(v[t, i]) and np.isfinite(np.delete(v[t], i)).all() and np.isfinite(np.delete(o, t, 0)).all()
    assert not np.isfinite(U.from16(out["rb"], dtype)[t, i])
    o2, v2 = U.norm_forward(c, F32, "lane", mut="keep_inf_off")
    if what != "nan":
        assert np.isfinite(v2[t, i]) and abs(v2[t, i]) > 3e38 and not np.isnan(o2[t]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [32, 64, 128])
def test_qk_exact_set_and_mutants(dh, dtype):
    seen = {m: 0 for m in U.QK_MUTANTS}
    for heads, kv in U.QK_SHAPES:
        for T in U.QK_ROWS:
            c = U.make_qk_case("exact", dtype, dh, heads, kv, T)
            q32, k32 = U.qk_forward(c, F32)
            q64, k64 = U.qk_forward(c, F64)
            assert np.array_equal(_bits(q32), _bits(q64)) and np.array_equal(_bits(k32), _bits(k64))
            for z, g in ((q64, c.gq), (k64, c.gk)):      # every output is +-g of one feature of its own side, exact in the operand type
                assert np.isin(np.abs(z), np.abs(g.astype(F64))).all()
                assert np.array_equal(U.from16(U.bits16(z.astype(F32), dtype), dtype).astype(F64), z)
            assert not np.isin(np.abs(c.gq), np.abs(c.gk)).any() and len(np.unique(np.abs(c.gq))) == dh and len(np.unique(np.abs(c.gk))) == dh
            ref = U.qk_expected(c)
            d = U.make_qk_case("diffuse", dtype, dh, heads, kv, T)
            qd, kd, bq, bk = U.qk_bound(d)
            q3, k3 = U.qk_forward(d, F32)
            assert (np.abs(U.to_hi(q3, dtype) - qd) <= bq).all() and (np.abs(U.to_hi(k3, dtype) - kd) <= bk).all()      # a correct kernel passes
            for m in U.QK_MUTANTS:
                if U.qk_applies(m, c):
                    alt = U.qk_expected(c, m)
                    assert any(not np.array_equal(ref[x], alt[x]) for x in ref), (dh, heads, kv, T, m)
                    seen[m] += 1
                if U.qk_applies(m, d):
                    qa, ka = U.qk_forward(d, F64, m)
                    with np.errstate(invalid="ignore"):
                        moved = max(float((np.abs(qa - qd) / bq).max()), float((np.abs(ka - kd) / bk).max()))
                    assert moved >= MOVE, (dh, heads, kv, T, m, moved)
                    seen[m] += 1
    for m in U.QK_MUTANTS:
        assert seen[m] >= 2 or (m == "partner_plain64" and dh != 64), m


def test_integer_kernels_and_their_mutants():
    sent = 0x7F7F7F7F
    for align in (4, 8):
        c = U.make_rot_case(align)
        ref = U.rot_expected(c, sent)
        assert sorted(set(c.seq_nq.tolist())) == sorted(U.ROT_LENGTHS) and (ref[c.total:] == sent).all() and (ref[:c.total] != sent).all()
        assert (ref[:c.total] >= 0).all() and U.int_applies("first_row_only", c) and not np.array_equal(ref, U.rot_expected(c, sent, "first_row_only"))
        for o, n in zip(c.seq_off, c.seq_nq):
            assert o % align == 0 and (n == 0 or ref[o:o + n].min() == 0) and (ref[o + n:o + (n + align - 1) // align * align] == 0).all()
    seen = set()
    for H, Dq in U.GATHER_SHAPES:
        for last_row in (0, 1):
            c = U.make_gather_case(H, Dq, last_row, True)
            ref = U.gather_expected(c, 0x7F7F)
            assert (c.seq_nk == 0).any() and ref["c_nk"].tolist() == [1, 1, 0, 1]
            for m in U.INT_MUTANTS[1:]:
                if U.int_applies(m, c):
                    alt = U.gather_expected(c, 0x7F7F, m)
                    assert any(not np.array_equal(ref[k], alt[k]) for k in ref), (H, Dq, last_row, m)
                    seen.add(m)
    assert seen == set(U.INT_MUTANTS[1:])


def test_check_norm_launch_mirrors_the_probe():
    c = U.make_norm_case("pre", "signs", "f16", 384, 5)
    assert U.check_norm_launch(c) is None and U.check_norm_launch(c, grid=2, alias=U.ALIAS_RB) is None
    assert U.check_norm_launch(c, grid=6) and U.check_norm_launch(c, grid=-1)
    for field, bad in (("H", 192), ("H", 4096), ("T", 0), ("T", c.capT + 1)):
        d = U.Case()
        d.__dict__.update(c.__dict__)
        setattr(d, field, bad)
        assert U.check_norm_launch(d), field
    e = U.make_norm_case("embed_ln", "signs", "f16", 128, 5)
    assert U.check_norm_launch(e) is None and U.check_norm_launch(e, alias=1)
    e.tok_id = e.tok_id.copy()
    e.tok_id[2] = U.N_WORD
    assert U.check_norm_launch(e)
