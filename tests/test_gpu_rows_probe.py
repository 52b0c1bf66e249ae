"""Every row kernel of kirag_amd/csrc/encoder_rows.hpp launched alone, through the library's own launchers, on operands the test controls
(tests/capi/rows_probe.hip, tests/rows_probe_util.py): the exact sets bit for bit against their one correct pattern — the device side of the low-byte codec
against its specification among them — the diffuse sets within the derived bound against float64, bit for bit across grids, aliases and absent outputs, and
every guard element and every row >= T still the sentinel after every launch.

The probe objects tests/capi/librows_probe_{bf16,f16}.so are built by kirag_amd/csrc/Makefile (__graft_entry__.build()); a missing object fails the tests.
Every tolerance is rows_probe_util's derived bound (norm_bound / qk_bound, bound16, bound_lo); tests/test_rows_probe_host.py shows on the CPU, on the same
cases, that the exact sets are exact and that every listed mutant of the kernels changes their bits or moves the diffuse reference by >= 10 bounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_probe_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ("f16", "bf16")
G = U.GUARD
F32, F64 = np.float32, np.float64
IN = ("y", "ybias", "g", "beta", "rb_in", "rlo_in", "word", "pos", "type", "tok_id", "tok_pos", "tok_type", "row_seq", "q_in", "k_in", "gk", "rot_cos", "rot_sin",
      "seq_off", "seq_a", "seq_nk")
OUT = ("xb", "xlo", "rb_out", "rlo_out", "q", "k", "i0", "i1", "i2", "err")
INTS = ("op", "H", "T", "capT", "grid", "alias", "rms", "sentinel", "n_word", "n_pos", "n_type", "heads", "kv_heads", "dh", "qw", "kw", "max_pos", "nseq", "align",
        "last_row")


class Args(C.Structure):      # RowsProbeArgs (tests/capi/rows_probe.hip)
    _fields_ = [(n, C.c_void_p) for n in IN + OUT] + [("eps", C.c_float), ("eps_k", C.c_float)] + [(n, C.c_int) for n in INTS]


_libs = {}


def probe(dtype):
    """the probe of one operand type, loaded the way kirag_amd/_lib.py loads the library: torch first (one HIP runtime per process), no fallback"""
    if dtype not in _libs:
        import torch  # noqa: F401
        path = os.path.join(HERE, "capi", "librows_probe_%s.so" % dtype)
        assert os.path.exists(path), path + " not found: build it with `make -C kirag_amd/csrc` (or __graft_entry__.build())"
        lib = C.CDLL(path)
        fn = getattr(lib, "kr_rows_probe_" + dtype)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(Args)]
        lib.kr_rows_probe_error.restype = C.c_char_p
        _libs[dtype] = (lib, fn)
    return _libs[dtype]


def sent32(dtype):
    s = U.SENTINEL[dtype]
    return np.uint32((s << 16) | s).astype(np.uint32).view(np.int32)


def call(dtype, op, ins, outs, eps=0.0, eps_k=0.0, **ints):
    """one call of the entry point: the return value; `outs` (name -> guarded host array) are filled by the probe"""
    lib, fn = probe(dtype)
    keep = {k: np.ascontiguousarray(v) for k, v in ins.items() if v is not None}
    a = Args()
    for n in IN:
        setattr(a, n, keep[n].ctypes.data if n in keep else None)
    for n in OUT:
        assert n not in outs or outs[n].flags["C_CONTIGUOUS"]
        setattr(a, n, outs[n].ctypes.data if n in outs else None)
    a.eps, a.eps_k, a.op, a.sentinel = eps, eps_k, U.OPS[op], U.SENTINEL[dtype]
    for n, v in ints.items():
        setattr(a, n, int(v))
    rc = fn(C.byref(a))
    if rc == -2:      # a HIP error: nothing more is launched on this device from this process
        pytest.exit("rows probe: %s" % lib.kr_rows_probe_error().decode(), returncode=3)
    return rc


def guards_hold(dtype, arr, live, what):
    """the guard rows and every row behind the `live` ones still hold the sentinel (16-bit arrays: the sentinel; bytes: its low byte; ints: both halves)"""
    s = U.SENTINEL[dtype]
    want = s & 0xff if arr.dtype == np.uint8 else s if arr.dtype == np.uint16 else sent32(dtype)
    assert (arr[:G] == want).all() and (arr[G + live:] == want).all(), ("written outside the live rows", what)
    return arr[G:G + live]


def norm_inputs(c, lo_in=True):
    ins = {"g": c.g, "beta": c.beta}
    if c.op in ("post", "pre"):
        ins.update(y=U.exact16(c.y, c.dtype), ybias=c.ybias, rb_in=U.exact16(c.r_hi, c.dtype), rlo_in=c.r_lo if (c.has_lo and lo_in) else None)
    elif c.op == "head":
        ins.update(y=U.exact16(c.y, c.dtype), row_seq=c.row_seq)
    else:
        ins.update(tok_id=c.tok_id, word=c.word)
        if c.op == "embed_ln":
            ins.update(tok_pos=c.tok_pos, tok_type=c.tok_type, pos=c.pos, type=c.type)
    return ins


def launch_norm(c, grid=0, alias=0, drop=()):
    """one launch of a norm-family case; `drop`: the outputs handed to the kernel as null pointers.  Returns name -> the T live rows (xb, xlo, rb, rlo; err)"""
    assert U.check_norm_launch(c, grid, alias) is None, U.check_norm_launch(c, grid, alias)
    rows = c.capT + 2 * G
    names = {"xb": ("xb", np.uint16), "xlo": ("xlo", np.uint8), "rb": ("rb_out", np.uint16), "rlo": ("rlo_out", np.uint8)}
    outs = {names[k][0]: np.zeros((rows, c.H), names[k][1]) for k in U.norm_keys(c) if k not in drop}
    if c.op == "head":
        outs["err"] = np.zeros(3, np.int32)
    what = (c.op, c.kind, c.dtype, c.H, c.T, grid, alias, drop)
    rc = call(c.dtype, c.op, norm_inputs(c), outs, eps=c.eps, H=c.H, T=c.T, capT=c.capT, grid=grid, alias=alias, rms=c.rms, n_word=U.N_WORD, n_pos=U.N_POS, n_type=U.N_TYPE)
    assert rc == 0, (rc, probe(c.dtype)[0].kr_rows_probe_error(), what)
    got = {k: guards_hold(c.dtype, outs[names[k][0]], c.T, what + (k,)) for k in names if names[k][0] in outs}
    if c.op == "head":
        assert outs["err"][0] == sent32(c.dtype) and outs["err"][2] == sent32(c.dtype), what
        got["err"] = int(outs["err"][1])
    return got


WORST = {}      # (kernel, dtype, quantity) -> (ratio, |out - ref|, bound, where)


def _within(key, got, ref, bound, where):
    err = np.abs(got.astype(F64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    i = int(np.argmax(ratio))
    if key not in WORST or ratio.flat[i] > WORST[key][0]:
        WORST[key] = (float(ratio.flat[i]), float(err.flat[i]), float(bound.flat[i]), str(where))
    assert np.isfinite(got).all() and (err <= bound).all(), (key, where, float(ratio.flat[i]), np.argwhere(err > bound)[:4].tolist())


def check_norm(c, got):
    """the exact keys bit for bit; every other output within the derived bound of the float64 reference: the 16-bit value, and the decoded hi + lo value"""
    want = U.norm_expected(c)
    where = (c.kind, c.H, c.T, c.eps)
    for k in want:
        if k in got:
            assert np.array_equal(got[k], want[k]), (c.op, c.dtype, where, k, "bits", int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:4].tolist())
    if c.kind in ("signs", "mean"):
        return
    o, v, do, dv = U.norm_bound(c)
    name = c.op + ("_rms" if c.rms and c.op == "pre" else "")
    if "xb" not in want:
        _within((name, c.dtype, "xb"), U.from16(got["xb"], c.dtype), o, U.bound16(o, do, c.dtype), where)
        if "xlo" in got:
            _within((name, c.dtype, "xb + xlo"), U.decoded(got["xb"], got["xlo"], c.dtype), o, U.bound_lo(do, got["xb"], got["xlo"], c.dtype), where)
    if "rb" in got and "rb" not in want:
        _within((name, c.dtype, "rb"), U.from16(got["rb"], c.dtype), v, U.bound16(v, dv, c.dtype), where)
        if "rlo" in got:
            _within((name, c.dtype, "rb + rlo"), U.decoded(got["rb"], got["rlo"], c.dtype), v, U.bound_lo(dv, got["rb"], got["rlo"], c.dtype), where)


def same(a, b, what, keys=None):
    for k in (keys or a):
        if k in b:
            assert np.array_equal(a[k], b[k]), (what, k, int(np.sum(a[k] != b[k])), np.argwhere(np.asarray(a[k] != b[k]))[:4].tolist())


@pytest.fixture(scope="module", autouse=True)
def report():
    """prints the worst measured error over its derived bound per kernel, type and quantity (KIRAG_AMD_ROWS_PROBE_REPORT: also into that file)"""
    yield
    lines = ["kernel      type  quantity     measured |out - ref|   derived bound   ratio   at"]
    for (kern, dtype, q), (ratio, err, bound, where) in sorted(WORST.items()):
        lines.append("%-11s %-5s %-12s %.6e           %.6e    %.3f   %s" % (kern, dtype, q, err, bound, ratio, where))
    print("\n" + "\n".join(lines))
    path = os.environ.get("KIRAG_AMD_ROWS_PROBE_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


NORM_OPS = (("post", False), ("pre", False), ("pre", True), ("head", False))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op,rms", NORM_OPS, ids=lambda x: x if isinstance(x, str) else "rms" if x else "ln")
def test_norms_at_every_width_row_count_and_grid(op, rms, dtype):
    """k_ln16 / k_ln16_pre (LayerNorm and RMS) / k_ln16_head: every width (NS = 1, 2, 4 with full, partial and empty steps) x every data set x T in 1, 4, 5, 9 on
    the library's grid against the reference, and on 1 and 2 blocks (9 rows on one block: three passes of the stride loop, the last with one wave) bit for bit
    against it; every row written exactly once (the rows >= T and the guards keep the sentinel)"""
    for H in U.WIDTHS:
        for kind in U.norm_kinds(op, rms):
            if op == "head" and kind == "fixed":
                continue
            for T in U.ROWS:
                c = U.make_norm_case(op, kind, dtype, H, T, rms=rms, eps=U.EPS[(H // 128 + T) % 3], seed=3)
                base = launch_norm(c)
                check_norm(c, base)
                for grid in U.GRIDS[:2]:
                    if grid <= T:
                        same(base, launch_norm(c, grid=grid), (op, kind, H, T, "grid", grid))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["embed_ln", "embed_rms"])
def test_embeddings(op, dtype):
    """k_embed_ln / k_embed_rms: repeated ids, the last row of every table, one and five rows, the low half present and absent"""
    for H in U.WIDTHS:
        for kind in U.norm_kinds(op, op == "embed_rms"):
            for T in (1, 5):
                c = U.make_norm_case(op, kind, dtype, H, T, rms=op == "embed_rms", eps=U.EPS[(H // 128 + T) % 3], seed=3)
                base = launch_norm(c)
                check_norm(c, base)
                lo = "xlo" if op == "embed_ln" else "rlo"
                bare = launch_norm(c, drop=(lo,))
                assert lo not in bare
                same(base, bare, (op, kind, H, T, "without", lo))
                if T == 5:      # a grid as a forward launches it for more rows than are live: the waves past T return
                    same(base, launch_norm(c, grid=2), (op, kind, H, T, "grid 2"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_low_half_present_and_absent(dtype):
    """xlo_in / rlo_in null decodes as byte 128; xlo, rb_out, rlo_out null: the other outputs keep their bits"""
    for H in (128, 640, 1152, 2048):
        for kind in ("signs", "diffuse"):
            for op, rms in (("post", False), ("pre", False), ("pre", True)):
                c = U.make_norm_case(op, kind, dtype, H, 5, rms=rms, seed=5)
                base = launch_norm(c)
                for drop in (("xlo",),) if op == "post" else (("xlo",), ("rlo",), ("rb", "rlo"), ("xlo", "rb", "rlo")):
                    got = launch_norm(c, drop=drop)
                    assert not set(drop) & set(got)
                    same(base, got, (op, kind, H, "without", drop))
                # no low half on input: the kernel has to decode byte 128 (the signs set is then built without a part in the bytes, and stays exact)
                n = U.make_norm_case(op, kind, dtype, H, 5, rms=rms, seed=5, has_lo=False)
                check_norm(n, launch_norm(n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_aliases_of_a_forward_change_no_bit(dtype):
    """k_ln16_pre with rb_in == xb (layer 0 of a ModernBert handle), rb_in == rb_out and rlo_in == rlo_out (every later layer), k_ln16 with xlo_in == xlo: a wave
    reads its whole row before it stores it — on one block with three passes and on the library's grid, the result is the unaliased launch's bit for bit"""
    for H in (128, 640, 2048):
        for kind in ("signs", "fixed", "diffuse"):
            for rms in (False, True):
                c = U.make_norm_case("pre", kind, dtype, H, 9, rms=rms, seed=6)
                for grid in (1, 0):
                    base = launch_norm(c, grid=grid)
                    if grid == 0:
                        check_norm(c, base)
                    for alias in (U.ALIAS_RB_XB, U.ALIAS_RB, U.ALIAS_LO, U.ALIAS_RB | U.ALIAS_LO, U.ALIAS_RB_XB | U.ALIAS_LO):
                        same(base, launch_norm(c, grid=grid, alias=alias), ("pre", kind, H, rms, grid, "alias", alias))
            if kind != "fixed":
                c = U.make_norm_case("post", kind, dtype, H, 9, seed=6)
                for grid in (1, 0):
                    same(launch_norm(c, grid=grid), launch_norm(c, grid=grid, alias=U.ALIAS_LO), ("post", kind, H, grid, "xlo_in == xlo"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["+inf", "-inf", "nan"])
def test_pre_ln_keeps_a_non_finite_residual(what, dtype):
    """KEEP_INF: one residual element hi = +-inf (with the byte 0 an overflow is stored with) or NaN: that row of xb is all NaN, the stored residual keeps the
    element, every other row keeps its bits"""
    for rms in (False, True):
        c0 = U.make_norm_case("pre", "diffuse", dtype, 640, 4, rms=rms, seed=2)
        base = launch_norm(c0)
        c = U.keep_inf_case(c0, what)
        t, i = c.planted
        got = launch_norm(c)
        # LayerNorm: inf - mean is NaN, the whole row is.  RMS of an infinite element: rstd = 0, the finite elements become 0 and the element itself 0 x inf
        # = NaN; a NaN element makes every sum NaN under both
        model = np.isnan(U.norm_forward(c, F32, "lane")[0][t])
        assert model[i] and (model.all() or (rms and what != "nan"))
        assert np.array_equal(np.isnan(U.from16(got["xb"], dtype)[t]), model), (what, rms, "the row normalised")
        r = U.from16(got["rb"], dtype)[t, i]
        assert (np.isnan(r) if what == "nan" else np.isinf(r) and (r > 0) == (what == "+inf")), (what, rms, float(r))
        keep = np.arange(c.T) != t
        for k in base:
            assert np.array_equal(got[k][keep], base[k][keep]), (what, rms, k)
        rest = np.arange(c.H) != i
        assert np.array_equal(got["rb"][t, rest], base["rb"][t, rest]) and np.array_equal(got["rlo"][t, rest], base["rlo"][t, rest])


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_norm_raises_the_error_word_for_rows_of_a_sequence_only(dtype):
    for H in (128, 1152):
        c = U.make_norm_case("head", "diffuse", dtype, H, 9, seed=7)
        assert (c.row_seq[:c.T] >= 0).any() and (c.row_seq[:c.T] < 0).any()
        base = launch_norm(c)
        assert base["err"] == 0
        for val in (np.inf, -np.inf, np.nan):
            for t in range(c.T):
                d = U.Case()
                d.__dict__.update(c.__dict__)
                d.y = c.y.copy()
                d.y[t, (37 * t + 11) % H] = val
                got = launch_norm(d, grid=1 if t % 2 else 0)
                assert got["err"] == (2 if c.row_seq[t] >= 0 else 0), (H, val, t, int(c.row_seq[t]), got["err"])
                keep = np.arange(c.T) != t
                assert np.array_equal(got["xb"][keep], base["xb"][keep])


def launch_qk(c, grid=0):
    q_in, k_in = U.qk_arrays(c)
    rows = c.capT + 2 * G
    qw, kw = c.heads * c.dh, c.kv_heads * c.dh
    outs = {"q": np.zeros((rows, qw), np.uint16), "k": np.zeros((rows, kw), np.uint16)}
    what = ("qk", c.kind, c.dtype, c.dh, c.heads, c.kv_heads, c.T, grid)
    rc = call(c.dtype, "qk", dict(q_in=U.exact16(q_in, c.dtype), k_in=U.exact16(k_in, c.dtype), g=c.gq, gk=c.gk, rot_cos=c.cos, rot_sin=c.sin, tok_pos=c.tpos), outs,
              eps=c.eps_q, eps_k=c.eps_k, T=c.T, capT=c.capT, grid=grid, heads=c.heads, kv_heads=c.kv_heads, dh=c.dh, qw=qw, kw=kw, max_pos=c.max_pos)
    assert rc == 0, (rc, probe(c.dtype)[0].kr_rows_probe_error(), what)
    return {k: guards_hold(c.dtype, outs[k], c.T, what + (k,)) for k in outs}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [32, 64, 128])
def test_qk_norm_rope(dh, dtype):
    """k_qk_norm_rope: the exact set bit for bit (every output names its feature, its side and its table row; positions -1 and max_pos behave as 0), the diffuse
    set (eps_q != eps_k, real tables) within the bound; grouped kv_heads; unit counts that fill no wave and no block; rows past T keep the sentinel in q and k"""
    for heads, kv in U.QK_SHAPES:
        for T in U.QK_ROWS:
            c = U.make_qk_case("exact", dtype, dh, heads, kv, T)
            got = launch_qk(c)
            want = U.qk_expected(c)
            for k in want:
                assert np.array_equal(got[k], want[k]), (dh, heads, kv, T, k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:4].tolist())
            d = U.make_qk_case("diffuse", dtype, dh, heads, kv, T)
            got = launch_qk(d)
            q, k, bq, bk = U.qk_bound(d)
            _within(("qk_norm_rope", dtype, "q"), U.natural_heads(d, U.from16(got["q"], dtype), heads), q, bq, (dh, heads, kv, T))
            _within(("qk_norm_rope", dtype, "k"), U.natural_heads(d, U.from16(got["k"], dtype), kv), k, bk, (dh, heads, kv, T))
            per_block = 4 * (64 // (dh // 8))      # the grid of a forward is sized by the padded row count: blocks without a live unit
            wide = (d.capT * (heads + kv) + per_block - 1) // per_block
            same(got, launch_qk(d, grid=wide), (dh, heads, kv, T, "grid", wide))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("align", [4, 8])
def test_rot_pos(align, dtype):
    """k_rot_pos: lengths 0 .. 130 under right and left padding, a mask with holes and the query-only CLS row last with column 0; the alignment rows get 0,
    the ints behind the last sequence keep the sentinel"""
    c = U.make_rot_case(align)
    out = np.zeros(c.capT + 2 * G, np.int32)
    rc = call(dtype, "rot_pos", dict(seq_off=c.seq_off, seq_a=c.seq_nq, tok_pos=c.tok_pos), {"i0": out}, T=c.total, capT=c.capT, nseq=c.nseq, align=align)
    assert rc == 0, probe(dtype)[0].kr_rows_probe_error()
    assert (out[:G] == sent32(dtype)).all() and (out[G + c.capT:] == sent32(dtype)).all()
    want = U.rot_expected(c, sent32(dtype))
    assert np.array_equal(out[G:G + c.capT], want), np.argwhere(out[G:G + c.capT] != want)[:6].tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_cls(dtype):
    """k_gather_cls: the CLS row or the last packed row of every sequence (one without attended rows), Dq = H, 2 H and 4096, xlo null and not; the compact
    tables and the row count"""
    s16, s32 = U.SENTINEL[dtype], sent32(dtype)
    for H, Dq in U.GATHER_SHAPES:
        for last_row in (0, 1):
            for has_lo in (True, False):
                c = U.make_gather_case(H, Dq, last_row, has_lo)
                rows = c.capT + 2 * G
                outs = {"q": np.zeros((rows, Dq), np.uint16), "xb": np.zeros((rows, H), np.uint16), "i0": np.zeros(rows, np.int32), "i1": np.zeros(rows, np.int32),
                        "i2": np.zeros(rows, np.int32), "err": np.zeros(3, np.int32)}
                if has_lo:
                    outs["xlo"] = np.zeros((rows, H), np.uint8)
                what = ("gather", H, Dq, last_row, has_lo)
                rc = call(dtype, "gather", dict(q_in=c.ctx, rb_in=c.xb, rlo_in=c.xlo if has_lo else None, seq_off=c.seq_off, seq_a=c.seq_cls, seq_nk=c.seq_nk), outs,
                          H=H, T=c.T, capT=c.capT, qw=Dq, nseq=c.nseq, last_row=last_row)
                assert rc == 0, (probe(dtype)[0].kr_rows_probe_error(), what)
                want = U.gather_expected(c, s16)
                got = {"c_ctx": "q", "c_xb": "xb", "c_xlo": "xlo", "c_off": "i0", "c_nk": "i1", "c_cls": "i2"}
                for k, name in got.items():
                    if name in outs:
                        assert np.array_equal(guards_hold(dtype, outs[name], c.nseq, what + (k,)), want[k]), what + (k,)
                assert outs["err"].tolist() == [int(s32), c.nseq, int(s32)], what


def test_probe_refuses_what_could_read_or_write_out_of_range():
    """the entry point checks its arguments before anything reaches the GPU"""
    dtype = "f16"
    c = U.make_norm_case("pre", "signs", dtype, 384, 5)
    rows = c.capT + 2 * G
    full = lambda H=384: {n: np.zeros((rows, H), t) for n, t in (("xb", np.uint16), ("xlo", np.uint8), ("rb_out", np.uint16), ("rlo_out", np.uint8))}
    base = dict(eps=0.0, H=c.H, T=c.T, capT=c.capT, grid=0, alias=0, rms=0)
    assert call(dtype, "pre", norm_inputs(c), full(), **base) == 0
    refused = []
    for change in (dict(H=192), dict(H=4096), dict(H=0), dict(T=c.capT + 1), dict(T=0), dict(grid=-1), dict(grid=c.T + 1), dict(alias=3), dict(alias=8)):
        refused.append(("pre", norm_inputs(c), full(), {**base, **change}))
    no_rb = full()
    del no_rb["rb_out"]
    refused.append(("pre", norm_inputs(c), no_rb, {**base, "alias": U.ALIAS_RB}))
    refused.append(("pre", norm_inputs(c, lo_in=False), full(), {**base, "alias": U.ALIAS_LO}))
    refused.append(("post", norm_inputs(c), full(), {**base, "alias": U.ALIAS_RB}))
    e = U.make_norm_case("embed_ln", "signs", dtype, 128, 5)
    eb = dict(eps=0.0, H=128, T=5, capT=e.capT, n_word=U.N_WORD, n_pos=U.N_POS, n_type=U.N_TYPE)
    eo = lambda: {"xb": np.zeros((e.capT + 2 * G, 128), np.uint16)}
    assert call(dtype, "embed_ln", norm_inputs(e), eo(), **eb) == 0
    for field, bad in (("tok_id", U.N_WORD), ("tok_id", -1), ("tok_pos", U.N_POS), ("tok_type", U.N_TYPE), ("tok_type", -1)):
        ins = norm_inputs(e)
        ins[field] = ins[field].copy()
        ins[field][3] = bad
        refused.append(("embed_ln", ins, eo(), eb))
    refused.append(("embed_ln", norm_inputs(e), eo(), {**eb, "grid": 1}))
    refused.append(("embed_ln", norm_inputs(e), eo(), {**eb, "alias": 1}))
    q = U.make_qk_case("exact", dtype, 64, 4, 2, 3)
    q_in, k_in = U.qk_arrays(q)
    qi = dict(q_in=U.bits16(q_in, dtype), k_in=U.bits16(k_in, dtype), g=q.gq, gk=q.gk, rot_cos=q.cos, rot_sin=q.sin, tok_pos=q.tpos)
    qo = lambda: {"q": np.zeros((q.capT + 2 * G, 256), np.uint16), "k": np.zeros((q.capT + 2 * G, 128), np.uint16)}
    qb = dict(T=3, capT=q.capT, heads=4, kv_heads=2, dh=64, qw=256, kw=128, max_pos=q.max_pos)
    assert call(dtype, "qk", qi, qo(), **qb) == 0
    for change in (dict(dh=48), dict(kv_heads=3, kw=192), dict(qw=320), dict(kw=256), dict(heads=0, qw=0), dict(max_pos=0), dict(grid=1000), dict(T=q.capT + 1)):
        refused.append(("qk", qi, qo(), {**qb, **change}))
    r = U.make_rot_case(4)
    ri = dict(seq_off=r.seq_off, seq_a=r.seq_nq, tok_pos=r.tok_pos)
    rb = dict(T=r.total, capT=r.capT, nseq=r.nseq, align=4)
    far = r.seq_off.copy()
    far[-1] = r.capT - 2      # the last sequence (130 rows) would end past capT
    refused.append(("rot_pos", {**ri, "seq_off": far}, {"i0": np.zeros(r.capT + 2 * G, np.int32)}, rb))
    refused.append(("rot_pos", ri, {"i0": np.zeros(r.capT + 2 * G, np.int32)}, {**rb, "align": 6}))
    g = U.make_gather_case(128, 256, 0, True)
    go = lambda: {"q": np.zeros((g.capT + 2 * G, 256), np.uint16), "xb": np.zeros((g.capT + 2 * G, 128), np.uint16), "xlo": np.zeros((g.capT + 2 * G, 128), np.uint8),
                  "i0": np.zeros(g.capT + 2 * G, np.int32), "i1": np.zeros(g.capT + 2 * G, np.int32), "i2": np.zeros(g.capT + 2 * G, np.int32), "err": np.zeros(3, np.int32)}
    gi = dict(q_in=g.ctx, rb_in=g.xb, rlo_in=g.xlo, seq_off=g.seq_off, seq_a=g.seq_cls, seq_nk=g.seq_nk)
    gb = dict(H=128, T=g.T, capT=g.capT, qw=256, nseq=g.nseq, last_row=0)
    assert call(dtype, "gather", gi, go(), **gb) == 0
    bad_cls = g.seq_cls.copy()
    bad_cls[3] = 8      # row 28 of 28
    refused.append(("gather", {**gi, "seq_a": bad_cls}, go(), gb))
    refused.append(("gather", gi, go(), {**gb, "qw": 100}))
    refused.append(("gather", gi, go(), {**gb, "nseq": 3}))
    for op, ins, outs, kw in refused:
        rc = call(dtype, op, ins, outs, **kw)
        assert rc == -1 and probe(dtype)[0].kr_rows_probe_error(), (rc, op, kw)
