"""Every projection epilogue on every main loop, launched alone on operands the test controls (tests/capi/proj_probe.hip, tests/proj_probe_util.py): bit for bit
against the one correct pattern of the exact set, within the derived bound against float64 on the diffuse set, and bit for bit across loops, grids and knobs.

The probe objects tests/capi/libproj_probe_{bf16,f16}.so are built by kirag_amd/csrc/Makefile (__graft_entry__.build()); a missing object fails the tests.
The bound of every comparison is proj_probe_util.error_bound, derived there from the kernels' rounding points; tests/test_proj_probe_host.py shows on the CPU,
on the same cases, that every listed mutant of the kernels changes the exact set's bits and moves the diffuse reference by >= 10 bounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_probe_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ("f16", "bf16")


class Args(C.Structure):      # ProjProbeArgs (tests/capi/proj_probe.hip)
    _fields_ = [(n, C.c_void_p) for n in ("X", "W", "bias", "out0", "out1", "outT", "rot_cos", "rot_sin", "tpos", "row_seq", "smax")] + \
               [("capT", C.c_int64), ("ldT", C.c_int64)] + \
               [(n, C.c_int) for n in ("T", "F", "K", "H", "A", "max_pos", "dh", "nseq", "V", "epi", "loop", "blocks", "nt", "ant", "epi_prio", "pw", "sentinel")]


_libs = {}


def probe(dtype):
    """the probe of one operand type, loaded the way kirag_amd/_lib.py loads the library: torch first (one HIP runtime per process), no fallback"""
    if dtype not in _libs:
        import torch  # noqa: F401
        path = os.path.join(HERE, "capi", "libproj_probe_%s.so" % dtype)
        assert os.path.exists(path), path + " not found: build it with `make -C kirag_amd/csrc` (or __graft_entry__.build())"
        lib = C.CDLL(path)
        fn = getattr(lib, "kr_proj_probe_" + dtype)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(Args)]
        lib.kr_proj_probe_error.restype = C.c_char_p
        _libs[dtype] = (lib, fn)
    return _libs[dtype]


_arrays = {}


def arrays(c, dtype):
    c = getattr(c, "arrays_of", c)      # a variant the probe must refuse carries the arrays of the case it was made from
    key = (id(c), dtype)
    if key not in _arrays:
        if len(_arrays) > 8:
            _arrays.clear()
        _arrays[key] = (c, U.probe_arrays(c, dtype))      # (c: the key's id stays taken)
    return _arrays[key][1]


def call(c, dtype, loop, blocks=0, nt=0, ant=0, epi_prio=0, pw=8):
    """one call of the entry point: (return value, the guarded arrays as the probe left them)"""
    lib, fn = probe(dtype)
    X, W, bias = arrays(c, dtype)
    sent = U.SENTINEL[dtype]
    qkv, splade = c.epi in U.QKV_LIKE, c.epi == U.EPI_SPLADE
    w0 = max(c.H if qkv else c.F // 2 if c.epi in U.GATED else c.F, 1)
    rows = c.capT + 2 * U.GUARD_ROWS
    raw = {"out0": np.zeros((rows, w0), np.uint16)}
    if qkv:
        raw["out1"] = np.zeros((rows, max(c.A, 1)), np.uint16)
        raw["outT"] = np.zeros((max(c.A, 1) + 2 * U.GUARD_T_ROWS, max(c.ldT, 0) + 2 * U.GUARD_T_COLS), np.uint16)
    if splade:
        raw["smax"] = np.zeros((max(c.nseq, 0) + 2, max(c.V, 1)), np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rot = c.epi in U.ROTATES
    cos = np.ascontiguousarray(c.cos) if rot else None
    sin = np.ascontiguousarray(c.sin) if rot else None
    a = Args(ptr(X), ptr(W), ptr(bias), ptr(raw["out0"]), ptr(raw.get("out1")), ptr(raw.get("outT")), ptr(cos), ptr(sin), ptr(c.tpos if rot else None),
             ptr(c.row_seq if splade else None), ptr(raw.get("smax")), c.capT, c.ldT, c.T, c.F, c.K, c.H, c.A, c.max_pos, c.dh,
             c.nseq if splade else 0, c.V, c.epi, loop, blocks, nt, ant, epi_prio, pw, sent)
    rc = fn(C.byref(a))
    if rc == -2:      # a HIP error: nothing more is launched on this device from this process
        pytest.exit("projection probe: %s" % lib.kr_proj_probe_error().decode(), returncode=3)
    return rc, raw


def launch(c, dtype, loop, **kw):
    """one launch the probe must accept (check_case first: a wrong test is refused on the host); asserts the sentinels; returns the outputs in checkpoint order"""
    assert U.check_case(c, loop, **kw) is None, (U.check_case(c, loop, **kw), loop, kw)
    rc, raw = call(c, dtype, loop, **kw)
    assert rc == 0, (rc, probe(dtype)[0].kr_proj_probe_error())
    sent, G = U.SENTINEL[dtype], U.GUARD_ROWS
    top = U.round_up(c.T, U.TILE_ROWS[loop])          # the rows a launch may write: whole token tiles
    what = (U.EPI_NAMES[c.epi], c.T, c.F, c.K, loop, kw)
    if c.epi == U.EPI_SPLADE:
        s32 = (sent << 16) | sent
        assert (raw["smax"][0] == s32).all() and (raw["smax"][-1] == s32).all(), ("a guard row of smax was written", what)
    else:
        for name in ("out0", "out1") if c.epi in U.QKV_LIKE else ("out0",):
            assert (raw[name][:G] == sent).all() and (raw[name][G + top:] == sent).all(), ("a row of %s outside the launch's token tiles was written" % name, what)
    if c.epi in U.QKV_LIKE:
        t = raw["outT"].copy()
        t[U.GUARD_T_ROWS:U.GUARD_T_ROWS + c.A, U.GUARD_T_COLS:U.GUARD_T_COLS + top] = sent
        assert (t == sent).all(), ("V^T was written outside its A rows x the launch's token tiles", what)
    return U.unpack_outputs(c, dtype, raw)


def base_loop(epi):
    return 128 if epi == U.EPI_QKV_ROTB else 256      # EPI_QKV_ROTB is not built for the 256 x 256 tile


def configs(name, epi):
    """(loop, knobs) of every launch of a case; the first is the baseline every other must equal bit for bit"""
    loops = U.loops_of(epi)
    out = [(base_loop(epi), {})]
    pers = [l for l in loops if l in U.PERSISTENT]
    nt_ok = epi != U.EPI_SPLADE
    if name == "walk":
        # 18 tiles of 256^2 on 8 blocks: three per block for two, two for the rest; 66 of 128^2 on 8 and 16: up to nine per block
        for l in pers:
            out += [(l, dict(blocks=b) if b else {}) for b in ((0, 8) if l == 256 else (0, 8, 16))]
            out += [(l, dict(blocks=8, pw=1)), (l, dict(blocks=8, pw=3)), (l, dict(blocks=8, epi_prio=1)), (l, dict(blocks=8, epi_prio=2)), (l, dict(blocks=0, pw=3, epi_prio=1))]
            if nt_ok and l != 130:
                out += [(l, dict(nt=1)), (l, dict(nt=1, blocks=8)), (l, dict(nt=1, blocks=8, pw=3, epi_prio=2))]
        if epi == U.EPI_DENSE:
            out += [(256, dict(ant=1)), (256, dict(ant=1, blocks=8)), (256, dict(ant=1, nt=1, blocks=8, pw=1))]
    else:
        for l in pers:
            out += [(l, {}), (l, dict(blocks=8))]
        if nt_ok and name.startswith("long"):
            out += [(l, dict(nt=1)) for l in pers if l != 130]
    out += [(l, {}) for l in loops if l not in U.PERSISTENT]
    return out[:1] + [x for x in out[1:] if x != out[0]]


WORST = {}     # (epilogue, dtype, data, "long" (K = 2560 / 9728: where the fp32 accumulation term leads) / "short") -> (ratio, measured |out - ref|, its bound, where)


def against_reference(c, dtype, out, name):
    """the baseline launch against float64: the exact set's linear epilogues bit for bit, everything within the derived bound"""
    ref, bound = U.reference(c, dtype=dtype)
    key = (U.EPI_NAMES[c.epi], dtype, c.data, "long" if name.startswith("long") else "short")
    for k in ref:
        if k == "smax":
            got, want, b = out[k][:c.nseq].view(np.float32).astype(np.float64), ref[k][:c.nseq], bound[k][:c.nseq]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, "the planted NaN")
        else:
            got, want, b = U.from_bits(out[k], dtype), ref[k], bound[k]
        assert got.shape == want.shape, (name, k, got.shape, want.shape)
        ok = ~np.isnan(want)
        assert np.isfinite(got[ok]).all(), (name, k)
        err = np.abs(got - want)[ok]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err > 0, err / b[ok], 0.0)
        i = int(np.argmax(ratio)) if ratio.size else 0
        w = WORST.get(key)
        if ratio.size and (w is None or ratio[i] > w[0]):
            WORST[key] = (float(ratio[i]), float(err[i]), float(b[ok][i]), "%s %s" % (name, k))
        print("%s %s %s %s %s %s: worst |out - ref| / bound = %.3f" % (key + (name, k, float(ratio[i]) if ratio.size else 0.0)))
        assert (err <= b[ok]).all(), (name, k, float(ratio[i]), np.argwhere(np.abs(got - want) > b)[:4].tolist())
    if c.data == "exact" and c.epi in U.EXACT_BITS:
        want = U.expected_bits(c, dtype)
        for k in want:
            if k == "smax":
                nan = np.isnan(want[k].view(np.float32))
                assert np.array_equal(out[k][:c.nseq][~nan[:c.nseq]], want[k][:c.nseq][~nan[:c.nseq]]), (name, k, "bits")
            else:
                assert np.array_equal(U.no_minus_zero(out[k]), want[k]), (name, k, "bits", int((U.no_minus_zero(out[k]) != want[k]).sum()))


def same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()), np.argwhere(a[k] != b[k])[:4].tolist())


@pytest.fixture(scope="module", autouse=True)
def report():
    """prints the worst measured error over its derived bound per epilogue, type, data set and K class (KIRAG_AMD_PROJ_PROBE_REPORT: also into that file)"""
    yield
    lines = ["epilogue    type  data     K      measured |out - ref|   derived bound   ratio   at (the element of the largest ratio)"]
    for (epi, dtype, data, kclass), (ratio, err, bound, where) in sorted(WORST.items()):
        lines.append("%-11s %-5s %-8s %-6s %.6e           %.6e    %.3f   %s" % (epi, dtype, data, kclass, err, bound, ratio, where))
    print("\n" + "\n".join(lines))
    path = os.environ.get("KIRAG_AMD_PROJ_PROBE_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", range(10), ids=U.EPI_NAMES)
def test_every_loop_grid_and_knob(epi, dtype):
    """Both data sets, every shape of proj_probe_util.cases_of: the baseline launch (loop 256, blocks = 0; EPI_QKV_ROTB: loop 128) against the reference —
    the exact set bit for bit where the epilogue is linear — and every other loop x grid x knob bit for bit against the baseline.  Every launch: the guards
    still hold the sentinel."""
    for data in ("exact", "diffuse"):
        for name, c in U.cases_of(epi, data):
            cfgs = configs(name.split("-")[0], epi)
            base = launch(c, dtype, cfgs[0][0], **cfgs[0][1])
            against_reference(c, dtype, base, name)
            for loop, kw in cfgs[1:]:
                same(base, launch(c, dtype, loop, **kw), (U.EPI_NAMES[epi], data, name, loop, kw))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", range(10), ids=U.EPI_NAMES)
def test_rows_below_T_do_not_depend_on_the_rows_behind(epi, dtype):
    """the rows >= T of X filled in two ways (the loops clamp or zero them): the rows < T keep their bits, on every loop, at every partial last tile"""
    kw = lambda c: dict(H=c.H, A=c.A, dh=c.dh, V=c.V)
    for name, c in U.cases_of(epi, "exact"):
        if name.startswith("long") or name.startswith("region"):
            continue
        other = U.make_case(epi, "exact", c.T, c.F, c.K, fill=U.FILLS[1], **kw(c))
        assert not np.array_equal(other.X[c.T:], c.X[c.T:]) and np.array_equal(other.X[:c.T], c.X[:c.T])
        for loop in U.loops_of(epi):
            b = dict(blocks=8) if (loop in U.PERSISTENT and name == "walk") else {}
            same(launch(c, dtype, loop, **b), launch(other, dtype, loop, **b), ("another fill", U.EPI_NAMES[epi], name, loop))


def test_probe_refuses_what_could_read_out_of_range():
    """the entry point checks its arguments before anything reaches the GPU, and check_case says the same on the host"""
    def variant(c, **changes):
        d = U.Case()
        d.__dict__.update(c.__dict__)
        d.__dict__.update(changes)
        d.arrays_of = c
        return d
    rot = U.make_case(U.EPI_QKV_ROT, "exact", 33, 320, 64, **U.shape_kwargs(U.EPI_QKV_ROT, 320))
    rotb = U.make_case(U.EPI_QKV_ROTB, "exact", 33, 320, 64, **U.shape_kwargs(U.EPI_QKV_ROTB, 320))
    spl = U.make_case(U.EPI_SPLADE, "exact", 33, 320, 64, V=283)
    bad_seq = spl.row_seq.copy()
    bad_seq[3] = spl.nseq
    assert launch(rot, "f16", 128)["out0"].shape == (33, rot.H)
    refused = [(variant(rot, T=rot.capT + 1), 128, {}), (variant(rot, K=96), 128, {}), (variant(rot, F=384), 128, {}), (variant(rot, A=128), 128, {}),
               (variant(rot, ldT=rot.capT - 8), 128, {}), (variant(rot, dh=48), 128, {}), (variant(rot, capT=rot.capT + 64), 128, {}), (rot, 128, dict(blocks=12)),
               (rot, 32, dict(blocks=8)), (rot, 130, dict(nt=1)), (rot, 256, dict(ant=1)), (rot, 128, dict(pw=0)), (rotb, 256, {}),
               (spl, 128, dict(nt=1)), (variant(spl, V=321), 128, {}), (variant(spl, row_seq=bad_seq), 128, {})]
    for c, loop, kw in refused:
        assert U.check_case(c, loop, **kw) is not None, (c.__dict__.get("T"), loop, kw)
        rc, _ = call(c, "f16", loop, **kw)
        assert rc == -1 and probe("f16")[0].kr_proj_probe_error(), (rc, loop, kw)
