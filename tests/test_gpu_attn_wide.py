"""k_attn_wide (128-wide heads) launched alone through the library's launch_attn_wide, on operands under which every key decides (tests/capi/attn_probe_wide.hip,
data and reference of tests/attn_probe_util.py at d_h = 128), against a float64 base-2 softmax within attn_probe_util.error_bound.  Plain and causal modes (and
the symmetric window the same instantiation serves), both operand types, heads / KV heads (2, 1) and (4, 2), the lengths where a sequence ends on the edges of a
q-tile, a 64-key step and the 128-key chunk, every heads-per-block variant, gathered key columns, sentinel rows untouched, and the probe's refusals.
tests/test_attn_wide_host.py shows on the CPU that the reference has teeth at this width."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probe_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ("f16", "bf16")
DH = 128
SHAPES = ((2, 1), (4, 2))
LENS = [1, 31, 32, 33, 63, 64, 65, 129]      # plus one of 300 (its own list: three 128-key chunks, ten q-tiles)
MODES = ("plain", "causal")
MODE_ID = {"plain": 0, "window": 2, "causal": 3}
_libs = {}


class Args(C.Structure):      # AttnProbeArgs (tests/capi/attn_probe_wide.hip: the structure of attn_probe.hip)
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("vT", C.c_void_p), ("ctx", C.c_void_p), ("seq_off", C.c_void_p), ("seq_nk", C.c_void_p), ("seq_nq", C.c_void_p),
                ("col", C.c_void_p), ("tab", C.c_void_p), ("capT", C.c_int64),
                ("nseq", C.c_int), ("H", C.c_int), ("ldk", C.c_int), ("heads", C.c_int), ("kv_heads", C.c_int), ("dh", C.c_int), ("mode", C.c_int),
                ("width", C.c_int), ("wl", C.c_int), ("wr", C.c_int), ("gather", C.c_int), ("kernel", C.c_int), ("cap", C.c_int)]


def probe(dtype):
    if dtype not in _libs:
        import torch  # noqa: F401  (one HIP runtime per process, as kirag_amd/_lib.py loads the library)
        path = os.path.join(HERE, "capi", "libattn_probe_wide_%s.so" % dtype)
        assert os.path.exists(path), path + " not found: build it with `make -C kirag_amd/csrc` (or __graft_entry__.build())"
        lib = C.CDLL(path)
        fn = getattr(lib, "kr_attn_probe_wide_" + dtype)
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(Args)]
        lib.kr_attn_probe_wide_error.restype = C.c_char_p
        _libs[dtype] = (lib, fn)
    return _libs[dtype]


def make_args(b, mode, hpb, gather=0, win=None, over=None):
    s0 = b.seqs[0]
    wl, wr = win if win is not None else (s0.win if s0.win is not None else (0, 0))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ctx = b.ctx.copy()
    f = dict(q=ptr(b.q), k=ptr(b.k), vT=ptr(b.vT), ctx=ptr(ctx), seq_off=ptr(b.off), seq_nk=ptr(b.nk), seq_nq=ptr(b.nq), col=ptr(b.col), tab=None, capT=b.capT,
             nseq=len(b.seqs), H=b.H, ldk=b.ldk, heads=s0.heads, kv_heads=s0.kv_heads, dh=s0.dh, mode=MODE_ID[mode], width=0, wl=wl, wr=wr, gather=gather,
             kernel=hpb, cap=U.round_up(int(b.nk.max()), 32))
    f.update(over or {})      # (the refusal test: fields of the structure set to something else)
    return Args(**f), ctx


def launch(b, mode, hpb, gather=0):
    lib, fn = probe(b.dtype)
    a, ctx = make_args(b, mode, hpb, gather)
    rc = fn(C.byref(a))
    if rc == -2:      # a HIP error: nothing more is launched on this device from this process
        pytest.exit("wide attention probe: %s" % lib.kr_attn_probe_wide_error().decode(), returncode=3)
    assert rc == 0, (rc, lib.kr_attn_probe_wide_error())
    assert (ctx[~b.rows] == U.SENTINEL[b.dtype]).all(), "a row outside the launched sequences was written"
    return {i: ctx[o:o + s.nq].copy() for i, (s, o) in enumerate(zip(b.seqs, b.off))}


def seqs_of(lens, shape, mode, data):
    keys = [(n, kind, shape[0], shape[1], DH, mode, data) for n, kind in U.list_kinds(lens, mode)]
    return keys, [U.make_seq(*k) for k in keys]


def hpbs(lens):
    """the heads per block the library picks for the list's width, and every other one the LDS of a CU serves (4 up to 64 keys staged at a time)"""
    cap = U.round_up(max(lens), 32)
    return [4, 2, 1] if cap <= 64 else [2, 1]


def check(out, keys, seqs, dtype, where):
    worst = 0.0
    for i, (key, s) in enumerate(zip(keys, seqs)):
        ref = U.seq_reference(*key).reshape(s.nq, -1)
        got = U.from_bits(out[i], dtype)
        assert np.isfinite(got).all(), (where, key)
        bound = U.error_bound(dtype, s.nk)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / bound)
        assert err <= bound, (where, key, err, bound, np.argwhere(np.abs(got - ref) > bound)[:4].tolist())
    return worst


LISTS = {"tile-edges": [1, 31, 32, 33], "step-edges": [63, 64, 65, 33], "chunk-edge": [129, 64, 1, 65], "long": [300, 31]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_lists_against_float64(shape, mode, dtype):
    """both data sets, every list as one batch (needles: also in reverse order), every heads-per-block variant that serves it; the variants agree bit for bit"""
    assert sorted({n for lens in LISTS.values() for n in lens}) == sorted(LENS + [300])
    worst = 0.0
    for data in ("needles", "diffuse"):
        for name, lens in LISTS.items():
            keys, seqs = seqs_of(lens, shape, mode, data)
            orders = [list(range(len(seqs)))] + ([list(range(len(seqs)))[::-1]] if data == "needles" else [])
            for order in orders:
                b = U.make_batch([seqs[i] for i in order], 4, dtype)
                first = None
                for hpb in hpbs(lens):
                    out = launch(b, mode, hpb)
                    worst = max(worst, check(out, [keys[i] for i in order], b.seqs, dtype, "%s hpb %d" % (name, hpb)))
                    if first is None:
                        first = out
                    for i in out:
                        assert np.array_equal(out[i], first[i]), (name, hpb, i)
    print("[k_attn_wide %dx%d %s %s] worst |ctx - ref| / bound %.3f" % (shape[0], shape[1], mode, dtype, worst))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gathered_key_columns_and_the_window(dtype):
    """causal with holes in the columns takes the gathered path by itself; gather = 1 forces it on consecutive columns: the same bits.  The symmetric window of
    the same instantiation against its own reference."""
    for shape in SHAPES:
        keys, seqs = seqs_of([129, 65, 33, 300], shape, "causal", "needles")
        assert any(k[1] == "holes" for k in keys)
        b = U.make_batch(seqs, 4, dtype)
        for hpb in (1, 2):
            plain = launch(b, "causal", hpb)
            check(plain, keys, seqs, dtype, "causal hpb %d" % hpb)
            forced = launch(b, "causal", hpb, gather=1)
            for i in plain:
                assert np.array_equal(plain[i], forced[i]), (shape, hpb, i)
        keys, seqs = seqs_of([129, 65, 300], shape, "window", "needles")
        b = U.make_batch(seqs, 4, dtype)
        out = launch(b, "window", 1)
        for i, (key, s) in enumerate(zip(keys, seqs)):
            ref = U.seq_reference(*key).reshape(s.nq, -1)
            assert np.abs(U.from_bits(out[i], dtype) - ref).max() <= U.error_bound(dtype, min(s.nk, s.win[0] + s.win[1] + 1)), key


def test_the_fill_around_the_sequences_does_not_leak():
    """the slack, the alignment rows and the other sequences hold +-1024 or -+512: a sequence's rows are the same bits under both"""
    keys, seqs = seqs_of([33, 1, 129, 65], (4, 2), "causal", "diffuse")
    outs = [launch(U.make_batch(seqs, 4, "f16", fill=f), "causal", 1) for f in U.FILLS]
    for i in outs[0]:
        assert np.array_equal(outs[0][i], outs[1][i]), i


def test_the_probe_refuses_what_could_leave_the_arrays():
    lib, fn = probe("f16")
    _, seqs = seqs_of([33, 65], (2, 1), "causal", "needles")
    b = U.make_batch(seqs, 4, "f16")
    bad_off = b.off.copy(); bad_off[1] = b.capT - 8
    odd_off = b.off.copy(); odd_off[1] += 2
    long_nk = b.nk.copy(); long_nk[0] += 8
    col_back = b.col.copy(); col_back[3] = col_back[2]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    cases = [dict(dh=64), dict(H=b.H + 128), dict(ldk=b.ldk * 2), dict(kv_heads=3), dict(capT=0), dict(nseq=0), dict(mode=1), dict(mode=4), dict(kernel=0), dict(kernel=3),
             dict(cap=48), dict(cap=0), dict(kernel=4, cap=128), dict(wl=0, wr=0), dict(col=None), dict(seq_off=ptr(bad_off)), dict(seq_off=ptr(odd_off)),
             dict(seq_nk=ptr(long_nk)), dict(col=ptr(col_back))]
    for over in cases:
        a, ctx = make_args(b, "causal", 1, over=over)
        assert fn(C.byref(a)) == -1 and lib.kr_attn_probe_wide_error(), over
        assert (ctx == U.SENTINEL["f16"]).all(), over
