"""Native grouped-query attention without a GPU: what the loader's host-only part (tests/capi/encoder_model_check.cpp over encoder_model.hpp) accepts and
refuses for k_proj / v_proj tensors of A = kv_heads d_h rows on a decoder handle, that [H, H] tensors and NomicBert handles are what they were, and that the
Python weight sync sends grouped tensors with their HF shapes (expanding only where A is no multiple of 64)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL, KR_ESTATE = -22, -1
L, FF, V = 2, 256, 200
DECODER = 7
DEC = ("setting", D.SETTING, [1.0])
# (H, heads): the checker's own shape of tests/test_decoder_host.py (d_h = 32: A = 64 is 2 KV heads), 64-wide heads over 1 KV head, and 6 x 64 over 2 (group 3)
OWN = (128, 4)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gqa_model") / "encoder_model_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "encoder_model_check.cpp"), "-o", exe])

    def run(lines, shape=OWN, type_vocab=1):
        H, heads = shape
        text = ["config %d %d %d %d %d %d %d" % (H, L, heads, FF, V, 512, type_vocab)]
        for ln in lines:
            text.append(" ".join([ln[0]] + ([ln[1]] if len(ln) > 1 else []) + ([" ".join("%r" % float(x) for x in ln[2])] if ln[0] == "setting" else [str(int(ln[2]))] if ln[0] == "tensor" else [])))
        p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = []
        for row in p.stdout.splitlines():
            head, tail = row.split(" rc=", 1)
            rc, _, msg = tail.partition(" ")
            d = {"rc": int(rc), "msg": msg}
            d.update(kv.split("=", 1) for kv in head.split()[1:] + (msg.split()[1:] if msg.startswith("plan ") else []) if "=" in kv)
            out.append(d)
        assert len(out) == len(lines), p.stdout
        return out
    return run


def _rot(shape):
    H, heads = shape
    return ("setting", "config.rotary_inv_freq", [0.5] * (H // heads // 2))


def _tensors(shape, A, bias=True, A_of=None):
    """a decoder's state dict as (name, count): k_proj / v_proj with A rows; A_of(layer, 'k' | 'v', 'weight' | 'bias') overrides A for single tensors"""
    H, _ = shape
    a = lambda l, x, t: A if A_of is None or A_of(l, x, t) is None else A_of(l, x, t)
    t = [("embed_tokens.weight", V * H), ("norm.weight", H)]
    for l in range(L):
        p = "layers.%d." % l
        t += [(p + "input_layernorm.weight", H), (p + "post_attention_layernorm.weight", H), (p + "mlp.gate_proj.weight", FF * H), (p + "mlp.up_proj.weight", FF * H),
              (p + "mlp.down_proj.weight", FF * H), (p + "self_attn.q_proj.weight", H * H), (p + "self_attn.o_proj.weight", H * H)]
        t += [(p + "self_attn.%s_proj.weight" % x, a(l, x, "weight") * H) for x in "kv"]
        if bias:
            t += [(p + "self_attn.q_proj.bias", H)] + [(p + "self_attn.%s_proj.bias" % x, a(l, x, "bias")) for x in "kv"]
    return [("tensor", n, k) for n, k in t]


def _last(check, lines, shape=OWN, **kw):
    out = check(lines, shape, **kw)
    assert all(d["rc"] == 0 for d in out[:-1]), out
    return out[-1]


GROUPED = [(OWN, 64), ((128, 2), 64), ((384, 6), 128), ((256, 8), 64), ((256, 8), 128)]


@pytest.mark.parametrize("shape,A", GROUPED, ids=["%dx%d-A%d" % (s[1], s[0] // s[1], A) for s, A in GROUPED])
@pytest.mark.parametrize("bias", [True, False])
def test_a_decoder_plan_finalizes_with_grouped_k_and_v(check, shape, A, bias):
    """k_proj / v_proj of A * H elements and biases of A: the same plan as with [H, H] tensors, which is what it was before"""
    plans = []
    for rows in (A, shape[0]):
        out = check([_rot(shape), DEC] + _tensors(shape, rows, bias) + [("finalize",)], shape)
        assert all(d["rc"] == 0 for d in out), (rows, out)
        plans.append(out[-1])
    g, e = plans
    assert g["msg"] == e["msg"]
    assert (e["family"], e["pre_ln"], e["rms"], e["pos"], e["ff"], e["ff_gated"]) == (str(DECODER), "1", "1", "2", "1", "1")
    assert e["qkv"] == ("2" if bias else "1") * L and e["attn"] == "4" * L and e["out_dim"] == str(shape[0])
    # load order is free: v before k, biases first
    t = _tensors(shape, A, bias)
    out = check([_rot(shape), DEC] + t[::-1] + [("finalize",)], shape)
    assert all(d["rc"] == 0 for d in out) and out[-1]["msg"] == g["msg"]


def test_k_and_v_and_the_layers_must_agree(check):
    H = OWN[0]
    cases = [
        (lambda l, x, t: 128 if (l, x, t) == (0, "v", "weight") else None, "layers.0.self_attn.v_proj.weight"),       # k != v
        (lambda l, x, t: 128 if (l, x, t) == (1, "k", "weight") else None, "layers.1.self_attn.k_proj.weight"),       # k != v in layer 1
        (lambda l, x, t: 128 if l == 1 else None, "layers.1.self_attn.k_proj.weight"),                                # the layers disagree
        (lambda l, x, t: 128 if (l, x, t) == (0, "v", "bias") else None, "layers.0.self_attn.v_proj.bias"),           # a bias against its matrix
        (lambda l, x, t: 128 if (l, t) == (1, "bias") else None, "layers.1.self_attn.k_proj.bias"),
    ]
    for A_of, name in cases:
        d = _last(check, [_rot(OWN), DEC] + _tensors(OWN, 64, True, A_of) + [("finalize",)])
        assert d["rc"] == KR_EINVAL and ("'%s'" % name) in d["msg"] and "one width A" in d["msg"], (name, d)
    # the other way round: an [H, H] handle with one grouped tensor
    d = _last(check, [_rot(OWN), DEC] + _tensors(OWN, H, True, lambda l, x, t: 64 if (l, x, t) == (1, "v", "weight") else None) + [("finalize",)])
    assert d["rc"] == KR_EINVAL and "'layers.1.self_attn.v_proj.weight'" in d["msg"]


@pytest.mark.parametrize("shape,A,why", [
    (OWN, 48, "no whole KV heads of 32"), (OWN, 96, "3 KV heads do not divide 4 heads"), (OWN, 32, "one KV head of 32: A % 64 != 0"), (OWN, 160, "more than H"),
    (OWN, 0, "empty"), ((384, 6), 256, "4 KV heads do not divide 6"), ((384, 6), 96, "no whole KV heads of 64"), ((256, 8), 96, "3 KV heads do not divide 8"),
    ((256, 8), 32, "one KV head of 32: A % 64 != 0")])
def test_a_count_that_is_no_valid_A_is_refused_at_load(check, shape, A, why):
    H = shape[0]
    for name, numel in (("layers.0.self_attn.k_proj.weight", A * H), ("layers.1.self_attn.v_proj.weight", A * H), ("layers.0.self_attn.k_proj.bias", A),
                        ("layers.1.self_attn.v_proj.bias", A), ("layers.0.self_attn.k_proj.weight", 64 * H + 1)):
        d = _last(check, [_rot(shape), DEC, ("tensor", name, numel)], shape)
        assert d["rc"] == KR_EINVAL and name in d["msg"] and "expected %d" % (H * H if name.endswith("weight") else H) in d["msg"] and "A % 64 == 0" in d["msg"], (why, d)
    # q and o have no grouped form
    for name in ("layers.0.self_attn.q_proj.weight", "layers.0.self_attn.o_proj.weight"):
        d = _last(check, [_rot(shape), DEC, ("tensor", name, 64 * H)], shape)
        assert d["rc"] == KR_EINVAL and d["msg"] == "tensor '%s' has %d elements, expected %d" % (name, 64 * H, H * H)
    d = _last(check, [_rot(shape), DEC, ("tensor", "layers.0.self_attn.q_proj.bias", 64)], shape)
    assert d["rc"] == KR_EINVAL


def test_a_grouped_count_needs_the_decoder_setting(check):
    """the shared names on a NomicBert handle: [H, H] as before, a grouped count refused at finalize by name"""
    import nomic_util as N
    H, heads = OWN
    w = N.weights(H, L, heads, FF, V)
    sizes = {k: v.size for k, v in w.items()}
    ok = check([_rot(OWN)] + [("tensor", k, n) for k, n in sizes.items()] + [("finalize",)], OWN, type_vocab=2)
    assert all(d["rc"] == 0 for d in ok) and ok[-1]["family"] == "3"
    for name in ("layers.1.self_attn.k_proj.weight", "layers.0.self_attn.v_proj.weight"):
        d = _last(check, [_rot(OWN)] + [("tensor", k, 64 * H if k == name else n) for k, n in sizes.items()] + [("finalize",)], type_vocab=2)
        assert d["rc"] == KR_EINVAL and ("'%s'" % name) in d["msg"] and "config.decoder_attention" in d["msg"], d
    both = {k: (64 * H if "self_attn.k_proj" in k or "self_attn.v_proj" in k else n) for k, n in sizes.items()}
    d = _last(check, [_rot(OWN)] + [("tensor", k, n) for k, n in both.items()] + [("finalize",)], type_vocab=2)
    assert d["rc"] == KR_EINVAL and "'layers.0.self_attn.k_proj.weight'" in d["msg"] and "decoder handles only" in d["msg"]


def test_A_is_fixed_at_the_first_finalize(check):
    H = OWN[0]
    base = [_rot(OWN), DEC] + _tensors(OWN, 64) + [("finalize",)]
    for name, numel in (("layers.0.self_attn.k_proj.weight", 128 * H), ("layers.1.self_attn.v_proj.weight", 128 * H), ("layers.1.self_attn.k_proj.bias", 128),
                        ("layers.0.self_attn.v_proj.bias", 128)):
        d = _last(check, base + [("tensor", name, numel)])
        assert d["rc"] == KR_EINVAL and name in d["msg"] and "after kr_encoder_finalize" in d["msg"] and "A = 64" in d["msg"], d
    # the same A takes new values (the weight sync reloads every parameter), and the handle finalizes again
    out = check(base + _tensors(OWN, 64) + [("finalize",)])
    assert all(d["rc"] == 0 for d in out), out
    # ... and so for a handle that was finalized with [H, H] tensors
    wide = [_rot(OWN), DEC] + _tensors(OWN, H) + [("finalize",)]
    d = _last(check, wide + [("tensor", "layers.0.self_attn.k_proj.weight", 64 * H)])
    assert d["rc"] == KR_EINVAL and "A = 128" in d["msg"]
    assert all(x["rc"] == 0 for x in check(wide + _tensors(OWN, H) + [("finalize",)]))
    # a handle finalized without biases takes one of the handle's A later (zero until then) and no other
    nob = [_rot(OWN), DEC] + _tensors(OWN, 64, bias=False) + [("finalize",)]
    assert _last(check, nob + [("tensor", "layers.0.self_attn.v_proj.bias", 64)])["rc"] == 0
    assert _last(check, nob + [("tensor", "layers.0.self_attn.v_proj.bias", 128)])["rc"] == KR_EINVAL


def test_a_matrix_that_comes_back_with_another_A_invalidates_its_partner(check):
    """before the first finalize: k's rows sit in front of v's in the packed matrix, so k arriving with another A than before has overwritten (or moved away
    from) v's rows; the handle then wants v again instead of computing with stale rows"""
    H = OWN[0]
    t = _tensors(OWN, 64)
    again = [("tensor", "layers.0.self_attn.k_proj.weight", 128 * H), ("tensor", "layers.0.self_attn.k_proj.weight", 64 * H)]
    d = _last(check, [_rot(OWN), DEC] + t + again + [("finalize",)])
    assert d["rc"] == KR_ESTATE and "never loaded" in d["msg"]
    d = _last(check, [_rot(OWN), DEC] + t + again + [("tensor", "layers.0.self_attn.v_proj.weight", 64 * H), ("finalize",)])
    assert d["rc"] == 0


# ---------------------------------------------------------------------------------------------------------
# the width the plan carries
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_kv_dim(tmp_path_factory):
    """tests/capi/gqa_plan_check.cpp: encoder_model_check.cpp prints no kv_dim, and the workspace, the QKV launch and both attention launches are sized by it"""
    exe = str(tmp_path_factory.mktemp("gqa_plan") / "gqa_plan_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "gqa_plan_check.cpp"), "-o", exe])

    def run(lines, shape, type_vocab=1):
        H, heads = shape
        text = ["config %d %d %d %d %d %d %d" % (H, L, heads, FF, V, 512, type_vocab)]
        for ln in lines:
            text.append(" ".join([ln[0]] + ([ln[1]] if len(ln) > 1 else []) + ([" ".join("%r" % float(x) for x in ln[2])] if ln[0] == "setting" else [str(int(ln[2]))] if ln[0] == "tensor" else [])))
        p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr)
        return p.stdout.splitlines()
    return run


@pytest.mark.parametrize("shape,A", GROUPED, ids=["%dx%d-A%d" % (s[1], s[0] // s[1], A) for s, A in GROUPED])
def test_the_plan_carries_A(plan_kv_dim, shape, A):
    """kv_dim = A for grouped tensors (with and without biases, any load order, again after a reload), H for [H, H] tensors and for a NomicBert handle"""
    H = shape[0]
    for bias in (True, False):
        t = _tensors(shape, A, bias)
        assert plan_kv_dim([_rot(shape), DEC] + t + [("finalize",)], shape) == ["finalize rc=0 kv_dim=%d" % A]
        assert plan_kv_dim([_rot(shape), DEC] + t[::-1] + [("finalize",)] + t + [("finalize",)], shape) == ["finalize rc=0 kv_dim=%d" % A] * 2
        assert plan_kv_dim([_rot(shape), DEC] + _tensors(shape, H, bias) + [("finalize",)], shape) == ["finalize rc=0 kv_dim=%d" % H]
    import nomic_util as N
    w = N.weights(H, L, shape[1], FF, V)
    assert plan_kv_dim([_rot(shape)] + [("tensor", k, v.size) for k, v in w.items()] + [("finalize",)], shape, type_vocab=2) == ["finalize rc=0 kv_dim=%d" % H]


# ---------------------------------------------------------------------------------------------------------
# the Python weight sync
# ---------------------------------------------------------------------------------------------------------
class _SpyLib:
    def __init__(self):
        self.loaded = []

    def kr_encoder_load_weight(self, h, name, ptr, numel):
        self.loaded.append((name.decode(), int(numel)))
        return 0

    def kr_encoder_finalize(self, h):
        return 0

    def kr_encoder_destroy(self, h):
        return 0


def _spy_forward(hidden, heads, kv_heads):
    """a HipBertForward that owns no handle: what load_state / sync read of it, and a library that records the loads"""
    from kirag_amd.retriever.encoders import HipBertForward
    f = HipBertForward.__new__(HipBertForward)
    f._lib, f._h = _SpyLib(), None
    f.rename = f.extra = f.fingerprint = None
    f.ff = f.ff_pad = FF
    f.is_decoder, f.is_mpnet, f.is_modern = True, False, False
    f.heads, f.kv_heads, f.hidden = heads, kv_heads, hidden
    return f


@pytest.mark.parametrize("kind", ["qwen2-32", "llama-64", "qwen2-384"])
def test_the_sync_sends_grouped_tensors_with_their_hf_shapes(kind):
    cfg = D.hf_config(kind)
    w = D.weights(cfg)
    H, heads, kv = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads
    A = kv * (H // heads)
    assert A % 64 == 0 and A < H
    want = [(k, v.size) for k, v in w.items()]
    f = _spy_forward(H, heads, kv)
    f.load_state(w)
    assert f._lib.loaded == want
    assert dict(want)["layers.0.self_attn.k_proj.weight"] == A * H and dict(want).get("layers.1.self_attn.v_proj.bias", A) == A
    # the module path: named_parameters() of the HF twin
    m = D.hf_model(cfg, w)
    f = _spy_forward(H, heads, kv)
    f.sync(m)
    assert sorted(f._lib.loaded) == sorted(want)
    # a caller who expanded the tensors: they pass as they are
    from kirag_amd.retriever.encoders import expand_kv
    f = _spy_forward(H, heads, kv)
    f.load_state({k: expand_kv(k, v, heads, kv) for k, v in w.items()})
    assert dict(f._lib.loaded)["layers.0.self_attn.v_proj.weight"] == H * H


@pytest.mark.parametrize("heads,kv", [(4, 1), (2, 1)])
def test_the_sync_expands_where_A_is_no_multiple_of_64(heads, kv):
    """4 heads of 32 over 1 KV head (A = 32): the library has no slice for it, the sync repeats the KV head's rows as before.  2 heads of 64 over 1: native"""
    from kirag_amd.retriever.encoders import expand_kv, kv_for_library
    H = 128
    d = H // heads
    A = kv * d
    rng = np.random.default_rng(3)
    w = {"layers.0.self_attn.k_proj.weight": rng.standard_normal((A, H)).astype(np.float32), "layers.0.self_attn.v_proj.bias": rng.standard_normal(A).astype(np.float32),
         "layers.0.self_attn.q_proj.weight": rng.standard_normal((H, H)).astype(np.float32), "layers.0.input_layernorm.weight": np.ones(H, np.float32)}
    f = _spy_forward(H, heads, kv)
    f.load_state(w)
    got = dict(f._lib.loaded)
    native = A % 64 == 0
    assert got["layers.0.self_attn.k_proj.weight"] == (A if native else H) * H and got["layers.0.self_attn.v_proj.bias"] == (A if native else H)
    assert got["layers.0.self_attn.q_proj.weight"] == H * H and got["layers.0.input_layernorm.weight"] == H
    for k, v in w.items():
        out = kv_for_library(k, torch.from_numpy(v), heads, kv, H)
        assert torch.equal(out, torch.from_numpy(v) if native else expand_kv(k, torch.from_numpy(v), heads, kv))
