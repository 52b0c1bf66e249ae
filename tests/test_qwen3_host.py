"""Qwen3 without a GPU: the Python config rules (kirag_amd.retriever.encoders.check_decoder_config for model_type qwen3), the library's model description
(kirag_amd/csrc/encoder_model.hpp through the stand-alone program tests/capi/qwen3_model_check.cpp, which hands check_tensor the value of config.head_dim as
the loader does), the exported surface, and the reference's teeth.  Every test but the surface one fails on a library without the feature: "qwen3" is an unknown
model_type, "config.head_dim" an unknown setting and "self_attn.q_norm.weight" an unknown tensor there."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qwen3_util as Q  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL, KR_ESTATE = -22, -1
DECODER, QKV_ROT, QKV_ROT_BIAS, QKV_SPLIT, AM_PLAIN, AM_CAUSAL = 7, 1, 2, 3, 0, 4
HEAD_SCORE = 6


def _config_dict(kind, **extra):
    d = Q.hf_config(kind, **extra).to_dict()
    d["model_type"] = "qwen3"
    return d


# ---------------------------------------------------------------------------------------------------------
# the Python rules, from config.json alone
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(Q.SHAPES))
def test_the_three_configs_are_accepted_from_config_json_alone(kind):
    from kirag_amd.retriever.encoders import FAMILIES, Qwen3BGEEncoder, Qwen3E5Encoder, check_decoder_config, describe_decoder
    import transformers
    H, heads, hd, kv = Q.SHAPES[kind]
    d = check_decoder_config(_config_dict(kind))
    assert (d["hidden"], d["heads"], d["kv_heads"], d["head_dim"]) == (H, heads, kv, hd)
    assert d["inv_freq"].numel() == hd // 2      # the frequencies of head_dim, not of hidden / heads
    fam = FAMILIES["qwen3"]
    assert fam.hf_base is transformers.Qwen3Model and fam.twins == (Qwen3E5Encoder, Qwen3BGEEncoder) and fam.flag == "is_decoder"
    spec = describe_decoder(Q.hf_config(kind))
    assert [n for n, _ in spec.settings] == [Q.HEAD_DIM_NAME, Q.INV_FREQ_NAME]      # the width first: the frequencies are counted against it
    assert float(spec.settings[0][1][0]) == hd and spec.cfg[:3] == (H, 2, heads)


def test_the_other_decoders_keep_their_rules():
    """head_dim stays tied to hidden / heads for every other model type, and their handles are sent no head width"""
    import decoder_util as D
    from kirag_amd.retriever.encoders import check_decoder_config, describe_decoder
    d = D.hf_config("qwen2-32").to_dict()
    assert check_decoder_config(dict(d, model_type="qwen2"))["head_dim"] is None
    assert [n for n, _ in describe_decoder(D.hf_config("llama-64")).settings] == [Q.INV_FREQ_NAME]
    with pytest.raises(NotImplementedError, match=r"^model_type='qwen2': head_dim=128 \(hidden_size=256 / num_attention_heads=2\)"):
        check_decoder_config(dict(d, model_type="qwen2", hidden_size=256, num_attention_heads=2, num_key_value_heads=1))


@pytest.mark.parametrize("change, fragment", [
    (dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1), r"hidden_size=256 / num_attention_heads=2 = 128: a handle is created from .* Qwen3-1.7B"),
    (dict(hidden_size=2048, num_attention_heads=16, num_key_value_heads=8, intermediate_size=6144), r"= 128: a handle is created from .* Qwen3-1.7B"),
    (dict(head_dim=96), r"head_dim=96: the attention kernels are built for heads of width 32, 64 and 128"),
    (dict(head_dim=256), r"head_dim=256"),
    (dict(num_attention_heads=4, num_key_value_heads=1, head_dim=32), r"num_key_value_heads=1 x head_dim=32 = 32: the width of k / v must be a multiple of 64"),
    (dict(hidden_size=256, num_attention_heads=8, num_key_value_heads=8, head_dim=32), None),      # accepted: 8 x 32 = 256
    (dict(num_attention_heads=4, num_key_value_heads=2, head_dim=32, hidden_size=256), None),      # hidden / heads = 64, head_dim 32, q 128 wide: accepted
    (dict(hidden_size=384, num_attention_heads=6, num_key_value_heads=2, head_dim=32), r"num_attention_heads=6 x head_dim=32 = 192: the width of q must be a multiple of 128"),
    (dict(hidden_size=2048, num_attention_heads=64, num_key_value_heads=8, head_dim=128, intermediate_size=512), r"= 8192: the width of q must be a multiple of 128 up to 4096"),
    (dict(attention_bias=True), r"attention_bias=True: the q / k norms of a Qwen3 handle run on projections without a bias"),
    (dict(use_sliding_window=True, sliding_window=64), r"use_sliding_window=True"),
    (dict(layer_types=["full_attention", "sliding_attention"]), r"layer_types="),
    (dict(hidden_act="gelu"), r"hidden_act='gelu'"),
    (dict(num_key_value_heads=3, num_attention_heads=4), r"num_key_value_heads=3 does not divide"),
])
def test_refusals_name_the_field(change, fragment):
    from kirag_amd.retriever.encoders import check_decoder_config
    d = _config_dict("q3-128")
    d.update(change)
    if fragment is None:
        check_decoder_config(d)
        return
    with pytest.raises(NotImplementedError, match=r"^model_type='qwen3': .*" + fragment):
        check_decoder_config(d)


def test_rerankers_dispatch_qwen3_and_keep_the_old_tuple():
    from kirag_amd.retriever import rerankers as RR
    import transformers
    assert set(RR.DECODER_RERANKER_TYPES) == {"qwen2", "llama", "mistral"} and RR.QWEN3_RERANKER_TYPES == ("qwen3",)
    assert RR._DECODER_RERANKERS["qwen3"] is RR.Qwen3Reranker and issubclass(RR.Qwen3Reranker, transformers.Qwen3ForSequenceClassification)
    d = _config_dict("q3-128")
    d["num_labels"] = 3
    assert RR.check_decoder_reranker_config(d)["head_dim"] == 128
    with pytest.raises(NotImplementedError, match=r"^model_type='qwen3': num_labels=65"):
        RR.check_decoder_reranker_config(dict(d, num_labels=65, id2label=None))
    with pytest.raises(NotImplementedError, match=r"^model_type='qwen3': .*Qwen3-1.7B"):
        RR.check_decoder_reranker_config(dict(d, hidden_size=256))


# ---------------------------------------------------------------------------------------------------------
# the library's model description
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qwen3_model") / "qwen3_model_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "qwen3_model_check.cpp"), "-o", exe])

    def run(lines, H=128, heads=2, layers=2, max_pos=Q.MAX_POS):
        text = ["config %d %d %d %d %d %d 1" % (H, layers, heads, Q.FF, Q.VOCAB, max_pos)]
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


@functools.lru_cache(maxsize=None)
def script(kind, norms=True, head_dim=True):
    """the lines that load a tiny Qwen3Model the way the Python layer does: settings, then every state-dict key with its element count"""
    cfg = Q.hf_config(kind)
    lines = [("setting", n, v) for n, v in Q.library_settings(cfg) if head_dim or n != Q.HEAD_DIM_NAME]
    for k, v in Q.weights(cfg).items():
        if norms or "_norm.weight" not in k.split("self_attn.")[-1] or "self_attn." not in k:
            lines.append(("tensor", k, v.size))
    return tuple(lines)


def refused(check, lines, code, *fragments, **kw):
    out = check(lines, **kw)
    for ln, d in zip(lines[:-1], out[:-1]):
        assert d["rc"] == 0, (ln, d)
    assert out[-1]["rc"] == code and all(f in out[-1]["msg"] for f in fragments), (lines[-1], out[-1])


@pytest.mark.parametrize("kind", sorted(Q.SHAPES))
def test_a_qwen3_state_dict_resolves_and_finalizes(check, kind):
    H, heads, hd, kv = Q.SHAPES[kind]
    out = check(list(script(kind)) + [("finalize",)], heads=heads)
    assert all(d["rc"] == 0 for d in out), [d for d in out if d["rc"]]
    plan = out[-1]
    assert int(plan["family"]) == DECODER and plan["qkv"] == str(QKV_SPLIT) * 2 and plan["attn"] == str(AM_CAUSAL) * 2
    assert (int(plan["head_w"]), int(plan["q_dim"]), int(plan["kv_dim"]), int(plan["qk_norm"])) == (hd, heads * hd, kv * hd, 1)
    # the weight sync reloads every parameter: the same names and counts are taken again, the norms included, and the plan stays
    again = check(list(script(kind)) + [("finalize",)] + list(script(kind)) + [("finalize",)], heads=heads)
    assert all(d["rc"] == 0 for d in again) and again[-1]["msg"] == plan["msg"]


def test_a_handle_without_the_setting_finalizes_to_the_plan_it_had(check):
    """qwen2-style and llama-style handles (decoder_util's shapes), no head width sent: rotating epilogues, q as wide as hidden, not one new field set"""
    import decoder_util as D
    for kind, qkv in (("qwen2-32", QKV_ROT_BIAS), ("llama-64", QKV_ROT)):
        cfg = D.hf_config(kind)
        mt, H, heads, kv = D.SHAPES[kind]
        inv = 1.0 / (100.0 ** (np.arange(0, H // heads, 2) / (H // heads)))
        lines = [("setting", D.INV_FREQ_NAME, inv), ("setting", D.SETTING, [1.0])] + [("tensor", k, v.size) for k, v in D.weights(cfg).items()] + [("finalize",)]
        out = check(lines, heads=heads)
        assert all(d["rc"] == 0 for d in out), [d for d in out if d["rc"]]
        p = out[-1]
        assert (int(p["family"]), p["qkv"], p["attn"]) == (DECODER, str(qkv) * 2, str(AM_CAUSAL) * 2)
        assert (int(p["head_w"]), int(p["q_dim"]), int(p["kv_dim"]), int(p["qk_norm"])) == (H // heads, H, kv * (H // heads), 0)
    # and the refusal by width at the old place: a grouped k_proj that is no whole number of hidden / heads wide heads
    refused(check, [("setting", D.INV_FREQ_NAME, np.ones(32)), ("setting", D.SETTING, [1.0]), ("tensor", "layers.0.self_attn.k_proj.weight", 96 * 128)], KR_EINVAL,
            "A = kv_heads * 64")


def test_the_setting_takes_32_64_128_on_decoder_handles_only(check):
    for bad in (16, 96, 100, 256, 64.5):
        refused(check, [("setting", Q.HEAD_DIM_NAME, [bad])], KR_EINVAL, "config.head_dim", "32, 64 or 128")
    refused(check, [("setting", Q.HEAD_DIM_NAME, [64, 64])], KR_EINVAL, "takes one value")
    # a handle that is no decoder's: the setting, and either norm tensor, are refused at finalize, by name
    refused(check, [("setting", Q.HEAD_DIM_NAME, [64]), ("finalize",)], KR_EINVAL, "config.head_dim on a handle without config.decoder_attention")
    for t in ("q_norm", "k_norm"):
        refused(check, [("tensor", f"layers.0.self_attn.{t}.weight", 64), ("finalize",)], KR_EINVAL, "_norm.weight", "decoder handles only")
    # the frequencies are counted against the setting; in the wrong order finalize says which comes first
    refused(check, [("setting", Q.HEAD_DIM_NAME, [128]), ("setting", Q.INV_FREQ_NAME, np.ones(32))], KR_EINVAL, "d_h / 2 = 64")
    refused(check, [("setting", Q.INV_FREQ_NAME, np.ones(32)), ("setting", Q.HEAD_DIM_NAME, [128]), ("setting", Q.SETTING, [1.0]), ("finalize",)], KR_EINVAL,
            "config.rotary_inv_freq holds 32 values", "load config.head_dim first")
    # fixed at the first finalize like every setting
    done = list(script("q3-128")) + [("finalize",)]
    out = check(done + [("setting", Q.HEAD_DIM_NAME, [128])])
    assert out[-1]["rc"] == 0
    refused(check, done + [("setting", Q.HEAD_DIM_NAME, [64])], KR_EINVAL, "after kr_encoder_finalize")
    # heads * head_dim: a multiple of 128
    refused(check, [("setting", Q.HEAD_DIM_NAME, [32]), ("setting", Q.INV_FREQ_NAME, np.ones(16)), ("setting", Q.SETTING, [1.0]), ("finalize",)], KR_EINVAL,
            "heads * head_dim = 64 must be a multiple of 128")


def test_partial_norms_width_128_without_norms_and_biases_are_refused(check):
    full = list(script("q3-128"))
    for missing in ("layers.1.self_attn.k_norm.weight", "layers.0.self_attn.q_norm.weight"):
        refused(check, [ln for ln in full if ln[1] != missing] + [("finalize",)], KR_ESTATE, missing, "every layer or none")
    refused(check, [ln for ln in full if "_norm.weight" not in ln[1] or "self_attn" not in ln[1]] + [("finalize",)], KR_EINVAL, "config.head_dim = 128 without", "q / k norms only")
    refused(check, full + [("tensor", "layers.0.self_attn.q_proj.bias", 256), ("finalize",)], KR_EINVAL, "layers.0.self_attn.q_proj.bias", "no q / k bias")
    refused(check, full[:3] + [("tensor", "layers.0.self_attn.q_norm.weight", 64)], KR_EINVAL, "expected head_dim = 128")
    # 64 wide and decoupled, without the norms: accepted, on the rotating epilogue
    out = check([ln for ln in script("q3-64") if "q_norm" not in ln[1] and "k_norm" not in ln[1]] + [("finalize",)], heads=4)
    assert out[-1]["rc"] == 0 and out[-1]["qkv"] == str(QKV_ROT) * 2 and (int(out[-1]["q_dim"]), int(out[-1]["qk_norm"])) == (256, 0), out[-1]
    # norms on a handle finalized without them
    refused(check, [ln for ln in script("q3-64") if "q_norm" not in ln[1] and "k_norm" not in ln[1]] + [("finalize",), ("tensor", "layers.0.self_attn.q_norm.weight", 64)],
            KR_EINVAL, "finalized without q / k norms", heads=4)


def test_element_counts_follow_the_setting(check):
    head = list(script("q3-128"))[:3]
    refused(check, head + [("tensor", "layers.0.self_attn.q_proj.weight", 128 * 128)], KR_EINVAL, "q_proj.weight", "expected 32768", "config.head_dim = 128")
    refused(check, head + [("tensor", "layers.0.self_attn.o_proj.weight", 128 * 128)], KR_EINVAL, "o_proj.weight", "expected 32768")
    refused(check, head + [("tensor", "layers.0.self_attn.k_proj.weight", 64 * 128)], KR_EINVAL, "k_proj.weight", "A = kv_heads * 128")
    refused(check, head + [("tensor", "layers.0.self_attn.k_proj.weight", 384 * 128)], KR_EINVAL, "k_proj.weight")      # A <= Dq = 256
    # without the setting the same q_proj is what every decoder handle refuses
    refused(check, [("setting", Q.INV_FREQ_NAME, np.ones(32)), head[2], ("tensor", "layers.0.self_attn.q_proj.weight", 256 * 128)], KR_EINVAL, "expected 16384")
    # the score head is the decoders' own: one tensor [L, hidden]
    out = check(list(script("q3-128")) + [("tensor", "score.weight", 3 * 128), ("finalize",)])
    assert out[-1]["rc"] == 0 and int(out[-1]["classifier"]) == HEAD_SCORE and int(out[-1]["out_width"]) == 128


def test_abi_9_and_50_exported_functions():
    from kirag_amd import _lib
    assert _lib.ABI_VERSION == 9
    lib = os.path.join(REPO, "kirag_amd", "libkirag_amd.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    names = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines() if " T " in ln}
    assert len([n for n in names if n.startswith("kr_")]) == 50, sorted(names)
    header = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert '"config.head_dim"' in header and "q_norm.weight" in header


# ---------------------------------------------------------------------------------------------------------
# the reference has teeth (HF alone, on the CPU)
# ---------------------------------------------------------------------------------------------------------
HIDDEN_BAR = 3e-2


@pytest.mark.parametrize("kind", ["q3-128", "q3-64"])
def test_every_break_moves_a_reference_row_by_ten_bars(kind):
    cfg = Q.hf_config(kind)
    m = Q.hf_model(cfg, Q.weights(cfg))
    ids, mask = Q.tokens(3, 40, "R", 11)
    keep = mask.astype(bool)
    ref = Q.hf_last_hidden(m, ids, mask)
    with Q.broken(m, None):
        assert np.abs(Q.hf_last_hidden(m, ids, mask) - ref)[keep].max() < 1e-5      # the restated forward IS HF's
    assert np.abs(Q.hf_last_hidden(m, ids, mask) - ref).max() == 0                   # ... and it is gone again
    for how in Q.BREAKS:
        if how == "partner_32" and cfg.head_dim == 64:
            continue                                                                 # j + 32 IS the partner at that width
        with Q.broken(m, how):
            moved = np.abs(Q.hf_last_hidden(m, ids, mask) - ref)[keep].max()
        print("teeth %s %-16s %.3f" % (kind, how, moved))
        assert moved >= 10 * HIDDEN_BAR, (how, moved)
