"""The encoder's model description without a GPU: kirag_amd/csrc/encoder_model.hpp (name tables, head table, settings table, describe()) driven through the
stand-alone program tests/capi/encoder_model_check.cpp.

1. Resolution: every state_dict key of a tiny HF model of each supported type resolves to a slot with the tensor's element count (or is an ignored name), the
   handle finalizes, and the plan names the family's norm, position source, epilogues and attention per layer; the same for each head on an accepting family.
2. Refusals: what the test_gpu_* files reach through kr_last_error() — same return code, same message fragment, same order where two rules are broken."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3_util as M3  # noqa: E402
import modernbert_reranker_util as MR  # noqa: E402
import modernbert_util as M  # noqa: E402
import mpnet_util as MP  # noqa: E402
import nomic_util as N  # noqa: E402
import reranker_util as R  # noqa: E402
import splade_util as SP  # noqa: E402
import t5_util as T  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL, KR_ESTATE = -22, -1
H, L, FF, V, MAX_POS = 128, 2, 256, 120, 64
# the enums of encoder_model.hpp, as the program prints them
BERT, MPNET, NOMIC, MODERN, T5 = 1, 2, 3, 4, 5
POS_COLUMN, POS_FAIRSEQ, POS_ROTARY, POS_BIAS_ONLY = 0, 1, 2, 3
FF_GELU, FF_SWIGLU, FF_GEGLU, FF_RELU, FF_GEGLU_TANH = 0, 1, 2, 3, 4
HEAD_MLM, HEAD_COLBERT, HEAD_SPARSE, HEAD_DENSE, HEAD_CLS, HEAD_MODERN_CLS = range(6)
WS_POOLED, WS_SLOT_ROW, WS_ROW_SEQ, WS_CY = 1, 2, 4, 8
TYPES = "embeddings.token_type_embeddings.weight"
PAD_NAME, T5_NAME = "config.position_padding_idx", T.SETTING


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("encoder_model") / "encoder_model_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "encoder_model_check.cpp"), "-o", exe])

    def run(lines, heads=2, type_vocab=2, layers=L, max_pos=MAX_POS):
        """lines: ("setting", name, values) / ("tensor", name, numel) / ("finalize",) -> one dict per line: rc, msg and the printed fields"""
        text = ["config %d %d %d %d %d %d %d" % (H, layers, heads, FF, V, max_pos, type_vocab)]
        for ln in lines:
            text.append(" ".join([ln[0]] + ([ln[1]] if len(ln) > 1 else []) + ([" ".join("%r" % float(x) for x in ln[2])] if ln[0] == "setting" else [str(int(ln[2]))] if ln[0] == "tensor" else [])))
        p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = []
        for row in p.stdout.splitlines():
            head, tail = row.split(" rc=", 1)
            rc, _, msg = tail.partition(" ")
            d = {"rc": int(rc), "msg": msg, "cmd": head.split()[0]}
            d.update(kv.split("=", 1) for kv in head.split()[1:] + (msg.split()[1:] if msg.startswith("plan ") else []) if "=" in kv)
            out.append(d)
        assert len(out) == len(lines), p.stdout
        return out
    return run


def refused(check, lines, code, *fragments, **kw):
    """the LAST line of the script is refused with `code` and a message holding every fragment; every line before it succeeds"""
    out = check(lines, **kw)
    for ln, d in zip(lines[:-1], out[:-1]):
        assert d["rc"] == 0, (ln, d)
    assert out[-1]["rc"] == code and all(f in out[-1]["msg"] for f in fragments), (lines[-1], out[-1])
    return out[-1]["msg"]


# ---------------------------------------------------------------------------------------------------------
# tiny HF models: the settings the Python layer derives, every state_dict key with its element count
# ---------------------------------------------------------------------------------------------------------
KINDS = ("bert", "xlm-roberta", "mpnet", "nomic_bert", "modernbert", "modernbert+bias", "t5", "t5-gated")


@functools.lru_cache(maxsize=None)
def model(kind, heads):
    """-> (settings, tensors, type_vocab): lines of a script that finalizes"""
    import transformers as tr
    common = dict(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=V, max_position_embeddings=MAX_POS)
    half, type_vocab, settings = H // heads // 2, 1, []
    if kind == "bert":
        m, type_vocab = tr.BertModel(tr.BertConfig(type_vocab_size=2, **common)), 2
    elif kind == "xlm-roberta":
        m, settings = tr.XLMRobertaModel(tr.XLMRobertaConfig(type_vocab_size=1, pad_token_id=1, **common)), [(PAD_NAME, [1])]
    elif kind == "mpnet":
        m, settings = tr.MPNetModel(tr.MPNetConfig(relative_attention_num_buckets=32, **common)), [(PAD_NAME, [MP.PAD])]
    elif kind == "nomic_bert":
        m, type_vocab = tr.NomicBertModel(N.hf_config(N.cfg(H, L, heads, FF, V, MAX_POS)), add_pooling_layer=False), 2
        settings = [(N.INV_FREQ_NAME, N.inv_freq(H // heads))]
    elif kind.startswith("modernbert"):
        extra = dict(norm_bias=True, attention_bias=True, mlp_bias=True) if kind.endswith("+bias") else {}
        m = tr.ModernBertModel(M.hf_config(M.cfg(H, L, heads, FF, V, MAX_POS, types=[M.FULL, M.SLIDING], local_attention=16, **extra)))
        settings = [(M.GLOBAL_FREQ_NAME, M.inv_freq(H // heads, M.THETA[M.FULL])), (M.LOCAL_FREQ_NAME, M.inv_freq(H // heads, M.THETA[M.SLIDING])),
                    (M.HALF_WINDOW_NAME, [8]), (M.LAYER_FLAGS_NAME, [0, 1])]
    else:
        m = tr.T5EncoderModel(T.hf_config(T.cfg(H, L, heads, FF, V, T.GATED if kind == "t5-gated" else T.RELU)))
        settings = [(T5_NAME, [1 if kind == "t5-gated" else 0])]
    assert all(len(v) in (1, half, L) for _, v in settings)
    tensors = [(k, v.numel()) for k, v in m.state_dict().items()]
    if not any(k.endswith("token_type_embeddings.weight") for k, _ in tensors) and not kind.startswith("t5"):
        tensors.append((TYPES, type_vocab * H))      # the zero row the Python layer loads for a model without token types (encoders.py)
    return tuple(("setting", k, tuple(float(x) for x in np.asarray(v).ravel())) for k, v in settings), tuple(("tensor", k, n) for k, n in tensors), type_vocab


def script(kind, heads=2, drop=(), extra=()):
    s, t, tv = model(kind, heads)
    return [ln for ln in list(s) + list(t) if ln[1] not in drop] + list(extra), dict(heads=heads, type_vocab=tv)


EXPECT = {   # family, pre_ln, rms, pos, ff, ff_gated, qkv per layer, attention per layer
    "bert": (BERT, 0, 0, POS_COLUMN, FF_GELU, 0, "00", "00"), "xlm-roberta": (BERT, 0, 0, POS_FAIRSEQ, FF_GELU, 0, "00", "00"),
    "mpnet": (MPNET, 0, 0, POS_FAIRSEQ, FF_GELU, 0, "00", "11"), "nomic_bert": (NOMIC, 0, 0, POS_ROTARY, FF_SWIGLU, 1, "11", "00"),
    "modernbert": (MODERN, 1, 0, POS_ROTARY, FF_GEGLU, 1, "11", "02"), "modernbert+bias": (MODERN, 1, 0, POS_ROTARY, FF_GEGLU, 1, "22", "02"),
    "t5": (T5, 1, 1, POS_BIAS_ONLY, FF_RELU, 0, "00", "11"), "t5-gated": (T5, 1, 1, POS_BIAS_ONLY, FF_GEGLU_TANH, 1, "00", "11")}


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_every_state_dict_key_resolves_and_the_plan_names_the_family(check, kind, heads):
    lines, kw = script(kind, heads, extra=[("finalize",)])
    out = check(lines, **kw)
    seen = set()
    for ln, d in zip(lines[:-1], out[:-1]):
        assert d["rc"] == 0, (ln, d)
        if ln[0] == "tensor":
            if "pooler." in ln[1] or "position_ids" in ln[1]:
                assert int(d["slot"]) == -1, (ln, d)
            else:
                assert int(d["slot"]) != -1 and int(d["expect"]) == ln[2], (ln, d)
                seen.add(int(d["family"]))
    fam, pre_ln, rms, pos, ff, gated, qkv, attn = EXPECT[kind]
    # the family of the names: BERT's for the embeddings of MPNet and NomicBert, else the model's own
    assert seen == {BERT: {BERT}, MPNET: {BERT, MPNET}, NOMIC: {BERT, NOMIC}, MODERN: {MODERN, BERT}, T5: {T5}}[fam if kind != "xlm-roberta" else BERT], seen
    p = out[-1]
    assert p["rc"] == 0, p
    got = (int(p["family"]), int(p["pre_ln"]), int(p["rms"]), int(p["pos"]), int(p["ff"]), int(p["ff_gated"]), p["qkv"], p["attn"])
    assert got == EXPECT[kind], (got, EXPECT[kind])
    assert int(p["pad_idx"]) == (1 if pos == POS_FAIRSEQ else -1) and int(p["half_window"]) == (8 if fam == MODERN else 0)
    assert p["heads"] == "000000" and int(p["classifier"]) == -1 and int(p["out_dim"]) == H and int(p["out_width"]) == H and int(p["ws"]) == 0


HEAD_CASES = [   # family, head tensors with counts, the plan's head bits, classifier, out_dim, out_width, workspace
    ("t5", [("dense.weight", 8 * H)], "000100", -1, 8, 8, WS_POOLED),
    ("bert", list(zip(R.HEAD, (H * H, H, 3 * H, 3))), "000010", HEAD_CLS, H, H, WS_POOLED),
    ("mpnet", list(zip(R.HEAD, (H * H, H, 3 * H, 3))), "000010", HEAD_CLS, H, H, WS_POOLED),
    ("modernbert", list(zip(MR.HEAD, (H * H, H, H, H, 3 * H, 3))), "000001", HEAD_MODERN_CLS, H, H, WS_POOLED),
    ("modernbert", [(k, n) for k, n in zip(MR.HEAD, (H * H, H, H, H, 3 * H, 3)) if k in MR.HEAD_REQUIRED], "000001", HEAD_MODERN_CLS, H, H, WS_POOLED),
    ("xlm-roberta", list(zip(M3.HEADS, (256 * H, 256, H, 1))), "011000", -1, H, H, WS_SLOT_ROW | WS_CY),
    ("xlm-roberta", list(zip(M3.HEADS[2:], (H, 1))), "001000", -1, H, H, WS_SLOT_ROW),
    ("bert", list(zip(SP.MLM, (H * H, H, H, H, V * H, V))), "100000", -1, H, H, WS_ROW_SEQ)]


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "%s-%s" % (c[0], c[2]))
def test_every_head_on_an_accepting_family(check, case):
    kind, tensors, bits, classifier, out_dim, out_width, ws = case
    lines, kw = script(kind, extra=[("tensor", k, n) for k, n in tensors] + [("finalize",)])
    out = check(lines, **kw)
    assert all(d["rc"] == 0 for d in out), [d for d in out if d["rc"]]
    p = out[-1]
    assert (p["heads"], int(p["classifier"]), int(p["out_dim"]), int(p["out_width"]), int(p["ws"])) == (bits, classifier, out_dim, out_width, ws), p
    # the same shapes again after the finalize: new values, and the handle finalizes again
    again = check(lines + [("tensor", k, n) for k, n in tensors] + [("finalize",)], **kw)
    assert all(d["rc"] == 0 for d in again)


def head_lines(names, counts):
    return [("tensor", k, n) for k, n in zip(names, counts)]


CLS = head_lines(R.HEAD, (H * H, H, 3 * H, 3))
MCLS = head_lines(MR.HEAD, (H * H, H, H, H, 3 * H, 3))
MLM = head_lines(SP.MLM, (H * H, H, H, H, V * H, V))
COLBERT, SPARSE = head_lines(M3.HEADS[:2], (128 * H, 128)), head_lines(M3.HEADS[2:], (H, 1))
DENSE = [("tensor", "dense.weight", 8 * H)]
FIN = [("finalize",)]


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
def test_names_of_the_wrong_family(check):
    nomic, kw = script("nomic_bert")
    modern, mkw = script("modernbert")
    bert, bkw = script("bert")
    t5, tkw = script("t5")
    gated, _ = script("t5-gated")
    setting = lambda lines: [ln for ln in lines if ln[0] == "setting"]
    tensors = lambda lines: [ln for ln in lines if ln[0] == "tensor"]
    # test_gpu_modernbert: ModernBert's names on a NomicBert handle and the reverse; test_gpu_nomic: NomicBert's names without the setting, BERT's with it
    refused(check, setting(nomic) + tensors(modern) + FIN, KR_EINVAL, "ModernBert name", **mkw)
    refused(check, setting(modern) + [ln for ln in tensors(nomic) if ln[1] != TYPES] + [("tensor", TYPES, H)] + FIN, KR_EINVAL, "takes ModernBert's names", **mkw)
    refused(check, tensors(nomic) + [("tensor", "embeddings.position_embeddings.weight", MAX_POS * H)] + FIN, KR_EINVAL, "config.rotary_inv_freq", **kw)
    refused(check, setting(nomic) + tensors(bert) + FIN, KR_EINVAL, "under NomicBert's names", **bkw)
    # test_gpu_t5: T5's names on a BERT handle (a matrix, the table, everything), BERT's and MPNet's spellings on a T5 handle, the wrong feed-forward spelling
    q = [ln for ln in t5 if ln[1] == "encoder.block.0.layer.0.SelfAttention.q.weight"]
    refused(check, bert + q + FIN, KR_EINVAL, T5_NAME, **bkw)
    refused(check, bert + [("tensor", T.BIAS_NAME, 32 * 2)] + FIN, KR_EINVAL, T5_NAME, **bkw)
    refused(check, tensors(t5) + FIN, KR_EINVAL, T5_NAME, **tkw)
    refused(check, t5 + [ln for ln in bert if ln[1] == "encoder.layer.0.attention.self.query.weight"] + FIN, KR_EINVAL, T5_NAME, **tkw)
    refused(check, [ln for ln in t5 if ln[1] != T.BIAS_NAME] + [("tensor", MP.BIAS_NAME, 32 * 2)] + FIN, KR_EINVAL, T5_NAME, **tkw)
    refused(check, setting(t5) + tensors(gated) + FIN, KR_EINVAL, "wi, not wi_0 / wi_1", **tkw)
    refused(check, setting(gated) + tensors(t5) + FIN, KR_EINVAL, "wi_0 / wi_1, not wi", **tkw)
    # load-time refusals of names (test_gpu_modernbert, test_gpu_t5)
    refused(check, [("tensor", "layers.0.attn_norm.weight", H)], KR_EINVAL, "identity", **mkw)
    refused(check, [("tensor", "layers.0.attn.Wqkv.bias", 2 * H)], KR_EINVAL, "expected %d" % (3 * H), **mkw)
    refused(check, [("tensor", "layers.0.attn.Wqkv.weight", H * H)], KR_EINVAL, **mkw)
    refused(check, [("tensor", T.BIAS_NAME, 16 * 2)], KR_EINVAL, "32 buckets", **tkw)
    refused(check, [("tensor", MP.BIAS_NAME, 16 * 4)], KR_EINVAL, "128", "32 buckets", heads=4)       # test_gpu_mpnet
    refused(check, [("tensor", T.BIAS_NAME.replace("block.0", "block.1"), 32 * 2)], KR_EINVAL, "block 0", **tkw)
    refused(check, [("tensor", "encoder.layer.2.output.dense.bias", H)], KR_EINVAL, "bad layer index")
    refused(check, [("tensor", "encoder.layer.0.output.dense.gamma", H)], KR_EINVAL, "unknown layer tensor")
    refused(check, [("tensor", "lm_head.weight", H)], KR_EINVAL, "unknown tensor name")


def test_mixed_position_schemes_and_settings_that_do_not_add_up(check):
    modern, mkw = script("modernbert")
    nomic, nkw = script("nomic_bert")
    t5, tkw = script("t5")
    half = H // 2 // 2
    # test_gpu_modernbert
    drop = lambda lines, *names: [ln for ln in lines if ln[1] not in names]
    refused(check, drop(modern, M.LAYER_FLAGS_NAME) + [("setting", M.LAYER_FLAGS_NAME, [0, 1, 0])] + FIN, KR_EINVAL, "config.local_attention_layers holds 3 flags", **mkw)
    refused(check, drop(modern, M.LOCAL_FREQ_NAME) + FIN, KR_EINVAL, "config.rotary_inv_freq_local", **mkw)
    refused(check, drop(modern, M.HALF_WINDOW_NAME) + FIN, KR_EINVAL, "config.attention_half_window", **mkw)
    refused(check, drop(modern, M.GLOBAL_FREQ_NAME) + FIN, KR_EINVAL, "without config.rotary_inv_freq", **mkw)
    refused(check, modern + [("setting", PAD_NAME, [1])] + FIN, KR_EINVAL, "one position scheme", **mkw)
    refused(check, modern + [("tensor", MP.BIAS_NAME, 32 * 2)] + FIN, KR_EINVAL, "one position scheme", **mkw)
    refused(check, [ln for ln in modern if ln[0] == "setting" and ln[1] != M.LAYER_FLAGS_NAME] + [ln for ln in nomic if ln[0] == "tensor"] + FIN, KR_EINVAL,
            "without config.local_attention_layers", **nkw)
    # all layers global: the local settings are not needed
    out = check(drop(modern, M.LOCAL_FREQ_NAME, M.HALF_WINDOW_NAME, M.LAYER_FLAGS_NAME) + [("setting", M.LAYER_FLAGS_NAME, [0, 0])] + FIN, **mkw)
    assert out[-1]["rc"] == 0 and out[-1]["attn"] == "00", out[-1]
    # NomicBert next to the other schemes
    refused(check, nomic + [("setting", PAD_NAME, [1])] + FIN, KR_EINVAL, "one position scheme", **nkw)
    # test_gpu_t5: next to each foreign setting the refusal names config.t5_feed_forward
    for name, val in ((PAD_NAME, [1]), ("config.rotary_inv_freq", np.ones(half)), ("config.rotary_inv_freq_local", np.ones(half)), (M.LAYER_FLAGS_NAME, [0, 0]),
                      (M.HALF_WINDOW_NAME, [4])):
        refused(check, t5 + [("setting", name, val)] + FIN, KR_EINVAL, T5_NAME, **tkw)


def test_settings_at_load_time_and_after_the_first_finalize(check):
    half = H // 2 // 2
    inv = N.inv_freq(H // 2)
    # counts and values (test_gpu_nomic, test_gpu_modernbert, test_gpu_t5, test_gpu_modernbert_reranker)
    refused(check, [("setting", N.INV_FREQ_NAME, inv[:8])], KR_EINVAL, str(half))
    refused(check, [("setting", M.LOCAL_FREQ_NAME, inv[:3])], KR_EINVAL, str(half))
    refused(check, [("setting", M.HALF_WINDOW_NAME, [0])], KR_EINVAL, ">= 1")
    refused(check, [("setting", M.HALF_WINDOW_NAME, [1, 2])], KR_EINVAL)
    refused(check, [("setting", M.LAYER_FLAGS_NAME, [0, 2])], KR_EINVAL, "0 / 1")
    for bad in ([2], [0.5], [-1], [0, 1]):
        refused(check, [("setting", T5_NAME, bad)], KR_EINVAL)
    for bad in ([2], [0.5], [0, 1]):
        refused(check, [("setting", MR.POOLING_NAME, bad)], KR_EINVAL)
    for bad in ([-1], [MAX_POS - 1], [1.5]):
        refused(check, [("setting", PAD_NAME, bad)], KR_EINVAL, PAD_NAME)
    refused(check, [("setting", "config.no_such_setting", [0])], KR_EINVAL, T5_NAME)
    refused(check, [("setting", N.INV_FREQ_NAME, inv)], KR_EINVAL, "8192", max_pos=8193)
    out = check([("setting", MR.POOLING_NAME, [1]), ("setting", MR.POOLING_NAME, [0])])     # before the first finalize: any order
    assert [d["rc"] for d in out] == [0, 0]
    # after the first finalize: the same values are a no-op, anything else is refused
    modern, mkw = script("modernbert")
    for ln in modern:
        if ln[0] == "setting":
            assert check(modern + FIN + [ln], **mkw)[-1]["rc"] == 0, ln
    lf = M.inv_freq(H // 2, M.THETA[M.SLIDING])
    for name, val in ((M.LOCAL_FREQ_NAME, 2 * lf), (M.HALF_WINDOW_NAME, [7]), (M.LAYER_FLAGS_NAME, [1, 1]), (M.LAYER_FLAGS_NAME, [0, 1, 0])):
        refused(check, modern + FIN + [("setting", name, val)], KR_EINVAL, "finalize", **mkw)
    nomic, nkw = script("nomic_bert")
    refused(check, nomic + FIN + [("setting", N.INV_FREQ_NAME, 2 * inv)], KR_EINVAL, "finalize", **nkw)
    bert, bkw = script("bert")
    refused(check, bert + FIN + [("setting", N.INV_FREQ_NAME, inv)], KR_EINVAL, "finalize", **bkw)
    refused(check, bert + FIN + [("setting", T5_NAME, [0])], KR_EINVAL, "finalize", **bkw)
    refused(check, bert + FIN + [("setting", PAD_NAME, [1])], KR_EINVAL, "finalize", "= 1", "BERT's position rule", **bkw)
    t5, tkw = script("t5")
    assert check(t5 + FIN + [("setting", T5_NAME, [0])], **tkw)[-1]["rc"] == 0
    refused(check, t5 + FIN + [("setting", T5_NAME, [1])], KR_EINVAL, "finalize", **tkw)
    refused(check, t5 + FIN + [("setting", PAD_NAME, [1])], KR_EINVAL, **tkw)
    xlmr, xkw = script("xlm-roberta")
    assert check(xlmr + FIN + [("setting", PAD_NAME, [1])], **xkw)[-1]["rc"] == 0
    refused(check, xlmr + FIN + [("setting", PAD_NAME, [2])], KR_EINVAL, "finalize", "= 2", "it has 1", **xkw)       # the offered value and the handle's
    # MPNet's table on a handle finalized without it
    refused(check, bert + FIN + [("tensor", MP.BIAS_NAME, 32 * 2)], KR_EINVAL, "finalize", **bkw)


def test_missing_slots(check):
    for kind, drop in (("nomic_bert", "layers.0.mlp.gate_proj.weight"), ("nomic_bert", "layers.0.mlp.up_proj.weight"), ("modernbert", "layers.1.mlp.Wi.weight"),
                       ("mpnet", "encoder.layer.1.attention.attn.o.bias"), ("bert", "embeddings.position_embeddings.weight"), ("t5", T.BIAS_NAME),
                       ("t5", "encoder.final_layer_norm.weight"), ("t5-gated", "encoder.block.0.layer.1.DenseReluDense.wi_1.weight")):
        lines, kw = script(kind, drop=(drop,))
        refused(check, lines + FIN, KR_ESTATE, "never loaded", **kw)
        numel = dict((ln[1], ln[2]) for ln in script(kind)[0])[drop]
        assert check(lines + FIN + [("tensor", drop, numel)] + FIN, **kw)[-1]["rc"] == 0, drop
    # what a family leaves optional: ModernBert's biases and betas, T5's position / type tables
    lines, kw = script("modernbert+bias")
    assert int(check(lines + FIN, **kw)[-1]["zero_fill"]) < int(check(script("modernbert")[0] + FIN, **kw)[-1]["zero_fill"])


def test_incomplete_heads_and_their_shapes(check):
    bert, bkw = script("bert")
    modern, mkw = script("modernbert")
    for head, base, kw, required in ((CLS, bert, bkw, R.HEAD), (MLM, bert, bkw, SP.MLM), (COLBERT, bert, bkw, M3.HEADS[:2]), (SPARSE, bert, bkw, M3.HEADS[2:]),
                                     (MCLS, modern, mkw, MR.HEAD_REQUIRED)):
        for drop in required:
            refused(check, base + [ln for ln in head if ln[1] != drop] + FIN, KR_ESTATE, "never loaded", drop, **kw)
    # shapes: the free dimension's bounds and granularity, weight and bias agreeing, the fixed shapes
    assert "%" not in refused(check, [("tensor", R.HEAD[2], 65 * H)], KR_EINVAL, "1 <= L <= 64")      # no granularity clause where every L is allowed
    refused(check, [("tensor", MR.HEAD[4], 65 * H)], KR_EINVAL, "64")
    refused(check, [("tensor", MR.HEAD[4], H + 4)], KR_EINVAL)
    refused(check, [("tensor", MR.HEAD[4], 64 * H), ("tensor", MR.HEAD[5], 63)], KR_EINVAL, "L = 64")
    for P in (64, 192, 2176):
        refused(check, [("tensor", M3.HEADS[0], P * H)], KR_EINVAL, "2048")
    refused(check, [("tensor", M3.HEADS[0], H - 1)], KR_EINVAL)
    refused(check, [("tensor", M3.HEADS[1], 100)], KR_EINVAL)
    refused(check, [("tensor", M3.HEADS[0], 2048 * H), ("tensor", M3.HEADS[1], 128)], KR_EINVAL, "2048")
    refused(check, [("tensor", M3.HEADS[2], H + 1)], KR_EINVAL)
    refused(check, [("tensor", M3.HEADS[3], 2)], KR_EINVAL)
    for n in (H * 8 + 1, H * 2, H * 6, H * 2052):
        refused(check, [("tensor", "dense.weight", n)], KR_EINVAL, "dense.weight")
    for rows in (V - 1, V + 1):
        refused(check, [("tensor", SP.MLM[4], rows * H)], KR_EINVAL, "vocab_size")
        refused(check, [("tensor", SP.MLM[5], rows)], KR_EINVAL)
    refused(check, [("tensor", SP.MLM[0], H * H + 1)], KR_EINVAL)
    refused(check, [("tensor", MR.HEAD[3], 2 * H)], KR_EINVAL)


def test_heads_on_the_wrong_family_and_exclusive_heads(check):
    bert, bkw = script("bert")
    modern, mkw = script("modernbert")
    t5, tkw = script("t5")
    half = lambda heads: H // heads // 2
    foreign = {"T5": (t5, tkw), "NomicBert": ([("setting", N.INV_FREQ_NAME, np.ones(half(2)))], {}),
               "ModernBert": ([("setting", N.INV_FREQ_NAME, np.ones(half(2))), ("setting", M.LAYER_FLAGS_NAME, [0, 0])], {}),
               "MPNet": ([("tensor", MP.BIAS_NAME, 32 * 2)], {})}
    # test_gpu_m3 / test_gpu_splade: refused at finalize naming the head's first tensor and the family, before anything is reported missing
    for word, (base, kw) in foreign.items():
        for head in (COLBERT, SPARSE, MLM):
            refused(check, base + head + FIN, KR_EINVAL, head[0][1], word, **kw)
    # test_gpu_reranker / test_gpu_modernbert_reranker: the tanh classifier is BERT's, RoBERTa's and MPNet's; ModernBert's head is ModernBert's
    for word in ("T5", "NomicBert", "ModernBert"):
        refused(check, foreign[word][0] + CLS + FIN, KR_EINVAL, "classifier.*", word, **foreign[word][1])
    for extra in ([], MCLS):
        refused(check, modern + extra + CLS + FIN, KR_EINVAL, "classifier.*", "ModernBert", **mkw)
    for ln in MCLS:
        refused(check, [ln] + FIN, KR_EINVAL, ln[1])
    refused(check, [("setting", N.INV_FREQ_NAME, np.ones(half(2)))] + MCLS + FIN, KR_EINVAL, MR.HEAD[0])
    refused(check, bert + DENSE + FIN, KR_EINVAL, "dense.weight", **bkw)
    # exclusive heads; where two rules are broken, the order of the GPU tests: the token-level heads and the MLM head are reported before the Dense head's own
    # rule and before the classifier
    refused(check, bert + CLS + MLM + FIN, KR_EINVAL, SP.MLM[0], "classifier", **bkw)
    refused(check, bert + SPARSE + MLM + FIN, KR_EINVAL, SP.MLM[0], "sparse_linear", **bkw)
    refused(check, bert + COLBERT + MLM + FIN, KR_EINVAL, SP.MLM[0], "colbert_linear", **bkw)
    for head in (COLBERT, SPARSE):
        refused(check, bert + CLS + head + FIN, KR_EINVAL, head[0][1], "classifier", **bkw)
        refused(check, bert + DENSE + head + FIN, KR_EINVAL, head[0][1], "dense.weight", **bkw)
    refused(check, t5 + DENSE + CLS + FIN, KR_EINVAL, "classifier", "T5", **tkw)
    # config.classifier_pooling goes with ModernBert's head
    refused(check, modern + [("setting", MR.POOLING_NAME, [0])] + FIN, KR_EINVAL, MR.POOLING_NAME, **mkw)
    refused(check, [("setting", MR.POOLING_NAME, [1])] + FIN, KR_EINVAL, MR.POOLING_NAME)
    out = check(modern + MCLS + [("setting", MR.POOLING_NAME, [1])] + FIN, **mkw)
    assert out[-1]["rc"] == 0 and int(out[-1]["classify_mean"]) == 1, out[-1]


def test_heads_after_the_first_finalize(check):
    bert, bkw = script("bert")
    modern, mkw = script("modernbert")
    t5, tkw = script("t5")
    # a head, or its setting, arriving late: "finalized without"
    for base, kw, head in ((bert, bkw, CLS), (bert, bkw, MLM), (bert, bkw, COLBERT), (bert, bkw, SPARSE), (modern, mkw, MCLS), (t5, tkw, DENSE)):
        for ln in head:
            msg = refused(check, base + FIN + [ln], KR_EINVAL, "finalize", **kw)
            assert head is DENSE or "finalized without" in msg, msg
    refused(check, modern + FIN + [("setting", MR.POOLING_NAME, [1])], KR_EINVAL, **mkw)
    refused(check, modern + FIN + [("setting", MR.POOLING_NAME, [0])], KR_EINVAL, **mkw)
    refused(check, bert + COLBERT + FIN + [SPARSE[0]], KR_EINVAL, "finalized without", **bkw)
    # another free dimension: refused naming it; the default of the pooling setting is a no-op, another value is refused
    refused(check, bert + CLS + FIN + [("tensor", R.HEAD[2], H)], KR_EINVAL, "L = 1", **bkw)
    refused(check, bert + CLS + FIN + [("tensor", R.HEAD[3], 1)], KR_EINVAL, **bkw)
    refused(check, modern + MCLS + FIN + [("tensor", MR.HEAD[4], H)], KR_EINVAL, "L = 1", **mkw)
    refused(check, bert + COLBERT + FIN + [("tensor", M3.HEADS[0], 256 * H)], KR_EINVAL, "P = 256", **bkw)
    refused(check, bert + COLBERT + FIN + [("tensor", M3.HEADS[1], 256)], KR_EINVAL, **bkw)
    refused(check, t5 + DENSE + FIN + [("tensor", "dense.weight", 12 * H)], KR_EINVAL, "finalize", **tkw)
    assert check(modern + MCLS + FIN + [("setting", MR.POOLING_NAME, [0])], **mkw)[-1]["rc"] == 0
    refused(check, modern + MCLS + FIN + [("setting", MR.POOLING_NAME, [1])], KR_EINVAL, MR.POOLING_NAME, **mkw)
    with_mean = modern + MCLS + [("setting", MR.POOLING_NAME, [1])] + FIN
    assert check(with_mean + [("setting", MR.POOLING_NAME, [1])], **mkw)[-1]["rc"] == 0
    refused(check, with_mean + [("setting", MR.POOLING_NAME, [0])], KR_EINVAL, **mkw)
    # an optional tensor of ModernBert's head may arrive after a finalize without it
    late = modern + [ln for ln in MCLS if ln[1] in MR.HEAD_REQUIRED] + FIN + [ln for ln in MCLS if ln[1] not in MR.HEAD_REQUIRED] + FIN
    assert all(d["rc"] == 0 for d in check(late, **mkw))


# ---------------------------------------------------------------------------------------------------------
# what a pool runs on a plan (resolve_pool): the forward and the result copy read this one table
# ---------------------------------------------------------------------------------------------------------
POOL_MEAN, POOL_CLS, POOL_CLASSIFY, POOL_SPLADE, POOL_LAST = 0, 1, 2, 4, 5
# pool -> (pack, select, classify, score, splade, one_row); select None: a splade forward does not pool
POOLS_COMMON = {POOL_MEAN: (POOL_MEAN, POOL_MEAN, 0, 0, 0, 0), POOL_CLS: (POOL_CLS, POOL_CLS, 0, 0, 0, 1), POOL_SPLADE: (POOL_MEAN, None, 0, 0, 1, 0),
                POOL_LAST: (POOL_MEAN, POOL_LAST, 0, 0, 0, 0)}
CLASSIFY_CLS_ROW, CLASSIFY_MEAN, CLASSIFY_SCORE = (POOL_CLS, POOL_CLS, 1, 0, 0, 1), (POOL_MEAN, POOL_MEAN, 1, 0, 0, 0), (POOL_MEAN, POOL_LAST, 1, 1, 0, 1)


def decoder_with_score_head(heads=4):
    """a decoder handle (config.decoder_attention, the Qwen2 / Llama names) with score.weight [3, H]"""
    t = [("embed_tokens.weight", V * H), ("norm.weight", H)]
    for l in range(L):
        p = "layers.%d." % l
        t += [(p + "input_layernorm.weight", H), (p + "post_attention_layernorm.weight", H)] + [(p + "mlp.%s_proj.weight" % x, FF * H) for x in ("gate", "up", "down")]
        t += [(p + "self_attn.%s_proj.weight" % x, H * H) for x in "qkvo"]
    lines = [("setting", "config.rotary_inv_freq", [0.5] * (H // heads // 2)), ("setting", "config.decoder_attention", [1.0])]
    return lines + [("tensor", n, k) for n, k in t] + [("tensor", "score.weight", 3 * H)], dict(heads=heads, type_vocab=1)


@pytest.mark.parametrize("plan,classify", [("bert+cls", CLASSIFY_CLS_ROW), ("modernbert+head", CLASSIFY_CLS_ROW), ("modernbert+head+mean", CLASSIFY_MEAN),
                                           ("decoder+score", CLASSIFY_SCORE)])
def test_resolve_pool_table(check, plan, classify):
    if plan == "bert+cls":
        lines, kw = script("bert", extra=CLS)
    elif plan.startswith("modernbert"):
        lines, kw = script("modernbert", extra=MCLS + ([("setting", MR.POOLING_NAME, [1])] if plan.endswith("+mean") else []))
    else:
        lines, kw = decoder_with_score_head()
    out = check(lines + FIN + [("pools",)], **kw)
    assert all(d["rc"] == 0 for d in out), [d for d in out if d["rc"]]
    want = dict(POOLS_COMMON)
    want[POOL_CLASSIFY] = classify
    for pool, row in want.items():
        got = tuple(int(x) for x in out[-1]["pool%d" % pool].split(","))
        assert len(got) == 6 and all(g == w for g, w in zip(got, row) if w is not None), (plan, pool, got, row)
    assert check([("pools",)])[-1]["rc"] == KR_ESTATE      # nothing finalized: no plan to resolve
