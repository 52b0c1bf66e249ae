"""jina-embeddings-v3 without a GPU: name resolution and describe() for a ROTARY_BERT handle (tests/capi/encoder_model_check.cpp, as it is), the rules of
config.rotary_feed_forward, NomicBert and decoder handles unchanged, every refusal of check_jina3_config from a folder holding only config.json, the dispatch,
the save / load round trip and train() mode against HF."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jina3_util as J  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL, KR_ESTATE = -22, -1
H, L, HEADS, FF, V = 128, 2, 2, 256, 200
NOMIC, DECODER, ROTARY_BERT = 3, 7, 8
ROT = ("setting", J.INV_FREQ_NAME, [0.5] * (H // HEADS // 2))
RFF = ("setting", J.SETTING, [1.0])
DEC = ("setting", "config.decoder_attention", [1.0])


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jina3_model") / "encoder_model_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "encoder_model_check.cpp"), "-o", exe])

    def run(lines, max_pos=512, type_vocab=2):
        text = ["config %d %d %d %d %d %d %d" % (H, L, HEADS, FF, V, max_pos, type_vocab)]
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


def _last(check, lines, **kw):
    out = check(lines, **kw)
    assert all(d["rc"] == 0 for d in out[:-1]), out
    return out[-1]


def _tensors(drop=()):
    """the state dict of JinaEmbeddingsV3Model (tiny shape) as checker lines, without the names that contain one of `drop`"""
    w = J.weights(J.hf_config("jina-64", L=L))
    return [("tensor", k, v.size) for k, v in w.items() if not any(d in k for d in drop)]


def test_state_dict_names_are_hfs_own():
    cfg = J.hf_config("jina-64")
    from transformers import JinaEmbeddingsV3Model
    assert set(JinaEmbeddingsV3Model(cfg).state_dict().keys()) == set(J.weights(cfg).keys())


def test_a_jina3_state_dict_finalizes_to_family_8(check):
    lines = [ROT, RFF] + _tensors() + [("finalize",)]
    out = check(lines)
    assert all(d["rc"] == 0 for d in out), out
    plan = out[-1]
    # post-LN, LayerNorm, rotary positions (2), GELU (0) ungated, EPI_QKV_ROTB (2), AM_PLAIN (0) in every layer, no head
    assert (plan["family"], plan["pre_ln"], plan["rms"], plan["pos"], plan["ff"], plan["ff_gated"]) == (str(ROTARY_BERT), "0", "0", "2", "0", "0"), plan
    assert plan["qkv"] == "2" * L and plan["attn"] == "0" * L and plan["heads"] == "000000" and plan["out_dim"] == str(H)
    by = {ln[1]: d for ln, d in zip(lines[:-1], out)}
    assert by["layers.0.self_attn.q_proj.weight"]["family"] == str(NOMIC)          # the rotary packed-row order
    assert by["layers.0.self_attn.q_proj.bias"]["family"] == str(DECODER)          # ... and the bias in the same order
    assert by["layers.1.mlp.fc1.weight"]["family"] == str(ROTARY_BERT) and int(by["layers.1.mlp.fc1.weight"]["slot"]) == 5 + 17 + 10       # L_IW, plain row order
    assert int(by["layers.0.mlp.fc1.bias"]["slot"]) == 5 + 11 and int(by["layers.0.mlp.fc2.weight"]["slot"]) == 5 + 12 and int(by["layers.0.mlp.fc2.bias"]["slot"]) == 5 + 13
    assert int(by["layers.0.self_attn.o_proj.bias"]["slot"]) == 5 + 7
    assert by["pooler.dense.weight"]["slot"] == "-1"                                # ignored


@pytest.mark.parametrize("drop,qkv", [((), "22"), (("q_proj.bias",), "22"), (("k_proj.bias",), "22"), (("q_proj.bias", "k_proj.bias"), "11"),
                                      (("layers.1.self_attn.q_proj.bias", "layers.1.self_attn.k_proj.bias"), "21"), ((".bias",), None)])
def test_qkv_is_rot_bias_iff_a_q_or_k_bias_was_sent(check, drop, qkv):
    """every bias is optional; a layer rotates with EPI_QKV_ROTB iff a q or k bias was loaded.  (Dropping every '.bias' drops the norms' too: never loaded.)"""
    d = _last(check, [ROT, RFF] + _tensors(drop) + [("finalize",)])
    if qkv is None:
        assert d["rc"] == KR_ESTATE and "never loaded" in d["msg"]
        only_linear = [t for t in _tensors() if not (t[1].endswith(".bias") and "layernorm" not in t[1].lower())]
        d = _last(check, [ROT, RFF] + only_linear + [("finalize",)])
        assert d["rc"] == 0 and d["qkv"] == "11" and d["family"] == str(ROTARY_BERT)
    else:
        assert d["rc"] == 0 and d["qkv"] == qkv, d


def test_rules_of_the_setting(check):
    t = _tensors()
    for bad in (2.0, -1.0, 0.5):
        d = _last(check, [ROT, ("setting", J.SETTING, [bad])])
        assert d["rc"] == KR_EINVAL and J.SETTING in d["msg"] and "0 (SwiGLU) or 1 (gelu with biases)" in d["msg"]
    d = _last(check, [ROT, ("setting", J.SETTING, [1.0, 1.0])])
    assert d["rc"] == KR_EINVAL and "takes one value" in d["msg"]
    d = _last(check, [("setting", "config.no_such_setting", [1.0])])
    assert d["rc"] == KR_EINVAL and "unknown setting" in d["msg"] and J.SETTING in d["msg"]
    # fixed at the first finalize; the same value is a no-op
    d = _last(check, [ROT, RFF] + t + [("finalize",), ("setting", J.SETTING, [0.0])])
    assert d["rc"] == KR_EINVAL and "fixed at the handle's first finalize" in d["msg"]
    assert _last(check, [ROT, RFF] + t + [("finalize",), RFF])["rc"] == 0
    # value 1 needs the frequencies, and excludes every other scheme
    d = _last(check, [RFF] + t + [("finalize",)])
    assert d["rc"] == KR_EINVAL and "config.rotary_feed_forward = 1 without config.rotary_inv_freq" in d["msg"]
    for other in (("setting", "config.position_padding_idx", [1.0]), ("setting", "config.local_attention_layers", [0.0] * L), ("setting", "config.t5_feed_forward", [1.0]),
                  ("setting", "config.attention_half_window", [8.0]), ("setting", "config.deberta_position_buckets", [32.0]), DEC,
                  ("tensor", "encoder.relative_attention_bias.weight", 32 * HEADS)):
        d = _last(check, [ROT, RFF, other] + t + [("finalize",)])
        assert d["rc"] == KR_EINVAL and "config.rotary_feed_forward = 1 next to" in d["msg"] and "a handle has one position scheme" in d["msg"], (other, d)


def test_refusals_name_the_tensor(check):
    t = _tensors()
    fc = [x for x in t if "mlp.fc1" not in x[1]]
    # gate_proj / up_proj on a handle with the setting
    for name in ("layers.0.mlp.gate_proj.weight", "layers.1.mlp.up_proj.weight"):
        d = _last(check, [ROT, RFF] + (fc if "gate" in name else t) + [("tensor", name, FF * H), ("finalize",)])
        assert d["rc"] == KR_EINVAL and f"'{name}'" in d["msg"] and "rotary BERT handle" in d["msg"], d
    # mlp.fc1 / mlp.fc2 / o_proj.bias on handles without it: a NomicBert handle (setting 0 and never set), a BERT handle
    import nomic_util as N
    nomic = [("tensor", k, v.size) for k, v in N.weights(H, L, HEADS, FF, V).items()]
    for name, numel in (("layers.0.mlp.fc1.bias", FF), ("layers.1.mlp.fc2.bias", H), ("layers.0.self_attn.o_proj.bias", H)):
        for pre in ([ROT], [ROT, ("setting", J.SETTING, [0.0])]):
            d = _last(check, pre + nomic + [("tensor", name, numel), ("finalize",)])
            assert d["rc"] == KR_EINVAL and f"'{name}'" in d["msg"] and "config.rotary_feed_forward = 1 was never loaded" in d["msg"], d
    d = _last(check, [ROT] + [x for x in nomic if "mlp.down_proj" not in x[1]] + [("tensor", "layers.%d.mlp.fc2.weight" % l, FF * H) for l in range(L)] + [("finalize",)])
    assert d["rc"] == KR_EINVAL and "'layers.0.mlp.fc2.weight'" in d["msg"]
    d = _last(check, [("tensor", "layers.0.mlp.fc1.weight", FF * H), ("finalize",)])
    assert d["rc"] == KR_EINVAL and "'layers.0.mlp.fc1.weight'" in d["msg"]
    # ... and on a decoder handle
    import test_decoder_host as TD
    d = _last(check, [ROT, DEC] + TD._tensors(True) + [("tensor", "layers.0.self_attn.o_proj.bias", H), ("finalize",)], type_vocab=1)
    assert d["rc"] == KR_EINVAL and "'layers.0.self_attn.o_proj.bias' on a decoder handle" in d["msg"]
    # grouped-query k / v tensors stay decoder-only
    gq = [x if "layers.0.self_attn.k_proj.weight" != x[1] else ("tensor", x[1], 64 * H) for x in t]
    d = _last(check, [ROT, RFF] + gq + [("finalize",)])
    assert d["rc"] == KR_EINVAL and "'layers.0.self_attn.k_proj.weight' with A = 64" in d["msg"] and "decoder handles only" in d["msg"]
    # the decoders' other names, BERT's spelling of a q bias, a head
    for name, numel, frag in (("layers.1.input_layernorm.weight", H, "on a rotary BERT handle"), ("norm.weight", H, "on a rotary BERT handle"),
                              ("encoder.layer.0.attention.self.query.bias", H, "on a rotary BERT handle"), ("classifier.dense.weight", H * H, "on a rotary BERT (jina-embeddings-v3) handle"),
                              ("colbert_linear.weight", 128 * H, "on a rotary BERT (jina-embeddings-v3) handle")):
        d = _last(check, [ROT, RFF] + [x for x in t if "layers.0.self_attn.q_proj.bias" != x[1]] + [("tensor", name, numel), ("finalize",)])
        assert d["rc"] == KR_EINVAL and frag in d["msg"], (name, d)
    d = _last(check, [ROT, RFF] + [x for x in t if x[1] != "layers.1.mlp.fc2.weight"] + [("finalize",)])
    assert d["rc"] == KR_ESTATE and "never loaded" in d["msg"]


def test_nomic_and_decoder_handles_plan_and_refuse_as_before(check):
    import nomic_util as N
    import test_decoder_host as TD
    w = N.weights(H, L, HEADS, FF, V)
    lines = [ROT] + [("tensor", k, v.size) for k, v in w.items()] + [("finalize",)]
    for pre in ([], [("setting", J.SETTING, [0.0])]):
        out = check(pre + lines)
        assert all(d["rc"] == 0 for d in out), out
        assert (out[-1]["family"], out[-1]["pre_ln"], out[-1]["rms"], out[-1]["attn"], out[-1]["qkv"], out[-1]["ff"], out[-1]["ff_gated"]) == (str(NOMIC), "0", "0", "0" * L, "1" * L, "1", "1")
    # 0 after the first finalize of a handle that never had the setting is a no-op; 1 is refused
    out = check(lines + [("setting", J.SETTING, [0.0]), ("setting", J.SETTING, [1.0])])
    assert out[-2]["rc"] == 0 and out[-1]["rc"] == KR_EINVAL and "after kr_encoder_finalize" in out[-1]["msg"]
    # a q bias on a NomicBert handle is still refused, in the words it had
    d = _last(check, lines[:-1] + [("tensor", "layers.0.self_attn.q_proj.bias", H), ("finalize",)])
    assert d["rc"] == KR_EINVAL and d["msg"] == "'layers.0.self_attn.q_proj.bias' but config.decoder_attention was never loaded: load it before kr_encoder_finalize"
    d = _last(check, lines[:-1] + [("tensor", "encoder.layer.0.attention.self.query.bias", H), ("finalize",)])
    assert d["rc"] == KR_EINVAL and d["msg"] == "layer 0: the q / k / gate / up projections of a NomicBert handle have no bias"
    for bias in (True, False):
        d = _last(check, [ROT, DEC] + TD._tensors(bias) + [("finalize",)], type_vocab=1)
        assert (d["family"], d["pre_ln"], d["rms"], d["pos"], d["ff"], d["ff_gated"], d["qkv"], d["attn"]) == (str(DECODER), "1", "1", "2", "1", "1", ("2" if bias else "1") * L, "4" * L)


BASE = dict(model_type="jina_embeddings_v3", hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=200,
            max_position_embeddings=8194, type_vocab_size=1, layer_norm_eps=1e-5, hidden_act="gelu")
REFUSED = [
    (dict(BASE, hidden_act="silu"), "hidden_act='silu'"), (dict(BASE, hidden_act="gelu_new"), "hidden_act='gelu_new'"),
    (dict(BASE, rope_parameters={"rope_type": "yarn", "rope_theta": 10000.0, "factor": 4.0, "original_max_position_embeddings": 2048}), "attention_scaling"),
    (dict(BASE, head_dim=32), "head_dim=32"), (dict(BASE, num_attention_heads=1), "head_dim=128"), (dict(BASE, num_attention_heads=8), "head_dim=16"),
    (dict(BASE, hidden_size=192, num_attention_heads=3), "hidden_size=192"), (dict(BASE, hidden_size=2560, num_attention_heads=40), "hidden_size=2560"),
    (dict(BASE, intermediate_size=200), "intermediate_size=200"),
]


@pytest.mark.parametrize("cfg,field", REFUSED, ids=[f for _, f in REFUSED])
def test_refusals_from_config_json_alone(tmp_path, cfg, field):
    """NotImplementedError beginning model_type='jina_embeddings_v3': and naming the field, from a folder that holds config.json and nothing else"""
    from kirag_amd.retriever.encoders import BGEEncoder, E5Encoder
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    for cls in (E5Encoder, BGEEncoder):
        with pytest.raises(NotImplementedError) as ei:
            cls.from_pretrained(str(tmp_path))
        assert str(ei.value).startswith("model_type='jina_embeddings_v3':") and field in str(ei.value), ei.value


def test_accepted_config_and_max_pos():
    from kirag_amd.retriever.encoders import check_jina3_config
    d = check_jina3_config(dict(BASE))
    assert d["max_pos"] == 8192 and d["inv_freq"].numel() == 32
    assert check_jina3_config(dict(BASE, max_position_embeddings=2048, num_attention_heads=4))["inv_freq"].numel() == 16
    m = J.hf_model(J.hf_config("jina-32"), J.weights(J.hf_config("jina-32")))
    assert torch.equal(check_jina3_config(m.config)["inv_freq"], m.rotary_emb.inv_freq)


def test_dispatch_round_trip_and_train_mode(tmp_path):
    """E5Encoder / BGEEncoder.from_pretrained reach the twins; save_pretrained -> from_pretrained keeps class and weights; train() mode is HF's forward + pooling"""
    from kirag_amd.retriever import encoders as ENC
    cfg = J.hf_config("jina-32")
    m = J.hf_model(cfg, J.weights(cfg))
    td = str(tmp_path / "m")
    m.save_pretrained(td)
    e5, bge = ENC.E5Encoder.from_pretrained(td), ENC.BGEEncoder.from_pretrained(td)
    assert type(e5) is ENC.JinaV3E5Encoder and type(bge) is ENC.JinaV3BGEEncoder and isinstance(e5, ENC.JinaEmbeddingsV3Model)
    assert e5._pool == J.POOL_MEAN and bge._pool == J.POOL_CLS and e5.embedding_size == cfg.hidden_size
    td2 = str(tmp_path / "again")
    bge.save_pretrained(td2)
    again = ENC.E5Encoder.from_pretrained(td2)
    assert type(again) is ENC.JinaV3E5Encoder
    sd, sd2 = m.state_dict(), again.state_dict()
    assert set(sd) == set(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    ids, mask = J.tokens(3, 16, "R", 2, holes=1)
    lh = J.hf_last_hidden(m, ids, mask)
    for enc, pool in ((e5, J.POOL_MEAN), (bge, J.POOL_CLS), (again, J.POOL_MEAN)):
        enc.train()
        out = enc(torch.from_numpy(ids), torch.from_numpy(mask)).detach().numpy()
        assert np.abs(out - J.pool_np(lh, mask, pool)).max() <= 1e-6
    e5.eval()
    with pytest.raises(RuntimeError, match="HIP path only"):      # no CPU fallback
        e5(torch.from_numpy(ids), torch.from_numpy(mask))
