"""Decoder-LLM embedders without a GPU: name resolution and describe() for a DECODER handle (tests/capi/encoder_model_check.cpp), the unchanged ABI, the exact
KV expansion against HF on the CPU, every refusal of check_decoder_config from a folder holding only config.json, and the pooling precedence."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL, KR_ESTATE = -22, -1
H, L, HEADS, FF, V = 128, 2, 4, 256, 200
DECODER, NOMIC = 7, 3
ROT = ("setting", "config.rotary_inv_freq", [0.5] * (H // HEADS // 2))
DEC = ("setting", D.SETTING, [1.0])


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decoder_model") / "encoder_model_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "encoder_model_check.cpp"), "-o", exe])

    def run(lines, max_pos=512, type_vocab=1):
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


def _tensors(bias, prefix=""):
    t = [(prefix + "embed_tokens.weight", V * H), (prefix + "norm.weight", H)]
    for l in range(L):
        p = "%slayers.%d." % (prefix, l)
        t += [(p + "input_layernorm.weight", H), (p + "post_attention_layernorm.weight", H), (p + "mlp.gate_proj.weight", FF * H), (p + "mlp.up_proj.weight", FF * H),
              (p + "mlp.down_proj.weight", FF * H)]
        t += [(p + "self_attn.%s_proj.weight" % x, H * H) for x in "qkvo"]
        if bias:
            t += [(p + "self_attn.%s_proj.bias" % x, H) for x in "qkv"]
    return [("tensor", n, k) for n, k in t]


@pytest.mark.parametrize("bias,prefix", [(True, ""), (False, ""), (True, "model.")])
def test_a_decoder_plan_from_qwen2_and_llama_names(check, bias, prefix):
    out = check([ROT, DEC] + _tensors(bias, prefix) + [("finalize",)])
    assert all(d["rc"] == 0 for d in out), out
    plan = out[-1]
    # pre-LN, RMS, rotary positions (2), SwiGLU (1) gated, EPI_QKV_ROTB (2) with biases else EPI_QKV_ROT (1), AM_CAUSAL (4) in every layer, no head
    assert (plan["family"], plan["pre_ln"], plan["rms"], plan["pos"], plan["ff"], plan["ff_gated"]) == (str(DECODER), "1", "1", "2", "1", "1"), plan
    assert plan["qkv"] == ("2" if bias else "1") * L and plan["attn"] == "4" * L and plan["heads"] == "000000" and plan["out_dim"] == str(H)
    by = {ln[1]: d for ln, d in zip([ROT, DEC] + _tensors(bias, prefix), out)}
    assert by[prefix + "layers.0.input_layernorm.weight"]["slot"] == "3"                                   # T_ELNG, as T5's block 0 norm
    assert int(by[prefix + "layers.1.input_layernorm.weight"]["slot"]) == 5 + 14                           # L_LN2G of layer 0: applied behind its MLP
    assert int(by[prefix + "norm.weight"]["slot"]) == 5 + (L - 1) * 17 + 14                                # L_LN2G of the last layer
    assert by[prefix + "layers.0.self_attn.q_proj.weight"]["family"] == str(NOMIC)                         # NomicBert's rows, shared
    # value 0: the same stack, plain attention
    out0 = check([ROT, ("setting", D.SETTING, [0.0])] + _tensors(bias, prefix) + [("finalize",)])
    assert out0[-1]["rc"] == 0 and out0[-1]["attn"] == "0" * L and out0[-1]["family"] == str(DECODER)


def test_refusals_of_the_setting(check):
    t = _tensors(True)
    def last(lines, **kw):
        out = check(lines, **kw)
        assert all(d["rc"] == 0 for d in out[:-1]), out
        return out[-1]
    d = last([DEC] + t + [("finalize",)])
    assert d["rc"] == KR_EINVAL and "without config.rotary_inv_freq" in d["msg"]
    for other in (("setting", "config.position_padding_idx", [1.0]), ("setting", "config.local_attention_layers", [0.0] * L), ("setting", "config.t5_feed_forward", [1.0]),
                  ("setting", "config.attention_half_window", [8.0]), ("setting", "config.deberta_position_buckets", [32.0]),
                  ("tensor", "encoder.relative_attention_bias.weight", 32 * HEADS)):
        d = last([ROT, DEC, other] + t + [("finalize",)])
        assert d["rc"] == KR_EINVAL and "a handle has one position scheme" in d["msg"], (other, d)
    for bad in (2.0, -1.0, 0.5):
        d = last([ROT, ("setting", D.SETTING, [bad])])
        assert d["rc"] == KR_EINVAL and "0 (bidirectional) or 1 (causal)" in d["msg"]
    d = last([ROT, ("setting", D.SETTING, [1.0, 1.0])])
    assert d["rc"] == KR_EINVAL and "takes one value" in d["msg"]
    d = last([("setting", "config.no_such_setting", [1.0])])
    assert d["rc"] == KR_EINVAL and "unknown setting" in d["msg"] and d["msg"].rstrip(")").endswith(D.SETTING)      # appended: the order before it is unchanged
    # fixed at the first finalize
    d = last([ROT, DEC] + t + [("finalize",), ("setting", D.SETTING, [0.0])])
    assert d["rc"] == KR_EINVAL and "fixed at the handle's first finalize" in d["msg"]
    d = last([ROT, DEC] + t + [("finalize",), DEC])
    assert d["rc"] == 0
    # a head's tensors, a NomicBert-only or BERT name, a missing tensor
    for name, numel, frag in (("classifier.dense.weight", H * H, "'classifier.*' on a decoder handle"), ("dense.weight", 64 * H, "on a decoder handle"),
                              ("colbert_linear.weight", 128 * H, "on a decoder handle"), ("cls.predictions.transform.dense.weight", H * H, "on a decoder handle"),
                              ("head.dense.weight", H * H, "on a decoder handle"), ("layers.0.post_mlp_layernorm.weight", H, "on a decoder handle (config.decoder_attention)"),
                              ("layers.0.post_attention_layernorm.bias", H, "on a decoder handle (config.decoder_attention)"),
                              ("embeddings.token_type_embeddings.weight", H, "on a decoder handle (config.decoder_attention)")):
        d = last([ROT, DEC] + t + [("tensor", name, numel), ("finalize",)])
        assert d["rc"] == KR_EINVAL and frag in d["msg"], (name, d)
    d = last([ROT, DEC] + [x for x in t if x[1] != "norm.weight"] + [("finalize",)])
    assert d["rc"] == KR_ESTATE and "never loaded" in d["msg"]
    # the decoders' own rows on a handle without the setting
    d = last([ROT] + t + [("finalize",)])
    assert d["rc"] == KR_EINVAL and "config.decoder_attention was never loaded" in d["msg"]


def test_nomic_handles_resolve_and_refuse_as_before(check):
    """the shared names without the new setting: a NomicBert plan word for word as before, and the same refusals"""
    import nomic_util as N
    w = N.weights(H, L, HEADS, FF, V)
    lines = [ROT] + [("tensor", k, v.size) for k, v in w.items()] + [("finalize",)]
    out = check(lines, type_vocab=2)
    assert all(d["rc"] == 0 for d in out), out
    assert (out[-1]["family"], out[-1]["pre_ln"], out[-1]["rms"], out[-1]["attn"], out[-1]["qkv"], out[-1]["ff"]) == (str(NOMIC), "0", "0", "0" * L, "1" * L, "1")
    noset = check([ln for ln in lines if ln[0] != "setting"], type_vocab=2)
    assert noset[-1]["rc"] == KR_EINVAL and noset[-1]["msg"] == "layer 0 holds tensors under NomicBert's names but config.rotary_inv_freq was never loaded: load it before kr_encoder_finalize"
    emb = check([ROT, ("tensor", "embeddings.norm.weight", H)])
    assert emb[-1]["family"] == "4" and emb[-1]["slot"] == "3"          # ModernBert's embedding norm is not captured by the decoders' norm.weight
    t5 = check([("tensor", "embed_tokens.weight", V * H)])
    assert t5[-1]["family"] == "5" and t5[-1]["slot"] == "0"             # T5's row still takes the whole name


def test_abi_is_unchanged_and_the_header_names_the_feature():
    from kirag_amd import _lib
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert re.search(r"#define KR_ABI_VERSION 9\b", hdr) and _lib.ABI_VERSION == 9
    funcs = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert len(funcs) == 50 and len(_lib.SIGNATURES) == 50
    assert re.search(r"#define KR_POOL_LAST 5\b", hdr) and '"config.decoder_attention"' in hdr and _lib.POOL_LAST == 5
    for name in ("input_layernorm", "self_attn.{q,k,v}_proj.bias", "norm.weight", "embed_tokens.weight"):
        assert name in hdr, name
    from kirag_amd.retriever.retrievers import RETRIEVER_MAP
    assert set(RETRIEVER_MAP) == {"E5Retriever", "BGERetriever"}


@pytest.mark.parametrize("kind", ["qwen2-32", "llama-64", "qwen2-384"])
def test_kv_expansion_is_exact(kind):
    """HF with the checkpoint's KV heads against the same model with expand_kv's weights on heads KV heads: last_hidden_state equal to the last bit"""
    from kirag_amd.retriever.encoders import expand_kv
    cfg = D.hf_config(kind)
    w = D.weights(cfg)
    heads, kv = cfg.num_attention_heads, cfg.num_key_value_heads
    big = {k: expand_kv(k, v, heads, kv) for k, v in w.items()}
    d = cfg.hidden_size // heads
    for k, v in w.items():
        grown = "self_attn.k_proj" in k or "self_attn.v_proj" in k
        assert big[k].shape[0] == (heads * d if grown else v.shape[0]) and (grown or big[k] is v)
    k0 = w["layers.0.self_attn.k_proj.weight"].reshape(kv, d, -1)
    assert np.array_equal(big["layers.0.self_attn.k_proj.weight"].reshape(heads, d, -1), np.repeat(k0, heads // kv, axis=0))
    ids, mask = D.tokens(3, 24, "L", 4, holes=2)
    a = D.hf_last_hidden(D.hf_model(cfg, w), ids, mask)
    b = D.hf_last_hidden(D.hf_model(D.expanded_config(cfg), big), ids, mask)
    assert np.array_equal(a, b)
    t = torch.from_numpy(w["layers.0.self_attn.v_proj.weight"])
    assert torch.equal(expand_kv("model.layers.0.self_attn.v_proj.weight", t, heads, kv), torch.from_numpy(big["layers.0.self_attn.v_proj.weight"]))


BASE = dict(model_type="qwen2", hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=256, vocab_size=200,
            max_position_embeddings=32768, rms_norm_eps=1e-6, hidden_act="silu")
LLAMA = dict(BASE, model_type="llama", head_dim=32)
REFUSED = [
    (dict(LLAMA, head_dim=64), "head_dim=64"), (dict(BASE, num_attention_heads=1, num_key_value_heads=1), "head_dim=128"),
    (dict(BASE, num_attention_heads=8, num_key_value_heads=2), "head_dim=16"), (dict(BASE, hidden_size=192, num_attention_heads=6), "hidden_size=192"),
    (dict(BASE, hidden_size=2560, num_attention_heads=40), "hidden_size=2560"), (dict(BASE, intermediate_size=200), "intermediate_size=200"),
    (dict(BASE, hidden_act="gelu"), "hidden_act='gelu'"), (dict(BASE, num_key_value_heads=3), "num_key_value_heads=3"),
    (dict(LLAMA, attention_bias=True), "attention_bias=True"), (dict(LLAMA, mlp_bias=True), "mlp_bias=True"),
    (dict(BASE, use_sliding_window=True, sliding_window=64, max_window_layers=1), "sliding"),
    (dict(BASE, model_type="mistral", head_dim=32, sliding_window=1024), "sliding_window=1024"),
    (dict(BASE, layer_types=["full_attention", "sliding_attention"]), "sliding"),
    (dict(LLAMA, rope_parameters={"rope_type": "yarn", "rope_theta": 10000.0, "factor": 4.0, "original_max_position_embeddings": 2048}), "attention_scaling"),
]


@pytest.mark.parametrize("cfg,field", REFUSED, ids=[f for _, f in REFUSED])
def test_refusals_from_config_json_alone(tmp_path, cfg, field):
    """NotImplementedError beginning model_type='<type>': and naming the field, from a folder that holds config.json and nothing else (no weight is read)"""
    from kirag_amd.retriever.encoders import BGEEncoder, E5Encoder
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    for cls in (E5Encoder, BGEEncoder):
        with pytest.raises(NotImplementedError) as ei:
            cls.from_pretrained(str(tmp_path))
        assert str(ei.value).startswith(f"model_type={cfg['model_type']!r}:") and field in str(ei.value), ei.value


def test_accepted_configs_and_max_pos():
    from kirag_amd.retriever.encoders import check_decoder_config
    for cfg in (BASE, LLAMA, dict(BASE, model_type="mistral", head_dim=32, sliding_window=None), dict(BASE, model_type="mistral", head_dim=32, sliding_window=8192),
                dict(LLAMA, rope_parameters={"rope_type": "llama3", "rope_theta": 500000.0, "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                             "original_max_position_embeddings": 8192})):
        d = check_decoder_config(dict(cfg))
        assert d["max_pos"] == 8192 and d["inv_freq"].numel() == 16 and d["kv_heads"] == 2
    assert check_decoder_config(dict(BASE, max_position_embeddings=2048))["max_pos"] == 2048


def test_pooling_precedence(tmp_path):
    """kwarg > 1_Pooling/config.json > class default (E5 -> mean, BGE -> last); other modes are refused; train() mode pools in torch like the library"""
    from kirag_amd.retriever import encoders as ENC
    cfg = D.hf_config("qwen2-32")
    m = D.hf_model(cfg, D.weights(cfg))
    td = str(tmp_path / "m")
    m.save_pretrained(td)
    e5, bge = ENC.E5Encoder.from_pretrained(td), ENC.BGEEncoder.from_pretrained(td)
    assert type(e5) is ENC.Qwen2E5Encoder and e5.pooling == "mean" and type(bge) is ENC.Qwen2BGEEncoder and bge.pooling == "last"
    assert type(ENC.DecoderE5Encoder.from_pretrained(td)) is ENC.Qwen2E5Encoder
    os.makedirs(os.path.join(td, "1_Pooling"))
    def pooling_file(**modes):
        with open(os.path.join(td, "1_Pooling", "config.json"), "w") as f:
            json.dump(dict({"word_embedding_dimension": 128, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False, "pooling_mode_lasttoken": False}, **modes), f)
    pooling_file(pooling_mode_lasttoken=True)
    assert ENC.E5Encoder.from_pretrained(td).pooling == "last" and ENC.E5Encoder.from_pretrained(td, pooling="mean").pooling == "mean"
    pooling_file(pooling_mode_mean_tokens=True)
    assert ENC.BGEEncoder.from_pretrained(td).pooling == "mean" and ENC.BGEEncoder.from_pretrained(td, pooling="last").pooling == "last"
    pooling_file(pooling_mode_cls_token=True)
    with pytest.raises(NotImplementedError, match="pooling_mode_cls_token"):
        ENC.BGEEncoder.from_pretrained(td)
    with pytest.raises(ValueError, match="pooling='first'"):
        ENC.BGEEncoder.from_pretrained(td, pooling="first")
    # train() mode: HF's own causal forward + the pooling
    ids, mask = D.tokens(3, 16, "L", 2, holes=1)
    lh = D.hf_last_hidden(m, ids, mask)
    for enc, pool in ((e5, D.POOL_MEAN), (bge, D.POOL_LAST)):
        enc.train()
        out = enc(torch.from_numpy(ids), torch.from_numpy(mask)).detach().numpy()
        assert np.abs(out - D.pool_np(lh, mask, pool)).max() <= 2e-6
    # llama and mistral folders reach their own twins
    for kind, twin in (("llama-32", ENC.LlamaBGEEncoder),):
        c2 = D.hf_config(kind)
        t2 = str(tmp_path / kind)
        D.hf_model(c2, D.weights(c2)).save_pretrained(t2)
        assert type(ENC.BGEEncoder.from_pretrained(t2)) is twin
