"""EuroBERT and the bidirectional switch of the decoder embedders without a GPU: EuroBertModel's state dict finalizes to a DECODER plan with plain attention
(tests/capi/encoder_model_check.cpp, as it is), check_decoder_config's refusals for model_type eurobert from a folder holding only config.json, the dispatch and
the pooling rules of the EuroBERT twins, the ``attention=`` kwarg of the Qwen2 / Llama / Mistral twins with its round trip, and train() mode against HF."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_util as D  # noqa: E402
import eurobert_util as U  # noqa: E402
from test_jina3_host import check  # noqa: E402,F401  (the stand-alone checker, built once per module)

KR_EINVAL = -22
L = 2


def test_state_dict_names_are_hfs_own_and_plan_is_a_bidirectional_decoder(check):  # noqa: F811
    from transformers import EuroBertModel
    cfg = U.hf_config("euro-64", L=L)
    w = U.weights(cfg)
    assert set(EuroBertModel(cfg).state_dict().keys()) == set(w.keys())
    lines = [("setting", D.INV_FREQ_NAME, [0.5] * 32), ("setting", D.SETTING, [0.0])] + [("tensor", k, v.size) for k, v in w.items()] + [("finalize",)]
    out = check(lines, type_vocab=1)
    assert all(d["rc"] == 0 for d in out), out
    plan = out[-1]
    # family 7, pre-LN, RMS, rotary, SwiGLU gated, EPI_QKV_ROT (no bias), AM_PLAIN (0) in every layer; k / v came as [64, 128]: grouped-query, native
    assert (plan["family"], plan["pre_ln"], plan["rms"], plan["pos"], plan["ff"], plan["ff_gated"], plan["qkv"], plan["attn"], plan["heads"]) == \
           ("7", "1", "1", "2", "1", "1", "1" * L, "0" * L, "000000"), plan


BASE = dict(model_type="eurobert", hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=256, vocab_size=200,
            max_position_embeddings=8192, rms_norm_eps=1e-5, hidden_act="silu", pad_token_id=0, bos_token_id=1, eos_token_id=2, mask_token_id=3)
REFUSED = [
    (dict(BASE, hidden_act="gelu"), "hidden_act='gelu'"), (dict(BASE, attention_bias=True), "attention_bias=True"), (dict(BASE, mlp_bias=True), "mlp_bias=True"),
    (dict(BASE, head_dim=64), "head_dim=64"), (dict(BASE, num_attention_heads=1, num_key_value_heads=1), "head_dim=128"),
    (dict(BASE, num_attention_heads=8, num_key_value_heads=2), "head_dim=16"), (dict(BASE, num_key_value_heads=3), "num_key_value_heads=3"),
    (dict(BASE, hidden_size=2304, num_attention_heads=36, num_key_value_heads=6), "hidden_size=2304"), (dict(BASE, intermediate_size=200), "intermediate_size=200"),
    (dict(BASE, rope_parameters={"rope_type": "yarn", "rope_theta": 10000.0, "factor": 4.0, "original_max_position_embeddings": 2048}), "attention_scaling"),
]


@pytest.mark.parametrize("cfg,field", REFUSED, ids=[f for _, f in REFUSED])
def test_refusals_from_config_json_alone(tmp_path, cfg, field):
    """NotImplementedError beginning model_type='eurobert': and naming the field, from a folder that holds config.json and nothing else"""
    from kirag_amd.retriever.encoders import BGEEncoder, E5Encoder
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    for cls in (E5Encoder, BGEEncoder):
        with pytest.raises(NotImplementedError) as ei:
            cls.from_pretrained(str(tmp_path))
        assert str(ei.value).startswith("model_type='eurobert':") and field in str(ei.value), ei.value


def test_accepted_configs():
    from kirag_amd.retriever.encoders import check_decoder_config, kv_for_library
    d = check_decoder_config(dict(BASE))
    assert d["max_pos"] == 8192 and d["inv_freq"].numel() == 16 and (d["heads"], d["kv_heads"]) == (4, 2) and d["ln_eps"] == 1e-5
    # EuroBERT-210m (12 x 64) and -610m (18 x 64 over 6 KV heads: A = 384, native)
    assert check_decoder_config(dict(BASE, hidden_size=768, num_attention_heads=12, num_key_value_heads=12, intermediate_size=3072))["kv_heads"] == 12
    d = check_decoder_config(dict(BASE, hidden_size=1152, num_attention_heads=18, num_key_value_heads=6, intermediate_size=4096))
    assert d["kv_heads"] == 6 and d["inv_freq"].numel() == 32
    k = np.zeros((384, 1152), np.float32)
    assert kv_for_library("layers.0.self_attn.k_proj.weight", k, 18, 6, 1152) is k
    # A = 32 (4 heads of 32 over 1 KV head) is expanded
    k = np.zeros((32, 128), np.float32)
    assert kv_for_library("layers.0.self_attn.k_proj.weight", k, 4, 1, 128).shape == (128, 128)


def test_dispatch_pooling_and_train_mode(tmp_path):
    """E5Encoder / BGEEncoder reach the EuroBERT twins, which both pool the mean; the kwarg and 1_Pooling keep their precedence and "last" stays available;
    "cls" and a causal mask are refused by name; save_pretrained -> from_pretrained keeps pooling; train() mode is HF's forward + the pooling"""
    from kirag_amd.retriever import encoders as ENC
    cfg = U.hf_config("euro-32")
    m = U.hf_model(cfg, U.weights(cfg))
    td = str(tmp_path / "m")
    m.save_pretrained(td)
    e5, bge = ENC.E5Encoder.from_pretrained(td), ENC.BGEEncoder.from_pretrained(td)
    assert type(e5) is ENC.EuroBertE5Encoder and type(bge) is ENC.EuroBertBGEEncoder and isinstance(bge, ENC.EuroBertModel)
    assert e5.pooling == "mean" and bge.pooling == "mean" and e5.attention == "bidirectional" and bge._decoder_attention == 0.0
    assert type(ENC.DecoderBGEEncoder.from_pretrained(td)) is ENC.EuroBertBGEEncoder
    last = ENC.BGEEncoder.from_pretrained(td, pooling="last")
    assert last.pooling == "last" and ENC.E5Encoder.from_pretrained(td, attention="bidirectional").attention == "bidirectional"
    with pytest.raises(ValueError, match="pooling='cls'.*KR_POOL_CLS on decoder handles"):
        ENC.BGEEncoder.from_pretrained(td, pooling="cls")
    with pytest.raises(ValueError, match="attention='causal'.*EuroBERT"):
        ENC.E5Encoder.from_pretrained(td, attention="causal")
    td2 = str(tmp_path / "again")
    last.save_pretrained(td2)
    again = ENC.E5Encoder.from_pretrained(td2)
    assert type(again) is ENC.EuroBertE5Encoder and again.pooling == "last" and again.attention == "bidirectional"
    assert ENC.E5Encoder.from_pretrained(td2, pooling="mean").pooling == "mean"
    with open(os.path.join(td2, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": 128, "pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}, f)
    with pytest.raises(NotImplementedError, match="pooling_mode_cls_token"):
        ENC.E5Encoder.from_pretrained(td2)
    ids, mask = U.tokens(3, 16, "L", 2, holes=1)
    lh = U.hf_last_hidden(m, ids, mask)
    for enc, pool in ((e5, U.POOL_MEAN), (last, U.POOL_LAST)):
        enc.train()
        out = enc(torch.from_numpy(ids), torch.from_numpy(mask)).detach().numpy()
        assert np.abs(out - U.pool_np(lh, mask, pool)).max() <= 1e-6


def test_the_bidirectional_switch_of_the_decoder_twins(tmp_path):
    """attention="bidirectional" on a Qwen2 folder: the default stays causal, the choice travels through save_pretrained / from_pretrained, the kwarg wins over
    the file, anything else is refused by name, and train() mode equals Qwen2Model under the all-admitting 4-D mask (and differs from the causal forward)"""
    from kirag_amd.retriever import encoders as ENC
    cfg = D.hf_config("qwen2-32")
    m = D.hf_model(cfg, D.weights(cfg))
    td = str(tmp_path / "q")
    m.save_pretrained(td)
    causal, bi = ENC.E5Encoder.from_pretrained(td), ENC.E5Encoder.from_pretrained(td, attention="bidirectional")
    assert type(bi) is ENC.Qwen2E5Encoder and causal.attention == "causal" and causal._decoder_attention == 1.0 and bi.attention == "bidirectional" and bi._decoder_attention == 0.0
    with pytest.raises(ValueError, match="attention='prefix'"):
        ENC.E5Encoder.from_pretrained(td, attention="prefix")
    td2 = str(tmp_path / "again")
    bi.save_pretrained(td2)
    with open(os.path.join(td2, "1_Pooling", "attention.json")) as f:
        assert json.load(f) == {"attention": "bidirectional"}
    with open(os.path.join(td2, "1_Pooling", "config.json")) as f:
        assert "attention" not in json.load(f)                     # sentence-transformers' Pooling module takes that file's keys as arguments
    again = ENC.BGEEncoder.from_pretrained(td2)
    assert again.attention == "bidirectional" and again.pooling == "mean"
    assert ENC.BGEEncoder.from_pretrained(td2, attention="causal").attention == "causal"
    td3 = str(tmp_path / "causal")
    causal.save_pretrained(td3)
    assert ENC.E5Encoder.from_pretrained(td3).attention == "causal"
    ids, mask = D.tokens(3, 16, "L", 2, holes=1)
    ref = D.pool_np(D.hf_last_hidden(m, ids, mask, "none"), mask, D.POOL_MEAN)
    ref_causal = D.pool_np(D.hf_last_hidden(m, ids, mask), mask, D.POOL_MEAN)
    for enc, want in ((bi, ref), (again, ref), (causal, ref_causal)):
        enc.train()
        out = enc(torch.from_numpy(ids), torch.from_numpy(mask)).detach().numpy()
        assert np.abs(out - want).max() <= 1e-6
    assert np.abs(ref - ref_causal).max() > 1e-2
