"""Host-side tests of the T5 encoder support: the dispatch under the two registry names, the settings the Python layer derives from an HF T5Config, the
refusals that happen before a handle exists, the discovery of the sentence-transformers Dense head with its refusals and its round trip through
save_pretrained, the train()-mode forward, and the fences the C ABI keeps (same functions, the new names documented in the header)."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import t5_util as T  # noqa: E402

from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever.retrievers import RETRIEVER_MAP, load_retriever  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save_tiny(tmp_path, name="t5", ff=T.RELU):
    from transformers import T5EncoderModel
    torch.manual_seed(11)
    m = T5EncoderModel(T.hf_config(T.cfg(128, 2, 4, 256, 120, ff)))
    d = str(tmp_path / name)
    m.save_pretrained(d)
    return d, m


def test_dispatch_by_the_checkpoints_model_type(tmp_path):
    from transformers import BertModel, T5EncoderModel
    assert set(RETRIEVER_MAP) == {"E5Retriever", "BGERetriever"}
    assert RETRIEVER_MAP["E5Retriever"] is ENC.E5Encoder and RETRIEVER_MAP["BGERetriever"] is ENC.BGEEncoder
    for ff in (T.RELU, T.GATED):
        d, src = _save_tiny(tmp_path, "t5-" + ff, ff)
        for name, twin, pool in (("E5Retriever", ENC.T5E5Encoder, ENC.POOL_MEAN), ("BGERetriever", ENC.T5BGEEncoder, ENC.POOL_CLS)):
            e = load_retriever(name, d)
            assert type(e) is twin and isinstance(e, T5EncoderModel) and not isinstance(e, BertModel) and e._pool == pool and not e.training
            assert twin._hf_base is T5EncoderModel and e.dense is None and e.embedding_size == 128
            sd, ref = e.state_dict(), src.state_dict()
            assert set(sd) == set(ref)
            for k, v in ref.items():
                assert torch.equal(sd[k], v), k
            assert T.BIAS_NAME in sd and "shared.weight" in sd and "encoder.final_layer_norm.weight" in sd
            # what the weight sync walks: the tied embedding once, under its own name
            names = [n for n, _ in e.named_parameters()]
            assert "shared.weight" in names and "encoder.embed_tokens.weight" not in names
    for name in ("_hip_forward", "forward_packed", "invalidate_hip_weights", "train", "load_state_dict", "_apply", "forward", "hip_last_hidden_state"):
        assert getattr(ENC.T5E5Encoder, name) is getattr(ENC.E5Encoder, name), name
        assert getattr(ENC.T5BGEEncoder, name) is getattr(ENC.E5Encoder, name), name


def test_settings_come_from_the_hf_config():
    s = ENC.HipBertForward._t5_settings(T.hf_config(T.cfg(768, 12, 12, 3072, 32128)))
    assert s == {"hidden": 768, "layers": 12, "heads": 12, "intermediate": 3072, "max_pos": 512, "ln_eps": 1e-6, "feed_forward": 0.0}
    s = ENC.HipBertForward._t5_settings(T.hf_config(T.cfg(384, 3, 12, 1024, 1000, T.GATED)))
    assert s["feed_forward"] == 1.0 and s["heads"] == 12 and s["hidden"] == 384
    assert ENC.HipBertForward._t5_settings(T.cfg(768, 12, 12, 3072, 32128, n_positions=1024))["max_pos"] == 1024
    assert ENC.T5_SETTING == T.SETTING


@pytest.mark.parametrize("change,field", [
    (dict(d_kv=64, num_heads=6, d_model=512), "d_kv"),                # v1.1-small: inner width 384 != d_model 512
    (dict(d_kv=128, num_heads=6), "d_kv"),                            # t5-3b / 11b heads
    (dict(relative_attention_num_buckets=64), "relative_attention_num_buckets"),
    (dict(relative_attention_max_distance=256), "relative_attention_max_distance"),
    (dict(dense_act_fn="gelu", is_gated_act=False), "dense_act_fn"),
    (dict(dense_act_fn="relu", is_gated_act=True), "is_gated_act"),
    (dict(dense_act_fn="silu", is_gated_act=True), "dense_act_fn"),
    (dict(d_ff=1000), "d_ff"),
])
def test_what_the_kernels_do_not_compute_is_refused_before_a_handle_exists(change, field):
    """NotImplementedError naming the field, from the config alone: no GPU is needed and no handle is created (HipBertForward loads the built library first)"""
    c = T.cfg(768, 2, 12, 1024, 100)
    for k, v in change.items():
        setattr(c, k, v)
    with pytest.raises(NotImplementedError, match=field):
        ENC.HipBertForward._t5_settings(c)
    with pytest.raises(NotImplementedError, match=field):
        ENC.HipBertForward(c, 0)          # raises before kr_encoder_create_ex


def test_dense_head_is_discovered_and_survives_save_pretrained(tmp_path):
    d, src = _save_tiny(tmp_path)
    assert ENC.read_st_dense(d, 128) is None                       # no modules.json: no head
    W = T.dense_weight(64, 128)
    for fmt in ("safetensors", "bin"):
        d, src = _save_tiny(tmp_path, "t5-" + fmt)
        T.write_st_dense(d, W, fmt=fmt)
        got = ENC.read_st_dense(d, 128)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), W)
        e = load_retriever("E5Retriever", d)
        assert type(e) is ENC.T5E5Encoder and isinstance(e.dense, torch.nn.Linear) and e.dense.bias is None
        assert np.array_equal(e.dense.weight.detach().numpy(), W) and e.embedding_size == 64
        assert [n for n, _ in e.named_parameters()][-1] == "dense.weight"          # the weight sync loads it under this name
    # a folder written by the twin loads back with its head, and its transformer files are a plain T5EncoderModel checkpoint
    again = str(tmp_path / "again")
    e.save_pretrained(again)
    assert isinstance(e.dense, torch.nn.Linear)                    # still installed after saving
    from safetensors.torch import load_file
    from transformers import T5EncoderModel
    assert not [k for k in load_file(os.path.join(again, "model.safetensors")) if "dense" in k]
    _, info = T5EncoderModel.from_pretrained(again, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"], info
    b = load_retriever("BGERetriever", again)
    assert type(b) is ENC.T5BGEEncoder and np.array_equal(b.dense.weight.detach().numpy(), W)
    # modules.json without a Dense module: no head
    import json
    d, _ = _save_tiny(tmp_path, "t5-plain-st")
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}], f)
    assert load_retriever("E5Retriever", d).dense is None


@pytest.mark.parametrize("kw,field", [(dict(in_features=96), "in_features"), (dict(bias=True), "bias"),
                                      (dict(activation="torch.nn.modules.activation.Tanh"), "activation_function")])
def test_dense_heads_the_library_does_not_compute_are_refused(tmp_path, kw, field):
    d, _ = _save_tiny(tmp_path)
    T.write_st_dense(d, T.dense_weight(64, 128), **kw)
    with pytest.raises(NotImplementedError, match=field):
        load_retriever("E5Retriever", d)


def test_train_mode_forward_is_hfs_with_pooling_dense_and_normalisation(tmp_path):
    d, src = _save_tiny(tmp_path, ff=T.GATED)
    W = T.dense_weight(192, 128)           # P > H
    ids = torch.tensor([[2, 5, 6, 9, 7, 3, 0, 0], [2, 5, 6, 7, 8, 9, 10, 3]]); mask = (ids != 0).long()
    with torch.no_grad():
        ref = src.eval()(input_ids=ids, attention_mask=mask).last_hidden_state
    for with_head in (False, True):
        if with_head:
            T.write_st_dense(d, W)
        for cls, pool in ((ENC.T5E5Encoder, 0), (ENC.T5BGEEncoder, 1)):
            e = cls.from_pretrained(d).train()
            with torch.no_grad():
                out = e(ids, mask)
            exp = T.pool_np(ref.numpy(), mask.numpy(), pool, W if with_head else None)
            assert out.shape == exp.shape == (2, 192 if with_head else 128)
            assert np.abs(out.numpy() - exp).max() <= 1e-5
            with pytest.raises(RuntimeError, match="HIP path only"):
                e.eval()(ids, mask)
    # the head takes part in training
    e = ENC.T5E5Encoder.from_pretrained(d).train()
    e(ids, mask).sum().backward()
    assert e.dense.weight.grad is not None and float(e.dense.weight.grad.abs().max()) > 0


def test_the_c_abi_keeps_its_functions_and_documents_the_new_names():
    text = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert re.search(r"#define\s+KR_ABI_VERSION\s+9\b", text)
    for name in ("config.t5_feed_forward", "dense.weight", "shared.weight", "encoder.embed_tokens.weight", "encoder.final_layer_norm.weight",
                 "SelfAttention.relative_attention_bias.weight", "DenseReluDense", "wi_0", "gelu_new"):
        assert name in text, name
    # the new names reach the library through kr_encoder_load_weight: no new entry point
    assert "kr_encoder_load_dense" not in text and "kr_encoder_set_" not in text
    src = open(os.path.join(REPO, "kirag_amd", "csrc", "encoder.hip")).read()
    assert '"config.t5_feed_forward"' in src and '"dense.weight"' in src
