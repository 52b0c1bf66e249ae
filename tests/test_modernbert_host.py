"""Host-side tests of the ModernBERT support: the dispatch under the two registry names, the settings the Python layer derives from an HF config, the
intermediate-size padding (exact, against a numpy restatement of the MLP), the refusals that happen before a handle exists, and the fences the C ABI keeps
(same functions, the settings documented in the header)."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modernbert_util as M  # noqa: E402

from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever.retrievers import RETRIEVER_MAP, load_retriever  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save_tiny(tmp_path, name="modern"):
    from transformers import ModernBertModel
    torch.manual_seed(11)
    m = ModernBertModel(M.hf_config(M.cfg(64, 4, 2, 96, 120, 64, local_attention=8)))
    d = str(tmp_path / name)
    m.save_pretrained(d)
    return d, m


def test_dispatch_by_the_checkpoints_model_type(tmp_path):
    from transformers import BertModel, ModernBertModel
    assert set(RETRIEVER_MAP) == {"E5Retriever", "BGERetriever"}
    d, src = _save_tiny(tmp_path)
    for name, twin, pool in (("E5Retriever", ENC.ModernBertE5Encoder, ENC.POOL_MEAN), ("BGERetriever", ENC.ModernBertBGEEncoder, ENC.POOL_CLS)):
        e = load_retriever(name, d)
        assert type(e) is twin and isinstance(e, ModernBertModel) and not isinstance(e, BertModel) and e._pool == pool and not e.training
        sd, ref = e.state_dict(), src.state_dict()
        assert set(sd) == set(ref)
        for k, v in ref.items():
            assert torch.equal(sd[k], v), k
        assert "layers.0.attn.Wqkv.weight" in sd and "layers.1.attn_norm.weight" in sd and "layers.0.attn_norm.weight" not in sd and "final_norm.weight" in sd
    _, info = ENC.E5Encoder.from_pretrained(d, output_loading_info=True)
    assert not info["missing_keys"], info["missing_keys"]
    # one mixin, no copy
    for name in ("_hip_forward", "forward_packed", "invalidate_hip_weights", "train", "load_state_dict", "_apply", "forward", "hip_last_hidden_state"):
        assert getattr(ENC.ModernBertE5Encoder, name) is getattr(ENC.E5Encoder, name), name
        assert getattr(ENC.ModernBertBGEEncoder, name) is getattr(ENC.E5Encoder, name), name
    # a twin loads its own checkpoints directly as well, and saves what it loaded
    t = ENC.ModernBertBGEEncoder.from_pretrained(d)
    t.save_pretrained(str(tmp_path / "again"))
    assert type(load_retriever("BGERetriever", str(tmp_path / "again"))) is ENC.ModernBertBGEEncoder


def test_train_mode_forward_is_hfs_with_the_encoders_pooling(tmp_path):
    d, src = _save_tiny(tmp_path)
    ids = torch.tensor([[2, 5, 6, 9, 7, 3, 0, 0], [2, 5, 6, 7, 8, 9, 10, 3]]); mask = (ids != 0).long()
    with torch.no_grad():
        ref = src.eval()(input_ids=ids, attention_mask=mask).last_hidden_state
    for cls, pool in ((ENC.ModernBertE5Encoder, 0), (ENC.ModernBertBGEEncoder, 1)):
        e = cls.from_pretrained(d).train()
        with torch.no_grad():
            out = e(ids, mask)
        exp = M.pool_np(ref.numpy(), mask.numpy(), pool)
        assert np.abs(out.numpy() - exp).max() <= 1e-5
        with pytest.raises(RuntimeError, match="HIP path only"):
            e.eval()(ids, mask)


def test_settings_come_from_the_hf_config():
    c = M.hf_config(M.cfg(768, 22, 12, 1152, 50368))
    s = ENC.HipBertForward._modern_settings(c)
    assert list(s) == ["config.rotary_inv_freq", *ENC.MODERN_SETTINGS]
    assert np.array_equal(s["config.rotary_inv_freq"].numpy(), M.inv_freq(64, 160000.0))
    assert np.array_equal(s[M.LOCAL_FREQ_NAME].numpy(), M.inv_freq(64, 10000.0))
    assert s[M.HALF_WINDOW_NAME].tolist() == [64.0]
    assert s[M.LAYER_FLAGS_NAME].tolist() == [0.0 if i % 3 == 0 else 1.0 for i in range(22)] and c.layer_types == M.layer_types(22)
    # every layer global: no local settings at all; every layer local: the local frequencies serve both names.  (transformers' own ModernBertConfig cannot
    # hold a single layer type; the settings do not depend on that)
    g = ENC.HipBertForward._modern_settings(M.cfg(128, 2, 4, 256, 100, types=[M.FULL, M.FULL]))
    assert list(g) == ["config.rotary_inv_freq", M.LAYER_FLAGS_NAME] and g[M.LAYER_FLAGS_NAME].tolist() == [0.0, 0.0]
    a = ENC.HipBertForward._modern_settings(M.cfg(128, 2, 4, 256, 100, types=[M.SLIDING, M.SLIDING], local_attention=10))
    assert np.array_equal(a["config.rotary_inv_freq"].numpy(), M.inv_freq(32, 10000.0)) and a[M.HALF_WINDOW_NAME].tolist() == [5.0]
    # the SimpleNamespace configs of the tests give the same
    s2 = ENC.HipBertForward._modern_settings(M.cfg(768, 22, 12, 1152, 50368))
    assert all(torch.equal(s[k], s2[k]) for k in s)


@pytest.mark.parametrize("ff", [2624, 200, 129])
def test_ff_padding_is_exact(ff):
    """pad_modernbert_ff against a numpy restatement of ModernBertMLP: the padded tensors give the unpadded result bit for bit in float64 (the padded
    intermediate features are gelu(0) * 0 = 0 and meet zero columns), with and without the bias; other tensors and multiples of 128 pass through."""
    H = 64
    ff_pad = -(-ff // 128) * 128
    rng = np.random.default_rng(ff)
    wi, wo, bi = rng.standard_normal((2 * ff, H)).astype(np.float32), rng.standard_normal((H, ff)).astype(np.float32), rng.standard_normal(2 * ff).astype(np.float32)
    x = rng.standard_normal((7, H))
    pwi, pwo, pbi = (ENC.pad_modernbert_ff(n, t, ff, ff_pad) for n, t in (("layers.3.mlp.Wi.weight", wi), ("layers.3.mlp.Wo.weight", wo), ("layers.3.mlp.Wi.bias", bi)))
    assert pwi.shape == (2 * ff_pad, H) and pwo.shape == (H, ff_pad) and pbi.shape == (2 * ff_pad,) and isinstance(pwi, np.ndarray)
    assert np.array_equal(pwi[:ff], wi[:ff]) and np.array_equal(pwi[ff_pad:ff_pad + ff], wi[ff:]) and not pwi[ff:ff_pad].any() and not pwi[ff_pad + ff:].any()
    assert not pwo[:, ff:].any() and not pbi[ff:ff_pad].any() and not pbi[ff_pad + ff:].any()
    assert np.array_equal(M.mlp_np(x, pwi, pwo), M.mlp_np(x, wi, wo))
    assert np.array_equal(M.mlp_np(x, pwi, pwo, pbi), M.mlp_np(x, wi, wo, bi))
    # torch tensors stay torch tensors; what is not an MLP tensor, and an intermediate size that needs no padding, come back as they are
    t = ENC.pad_modernbert_ff("layers.0.mlp.Wo.weight", torch.from_numpy(wo), ff, ff_pad)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), pwo)
    for name in ("layers.0.attn.Wo.weight", "layers.0.mlp_norm.weight", "final_norm.weight", "layers.0.mlp.Wo.bias"):
        assert ENC.pad_modernbert_ff(name, wo, ff, ff_pad) is wo
    assert ENC.pad_modernbert_ff("layers.0.mlp.Wi.weight", wi, 256, 256) is wi


def test_refusals_name_the_field_before_a_handle_exists(monkeypatch):
    from kirag_amd import _lib
    class NoHandle:      # stands in for the loaded library: any call into it (kr_encoder_create_ex first of all) fails the test
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached before the refusal")
    monkeypatch.setattr(_lib, "load", lambda: NoHandle())
    base = dict(H=128, L=3, heads=4, FF=256, vocab=100)
    def cfg(**kw):
        return M.cfg(base["H"], base["L"], base["heads"], base["FF"], base["vocab"], **kw)
    for kw, field in ((dict(hidden_activation="silu"), "hidden_activation"), (dict(head_dim=48), "head_dim"),
                      (dict(types=[M.FULL, "chunked_attention", M.SLIDING]), "layer_types"), (dict(types=[M.FULL, M.SLIDING]), "layer_types")):
        with pytest.raises((NotImplementedError, AssertionError)) as ei:
            ENC.HipBertForward(cfg(**kw), 0)
        assert isinstance(ei.value, NotImplementedError) and field in str(ei.value), (field, ei.value)
    # a rope variant with an attention factor (yarn): refused by attention_scaling
    c = M.hf_config(cfg())
    c.rope_parameters = {M.FULL: {"rope_type": "yarn", "rope_theta": 160000.0, "factor": 4.0, "original_max_position_embeddings": 2048},
                         M.SLIDING: {"rope_type": "default", "rope_theta": 10000.0}}
    with pytest.raises((NotImplementedError, AssertionError)) as ei:
        ENC.HipBertForward(c, 0)
    assert isinstance(ei.value, NotImplementedError) and "attention_scaling" in str(ei.value), ei.value


def test_header_documents_the_settings_and_the_abi_stays():
    from kirag_amd import _lib
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    for name in ("config.rotary_inv_freq", *ENC.MODERN_SETTINGS):
        assert name in hdr, name
    m = re.search(r"#define\s+KR_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 9
