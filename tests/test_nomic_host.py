"""Host-side tests of the NomicBert support (nomic-embed-text-v1 / -v1.5): the dispatch under the two registry names, the train-mode forward of the twins,
the refusals that happen before a handle exists, the rotary table rule and the packed row orders that the GPU tests rest on, and the fences the C ABI keeps
(same functions, ABI 9, the setting and the names documented in the header)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nomic_util as N  # noqa: E402

from kirag_amd import _lib  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever.retrievers import RETRIEVER_MAP, load_retriever  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save_tiny(tmp_path, name="nomic"):
    from transformers import NomicBertConfig, NomicBertModel
    torch.manual_seed(11)
    m = NomicBertModel(NomicBertConfig(vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, max_position_embeddings=64),
                       add_pooling_layer=False)
    d = str(tmp_path / name)
    m.save_pretrained(d)
    return d, m


def test_dispatch_by_the_checkpoints_model_type(tmp_path):
    from transformers import BertModel, NomicBertModel
    assert set(RETRIEVER_MAP) == {"E5Retriever", "BGERetriever"}
    d, src = _save_tiny(tmp_path)
    for name, twin, pool in (("E5Retriever", ENC.NomicBertE5Encoder, ENC.POOL_MEAN), ("BGERetriever", ENC.NomicBertBGEEncoder, ENC.POOL_CLS)):
        e = load_retriever(name, d)
        assert type(e) is twin and isinstance(e, NomicBertModel) and not isinstance(e, BertModel) and e._pool == pool and not e.training
        sd, ref = e.state_dict(), src.state_dict()
        for k, v in ref.items():
            assert torch.equal(sd[k], v), k
        assert "layers.0.self_attn.q_proj.weight" in sd and "layers.1.mlp.up_proj.weight" in sd and not any("position_embeddings" in k for k in sd)
    _, info = ENC.E5Encoder.from_pretrained(d, output_loading_info=True)
    assert not [k for k in info["missing_keys"] if not k.startswith("pooler.")], info["missing_keys"]
    # one mixin, no copy
    for name in ("_hip_forward", "forward_packed", "invalidate_hip_weights", "train", "load_state_dict", "_apply", "forward", "hip_last_hidden_state"):
        assert getattr(ENC.NomicBertE5Encoder, name) is getattr(ENC.E5Encoder, name), name
        assert getattr(ENC.NomicBertBGEEncoder, name) is getattr(ENC.E5Encoder, name), name
    # a twin loads its own checkpoints directly as well, and saves what it loaded
    t = ENC.NomicBertBGEEncoder.from_pretrained(d)
    t.save_pretrained(str(tmp_path / "again"))
    assert type(load_retriever("BGERetriever", str(tmp_path / "again"))) is ENC.NomicBertBGEEncoder


IDS = np.array([[2, 5, 6, 9, 7, 3, 0, 0],
                [0, 0, 2, 5, 6, 7, 8, 3],
                [2, 5, 6, 7, 8, 9, 10, 3],
                [0, 2, 5, 3, 0, 0, 0, 0]])
MASK = np.array([[1, 1, 1, 1, 1, 1, 0, 0],
                 [0, 0, 1, 1, 1, 1, 1, 1],
                 [1, 1, 1, 1, 1, 1, 1, 1],
                 [0, 1, 1, 1, 0, 0, 0, 0]])


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_train_mode_forward_is_nomic_bert_with_the_encoders_pooling(tmp_path, name, pool):
    """train() mode on the CPU: the inherited autograd forward of NomicBertModel + pooling + normalise, within the bar the XLM-R host test uses (1e-6)."""
    d, m = _save_tiny(tmp_path)
    ids, mask = torch.from_numpy(IDS), torch.from_numpy(MASK)
    m.eval()
    with torch.no_grad():
        lh = m(input_ids=ids, attention_mask=mask).last_hidden_state
    v = (lh * mask[..., None]).sum(1) / mask.sum(1)[..., None] if pool == 0 else lh[:, 0]
    ref = torch.nn.functional.normalize(v, dim=-1)
    e = load_retriever(name, d)
    e.train()
    for mod in e.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    out = e(ids, mask)
    assert out.requires_grad and out.shape == ref.shape
    assert float((out.detach() - ref).abs().max()) <= 1e-6
    out.sum().backward()
    g = e.layers[0].mlp.up_proj.weight.grad
    assert g is not None and float(g.abs().max()) > 0
    with pytest.raises(RuntimeError, match="HIP path only"):
        e.eval()(ids, mask)                                     # a CPU model in eval mode: no fallback, as for BERT


def test_refusals_name_the_field_and_come_before_any_handle(monkeypatch):
    """an unsupported activation, attention_scaling != 1 and a head_dim other than hidden / heads raise NotImplementedError naming the field; no handle is made"""
    def no_handle(*a, **k):
        raise AssertionError("a handle was created")
    lib = _lib.load()
    monkeypatch.setattr(lib, "kr_encoder_create_ex", no_handle)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        ENC.HipBertForward(N.cfg(128, 1, 4, 512, 100, hidden_act="gelu"), 0)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        ENC.HipBertForward(N.cfg(128, 1, 4, 512, 100, hidden_act="relu"), 0)
    with pytest.raises(NotImplementedError, match="head_dim"):
        ENC.HipBertForward(N.cfg(128, 1, 4, 512, 100, head_dim=64), 0)
    yarn = {"rope_theta": 1000.0, "rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 2048}
    with pytest.raises(NotImplementedError, match="attention_scaling"):
        ENC.HipBertForward(N.hf_config(N.cfg(128, 1, 4, 512, 100, rope_parameters=yarn)), 0)     # HF's yarn initialiser wants its own config class
    # a BERT config with silu is still refused (silu belongs to the gated MLP of nomic_bert)
    from types import SimpleNamespace
    with pytest.raises(NotImplementedError, match="hidden_act"):
        ENC.HipBertForward(SimpleNamespace(hidden_act="silu", model_type="bert"), 0)
    # what is accepted: the frequencies HF computes, d_h / 2 of them
    for H, heads in ((768, 12), (384, 12)):
        f = ENC.HipBertForward._nomic_inv_freq(N.cfg(H, 1, heads, 512, 100))
        assert f.dtype == torch.float32 and np.array_equal(f.numpy(), N.inv_freq(H // heads))


@pytest.mark.parametrize("d_h", [32, 64])
def test_table_rule_equals_hf_rotary_emb(d_h):
    """angle[pos, j] = the fp32 product float(pos) * inv_freq[j]: with the angles restated in numpy, HF's cos / sin come out bit for bit at positions 0 .. 8191
    (through the same elementary functions: torch's fp32 cos / sin are not correctly rounded, numpy's differ from them in ~5 % of the entries by one ulp).
    The library's entries, the correctly rounded cosine / sine of the same fp32 angle, are within one ulp of HF's."""
    from transformers.models.nomic_bert.modeling_nomic_bert import NomicBertRotaryEmbedding
    c = N.cfg(d_h * 12, 1, 12, 512, 100, max_pos=8192)
    rope = NomicBertRotaryEmbedding(N.hf_config(c))
    assert np.array_equal(rope.inv_freq.numpy(), N.inv_freq(d_h)) and float(rope.attention_scaling) == 1.0
    cos, sin = rope(torch.zeros(1, 1, 1), torch.arange(8192)[None])
    cos, sin = cos[0].numpy(), sin[0].numpy()
    assert cos.shape == (8192, d_h) and np.array_equal(cos[:, :d_h // 2], cos[:, d_h // 2:]) and np.array_equal(sin[:, :d_h // 2], sin[:, d_h // 2:])
    a = torch.from_numpy(N.angles(N.inv_freq(d_h), 8192))
    assert np.array_equal(a.cos().numpy().view(np.uint32), cos[:, :d_h // 2].view(np.uint32))
    assert np.array_equal(a.sin().numpy().view(np.uint32), sin[:, :d_h // 2].view(np.uint32))
    tc, ts = N.tables(N.inv_freq(d_h), 8192)
    ulp = np.spacing(np.float32(1.0))            # |cos|, |sin| <= 1
    assert float(np.abs(tc - cos[:, :d_h // 2]).max()) <= ulp and float(np.abs(ts - sin[:, :d_h // 2]).max()) <= ulp
    # the rotation written with the half tables is HF's apply_rotary_pos_emb
    from transformers.models.nomic_bert.modeling_nomic_bert import apply_rotary_pos_emb
    x = torch.randn(1, 2, 50, d_h, generator=torch.Generator().manual_seed(1))
    q, _ = apply_rotary_pos_emb(x, x, torch.from_numpy(cos[None, :50]), torch.from_numpy(sin[None, :50]))
    assert np.array_equal(N.rotate(x.numpy(), cos[:50, :d_h // 2], sin[:50, :d_h // 2]), q.numpy())


def test_packed_row_orders_round_trip():
    rng = np.random.default_rng(3)
    g, u = rng.standard_normal((256, 8)).astype(np.float32), rng.standard_normal((256, 8)).astype(np.float32)
    w = N.interleave_gate_up(g, u)
    assert w.shape == (512, 8) and np.array_equal(w[:16], g[:16]) and np.array_equal(w[16:32], u[:16]) and np.array_equal(w[32:48], g[16:32])
    g2, u2 = N.split_gate_up(w)
    assert np.array_equal(g2, g) and np.array_equal(u2, u)
    # 64-wide heads: a permutation inside every head that puts j and j + 32 into one 32-row tile, 16 rows apart
    r = np.arange(256)
    p = N.head64_row(r)
    assert sorted(p) == list(r) and (p // 64 == r // 64).all()
    j = r % 64
    first = j < 32
    assert (p[first] // 32 == N.head64_row(r[first] + 32) // 32).all() and (N.head64_row(r[first] + 32) - p[first] == 16).all()
    # permuting q and k of a head alike leaves every score alone
    q, k = rng.standard_normal((5, 64)), rng.standard_normal((7, 64))
    inv = np.argsort(N.head64_row(np.arange(64)))
    assert np.allclose(q @ k.T, q[:, inv] @ k[:, inv].T, rtol=0, atol=1e-12)


def test_c_abi_is_unchanged_and_the_setting_is_documented():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50
    assert _lib.ABI_VERSION == 9
    for word in ("config.rotary_inv_freq", "self_attn.", "mlp.gate_proj", "mlp.up_proj", "post_mlp_layernorm"):
        assert word in hdr, word
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "enc_bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "nomic-base" in r.stdout
