"""Host-side tests of the MPNet support (all-mpnet-base-v2, multi-qa-mpnet-*): the dispatch under the two registry names, the train-mode forward of the MPNet
twins against MPNetModel computed by hand, the integer bucket rule and the per-head table by column difference that the GPU tests rest on, and the fences
the C ABI keeps (same functions, ABI 9, the bias tensor's name documented in the header)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpnet_util as M  # noqa: E402

from kirag_amd import _lib  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever.retrievers import RETRIEVER_MAP, load_retriever  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save_tiny(tmp_path, kind, name):
    from transformers import BertConfig, BertModel, MPNetConfig, MPNetModel, XLMRobertaConfig, XLMRobertaModel, XLMRobertaXLConfig, XLMRobertaXLModel
    kw = dict(vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128)
    torch.manual_seed(11)
    if kind == "bert":
        m = BertModel(BertConfig(max_position_embeddings=64, **kw), add_pooling_layer=False)
    elif kind == "mpnet":
        m = MPNetModel(MPNetConfig(max_position_embeddings=66, layer_norm_eps=1e-5, **kw), add_pooling_layer=False)
        with torch.no_grad():
            m.encoder.relative_attention_bias.weight.normal_(0.0, 2.0)       # HF's init is N(0, 0.02): too small for the bias to show
    elif kind == "xlm-roberta":
        m = XLMRobertaModel(XLMRobertaConfig(max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, **kw), add_pooling_layer=False)
    else:
        m = XLMRobertaXLModel(XLMRobertaXLConfig(max_position_embeddings=66, type_vocab_size=1, pad_token_id=1, **kw), add_pooling_layer=False)
    d = str(tmp_path / name)
    m.save_pretrained(d)
    return d, m


def test_dispatch_by_the_checkpoints_model_type(tmp_path, caplog):
    from transformers import BertModel, MPNetModel, XLMRobertaModel
    assert set(RETRIEVER_MAP) == {"E5Retriever", "BGERetriever"}
    d_mp, src = _save_tiny(tmp_path, "mpnet", "mpnet")
    for name, twin, pool in (("E5Retriever", ENC.MPNetE5Encoder, ENC.POOL_MEAN), ("BGERetriever", ENC.MPNetBGEEncoder, ENC.POOL_CLS)):
        e = load_retriever(name, d_mp)
        assert type(e) is twin and isinstance(e, MPNetModel) and not isinstance(e, BertModel) and e._pool == pool and not e.training
        # no missing keys: every parameter the checkpoint holds arrived (a BertModel filled from it keeps its random layers)
        sd, ref = e.state_dict(), src.state_dict()
        for k, v in ref.items():
            assert torch.equal(sd[k], v), k
        assert "encoder.relative_attention_bias.weight" in sd and "encoder.layer.0.attention.attn.q.weight" in sd
    _, info = ENC.E5Encoder.from_pretrained(d_mp, output_loading_info=True)
    assert not [k for k in info["missing_keys"] if not k.startswith("pooler.")], info["missing_keys"]
    # the other families dispatch as before
    d_bert, _ = _save_tiny(tmp_path, "bert", "bert")
    d_xlmr, _ = _save_tiny(tmp_path, "xlm-roberta", "xlmr")
    d_xl, _ = _save_tiny(tmp_path, "xlm-roberta-xl", "xl")
    assert type(load_retriever("E5Retriever", d_bert)) is ENC.E5Encoder and type(load_retriever("BGERetriever", d_bert)) is ENC.BGEEncoder
    x = load_retriever("E5Retriever", d_xlmr)
    assert type(x) is ENC.XLMRobertaE5Encoder and isinstance(x, XLMRobertaModel)
    assert type(ENC.BGEEncoder.from_pretrained(d_xlmr)) is ENC.XLMRobertaBGEEncoder
    assert type(ENC.E5Encoder.from_pretrained(d_xl)) is ENC.E5Encoder
    # one mixin, no copy
    for name in ("_hip_forward", "forward_packed", "invalidate_hip_weights", "train", "load_state_dict", "_apply", "forward", "hip_last_hidden_state"):
        assert getattr(ENC.MPNetE5Encoder, name) is getattr(ENC.E5Encoder, name), name
        assert getattr(ENC.MPNetBGEEncoder, name) is getattr(ENC.E5Encoder, name), name
    # a twin loads its own checkpoints directly as well, and saves what it loaded
    t = ENC.MPNetE5Encoder.from_pretrained(d_mp)
    t.save_pretrained(str(tmp_path / "again"))
    assert type(load_retriever("E5Retriever", str(tmp_path / "again"))) is ENC.MPNetE5Encoder


IDS = np.array([[0, 5, 6, 9, 7, 2, 1, 1],
                [1, 1, 0, 5, 6, 7, 8, 2],
                [0, 5, 6, 7, 8, 9, 10, 2],
                [1, 0, 5, 2, 1, 1, 1, 1]])
MASK = np.array([[1, 1, 1, 1, 1, 1, 0, 0],
                 [0, 0, 1, 1, 1, 1, 1, 1],
                 [1, 1, 1, 1, 1, 1, 1, 1],
                 [0, 1, 1, 1, 0, 0, 0, 0]])


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_train_mode_forward_is_mpnet_with_the_encoders_pooling(tmp_path, name, pool):
    """train() mode on the CPU: the inherited autograd forward of MPNetModel + pooling + normalise, within the bar the XLM-R host test uses (1e-6)."""
    d, m = _save_tiny(tmp_path, "mpnet", "mpnet")
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
    g = e.encoder.relative_attention_bias.weight.grad
    assert g is not None and float(g.abs().max()) > 0
    # token_type_ids (what a BERT-style collator may pass) are accepted and ignored, as MPNetModel does
    assert torch.equal(e(ids, mask, token_type_ids=torch.zeros_like(ids)).detach(), out.detach())
    with pytest.raises(RuntimeError, match="HIP path only"):
        e.eval()(ids, mask)                                     # a CPU model in eval mode: no fallback, as for BERT


def test_integer_bucket_rule_and_delta_table_equal_hf():
    from transformers import MPNetConfig
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    d = np.arange(-8200, 8201)
    hf = MPNetEncoder.relative_position_bucket(torch.from_numpy(d)).numpy()
    assert np.array_equal(M.bucket(d), hf)
    first = [int(np.abs(d[(M.bucket(d) == b)]).min()) for b in range(8, 16)]
    assert tuple(first) == M.BOUNDARIES
    assert set(M.bucket(d)) == set(range(32)) - {16}
    assert (M.bucket(d[d <= -91]) == 15).all() and (M.bucket(d[d >= 91]) == 31).all()
    torch.manual_seed(5)
    enc = MPNetEncoder(MPNetConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128, vocab_size=50)).eval()
    with torch.no_grad():
        enc.relative_attention_bias.weight.normal_(0.0, 4.0)
    W = enc.relative_attention_bias.weight.detach().numpy()
    for S in (64, 300):
        with torch.no_grad():
            ref = enc.compute_position_bias(torch.zeros(1, S, 64))[0].numpy()
        got = M.bias_from_table(M.delta_table(W, S), S)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), S
    # the mirrored table is what bucket(-d) reads
    Wm = M.mirrored(W)
    dd = np.arange(-300, 301)
    assert np.array_equal(Wm[M.bucket(dd)], W[M.bucket(-dd)])
    bt = M.boundary_table(4)
    assert all(bt[b, 0] != bt[b + 1, 0] for b in range(15)) and all(bt[b, 0] != bt[b + 16, 0] for b in range(1, 16))


def test_c_abi_is_unchanged_and_the_bias_tensor_is_documented():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50
    assert _lib.ABI_VERSION == 9
    assert "encoder.relative_attention_bias.weight" in hdr and "attention.attn." in hdr
    fields = re.search(r"typedef struct\s*\{([^}]*)\}\s*kr_bert_cfg;", hdr).group(1)
    assert re.findall(r"\b(?:int|float)\s+(\w+)\s*;", fields) == ["hidden", "layers", "heads", "intermediate", "vocab", "max_pos", "type_vocab", "ln_eps"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "enc_bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "mpnet-base" in r.stdout


def test_python_side_refuses_another_bucket_count():
    """relative_attention_num_buckets != 32 is refused before a handle exists (HF's MPNetEncoder computes with 32 whatever the config says)"""
    with pytest.raises(ValueError, match="32"):
        ENC.HipBertForward(M.cfg(128, 1, 4, 512, 100, buckets=64), 0)
