"""Host-side tests of the RoBERTa-family support (multilingual-e5, bge-m3's dense head): the dispatch under the two registry names, the train-mode
forward of the XLM-R twins against XLMRobertaModel computed by hand, fairseq's position rule, the pad id of the feed's padded fallback, and the fences
the C ABI keeps (same functions, ABI 9, the reserved ``config.`` name documented)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xlmr_util as X  # noqa: E402

from kirag_amd import _lib, feed  # noqa: E402
from kirag_amd.collators import COLLATOR_MAP, E5Collator  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever.retrievers import RETRIEVER_MAP, load_retriever  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the layouts the rule treats differently from `column + P + 1`: P inside an attended sequence, a masked column holding a non-P id, an attended tail of P
ODD_IDS = np.array([[0, 5, 6, 1, 7, 2, 1, 1],
                    [1, 1, 0, 5, 6, 7, 8, 2],
                    [1, 9, 0, 5, 6, 7, 8, 2],
                    [0, 5, 6, 2, 1, 1, 1, 1]])
ODD_MASK = np.array([[1, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 1],
                     [0, 0, 1, 1, 1, 1, 1, 1],
                     [1, 1, 1, 1, 1, 1, 1, 0]])


def _save_tiny(tmp_path, kind, name):
    from transformers import BertConfig, BertModel, RobertaConfig, RobertaModel, XLMRobertaConfig, XLMRobertaModel, XLMRobertaXLConfig, XLMRobertaXLModel
    kw = dict(vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128)
    torch.manual_seed(11)
    if kind == "bert":
        m = BertModel(BertConfig(max_position_embeddings=64, **kw), add_pooling_layer=False)
    elif kind == "xlm-roberta":
        m = XLMRobertaModel(XLMRobertaConfig(max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, **kw), add_pooling_layer=False)
    elif kind == "roberta":
        m = RobertaModel(RobertaConfig(max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, **kw), add_pooling_layer=False)
    else:
        m = XLMRobertaXLModel(XLMRobertaXLConfig(max_position_embeddings=66, type_vocab_size=1, pad_token_id=1, **kw), add_pooling_layer=False)
    d = str(tmp_path / name)
    m.save_pretrained(d)
    return d, m


def test_registries_keep_their_two_names():
    assert set(RETRIEVER_MAP) == set(COLLATOR_MAP) == {"E5Retriever", "BGERetriever"}
    assert RETRIEVER_MAP["E5Retriever"] is ENC.E5Encoder and RETRIEVER_MAP["BGERetriever"] is ENC.BGEEncoder


def test_dispatch_by_the_checkpoints_model_type(tmp_path):
    from transformers import BertModel, XLMRobertaModel
    d_bert, _ = _save_tiny(tmp_path, "bert", "bert")
    d_xlmr, _ = _save_tiny(tmp_path, "xlm-roberta", "xlmr")
    d_rob, _ = _save_tiny(tmp_path, "roberta", "roberta")
    d_xl, _ = _save_tiny(tmp_path, "xlm-roberta-xl", "xl")
    e = load_retriever("E5Retriever", d_bert)
    assert type(e) is ENC.E5Encoder and isinstance(e, BertModel) and e._pool == ENC.POOL_MEAN
    b = load_retriever("BGERetriever", d_bert)
    assert type(b) is ENC.BGEEncoder and b._pool == ENC.POOL_CLS
    for d in (d_xlmr, d_rob):
        e = load_retriever("E5Retriever", d)
        assert type(e) is ENC.XLMRobertaE5Encoder and isinstance(e, XLMRobertaModel) and not isinstance(e, BertModel) and e._pool == ENC.POOL_MEAN
        b = ENC.BGEEncoder.from_pretrained(d)
        assert type(b) is ENC.XLMRobertaBGEEncoder and b._pool == ENC.POOL_CLS
        assert e.config.pad_token_id == 1 and not e.training
    # pre-LN XLM-R-XL is another architecture: not dispatched
    assert type(ENC.E5Encoder.from_pretrained(d_xl)) is ENC.E5Encoder
    # the twins share the machinery of the BERT classes: one mixin, no copy
    for name in ("_hip_forward", "forward_packed", "invalidate_hip_weights", "train", "load_state_dict", "_apply", "forward", "hip_last_hidden_state"):
        assert getattr(ENC.XLMRobertaE5Encoder, name) is getattr(ENC.E5Encoder, name), name
    # a twin loads its own checkpoints directly as well, and saves what it loaded
    t = ENC.XLMRobertaE5Encoder.from_pretrained(d_xlmr)
    t.save_pretrained(str(tmp_path / "again"))
    assert type(load_retriever("E5Retriever", str(tmp_path / "again"))) is ENC.XLMRobertaE5Encoder


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_train_mode_forward_is_xlm_roberta_with_the_encoders_pooling(tmp_path, name, pool):
    """train() mode on the CPU: the inherited autograd forward of XLMRobertaModel + pooling + normalise.  (The BertModel classes filled with these weights
    compute with BERT's position ids: the encoder this test loads differed from the hand computation before the dispatch existed.)"""
    d, m = _save_tiny(tmp_path, "xlm-roberta", "xlmr")
    ids, mask = torch.from_numpy(ODD_IDS), torch.from_numpy(ODD_MASK)
    assert all(X.differs_from_simple_rules(ODD_IDS[r], ODD_MASK[r]) for r in (0, 2, 3))            # row 1 is plain left padding
    assert ((X.fairseq_positions(ODD_IDS) != np.arange(8)[None, :] + 2) & (ODD_MASK != 0)).any(axis=1).all()
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
    assert e.embeddings.position_embeddings.weight.grad is not None
    with pytest.raises(RuntimeError, match="HIP path only"):
        e.eval()(ids, mask)                                     # a CPU model in eval mode: no fallback, as for BERT


def test_position_rule_restated_in_numpy_equals_hf():
    from transformers.models.xlm_roberta.modeling_xlm_roberta import XLMRobertaEmbeddings
    hf = XLMRobertaEmbeddings.create_position_ids_from_input_ids
    assert X.fairseq_positions(np.array([[0, 5, 6, 1, 7, 2, 1, 1]])).tolist() == [[2, 3, 4, 1, 5, 6, 1, 1]]
    assert X.fairseq_positions(np.array([[1, 1, 0, 5, 6, 7, 8, 2]])).tolist() == [[1, 1, 2, 3, 4, 5, 6, 7]]
    assert np.array_equal(X.fairseq_positions(ODD_IDS), hf(torch.from_numpy(ODD_IDS), 1).numpy())
    rng = np.random.default_rng(0)
    for P in (0, 1, 3):
        ids = rng.integers(0, 6, (50, 70))
        assert np.array_equal(X.fairseq_positions(ids, P), hf(torch.from_numpy(ids), P).numpy())
        assert X.fairseq_positions(ids, P).max() <= P + 70


def test_padded_fallback_of_the_feed_fills_the_tokenizers_pad_id():
    """Under fairseq's rule a masked column that does not hold the pad id counts: the padded form of a ragged frame must carry the tokenizer's pad id (1), and
    a left-padding tokenizer's batch travels as it is."""
    words = X.toy_words()
    texts = [" ".join(words[i:i + 3 + i % 5]) for i in range(6)]
    col = E5Collator(tokenizer=X.toy_tokenizer(), query_maxlength=16, doc_maxlength=16)
    enc = col.encode_doc(texts)
    ids, mask = enc["input_ids"].numpy(), enc["attention_mask"].numpy()
    assert (ids[mask == 0] == 1).all() and (mask == 0).any() and (ids[:, 0] == 0).all()
    t = feed.tokenize_batch(col, texts)
    assert t.kind == feed.KIND_RAGGED
    back = feed.repad(t.ids, t.lens, t.S, col.tokenizer.pad_token_id)
    assert torch.equal(back["input_ids"], enc["input_ids"]) and torch.equal(back["attention_mask"], enc["attention_mask"])
    assert np.array_equal(X.fairseq_positions(ids)[mask != 0], (np.arange(ids.shape[1])[None, :] + 2).repeat(len(ids), 0)[mask != 0])
    left = E5Collator(tokenizer=X.toy_tokenizer(padding_side="left"), query_maxlength=16, doc_maxlength=16)
    tl = feed.tokenize_batch(left, texts)
    assert tl.kind == feed.KIND_PADDED
    lids = tl.ids.reshape(tl.n, tl.S); lmask = tl.mask.reshape(tl.n, tl.S)
    assert (lids[lmask == 0] == 1).all() and (lmask[:, -1] == 1).all()
    # the positions of the real tokens do not depend on the padding side: 2, 3, ... from <s>
    for r in range(tl.n):
        assert X.fairseq_positions(lids)[r][lmask[r] != 0].tolist() == list(range(2, 2 + int(lmask[r].sum())))


def test_tools_know_the_roberta_family():
    import importlib.util
    import subprocess
    from transformers import XLMRobertaConfig, XLMRobertaModel
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(REPO, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    m = XLMRobertaModel(XLMRobertaConfig(vocab_size=300, hidden_size=128, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256, max_position_embeddings=66,
                                         type_vocab_size=1, pad_token_id=1), add_pooling_layer=False)
    # the torch emulation of the rounding points implements BERT's position rule only: an XLM-R model is refused there, never computed wrongly
    with pytest.raises(SystemExit, match="fairseq"):
        cc.check_model(m, cc.parse(["(xlm-r)", "--n", "4", "--max-length", "16", "--random-tokens", "--emulate"]))
    ids, mask = cc.load_inputs(cc.parse(["x", "--n", "4", "--max-length", "16", "--random-tokens"]), "(none)", 300, pad_id=1)[1]
    assert (ids[mask == 0] == 1).all() and (ids[:, 0] == 0).all() and (ids[mask != 0] != 1).all()
    src = open(os.path.join(REPO, "tools", "enc_bench.py")).read()
    for shape in ("xlmr-base", "xlmr-large", "bge-m3"):
        assert '"%s"' % shape in src
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "enc_bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "bge-m3" in r.stdout


def test_c_abi_is_unchanged_and_the_reserved_name_is_documented():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50
    assert _lib.ABI_VERSION == 9
    assert "config.position_padding_idx" in hdr
    fields = re.search(r"typedef struct\s*\{([^}]*)\}\s*kr_bert_cfg;", hdr).group(1)
    assert re.findall(r"\b(?:int|float)\s+(\w+)\s*;", fields) == ["hidden", "layers", "heads", "intermediate", "vocab", "max_pos", "type_vocab", "ln_eps"]
