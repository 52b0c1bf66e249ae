"""Host-side tests of the SPLADE head (no GPU): the header's new pool value on an unchanged ABI, the parameter names that reach the library (the ``bert.``
prefix, HF's alias of the decoder bias, the tied decoder weight), refusals that name the field before a handle exists, the dict building and the scores on
hand-made vectors, the registry entry, and the preconditions the GPU tests' bar rests on (the ReLU cutting through the reference's own output, every mutant
of the head far outside the bar) checked on the CPU reference."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reranker_util as R  # noqa: E402
import splade_util as U  # noqa: E402

from kirag_amd import _lib  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever import rerankers as RR  # noqa: E402
from kirag_amd.retriever import splade as SP  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_gains_one_pool_value_and_no_function():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert re.search(r"^#define KR_POOL_SPLADE 4\b", hdr, re.M)
    assert re.search(r"^#define KR_POOL_WITH_SPARSE 0x10\b", hdr, re.M) and re.search(r"^#define KR_POOL_CLASSIFY 2\b", hdr, re.M)
    assert re.search(r"^#define KR_ABI_VERSION 9\b", hdr, re.M)
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50 and _lib.ABI_VERSION == 9
    for name in U.MLM:
        assert '"%s"' % name in hdr
    assert _lib.POOL_SPLADE == 4 and ENC.POOL_SPLADE == 4
    h = ENC.HipBertForward.__new__(ENC.HipBertForward)
    h.out_dim, h.num_labels, h.colbert_dim, h.vocab, h._h = 128, 3, 256, 1031, None
    assert h._out_shape(ENC.POOL_SPLADE, 5, 7) == (5, 1031) and h._out_shape(ENC.POOL_MEAN, 5, 7) == (5, 128)


def _tiny(tie=True, V=64):
    return U.hf_mlm("h64", V, U.tied_weights(V) if tie else {**U.backbone(V), **U.head(V)}, cls=SP.BertSpladeEncoder, tie=tie)


@pytest.mark.parametrize("tie", [True, False])
def test_the_names_that_reach_the_library(tie):
    """what HipBertForward.sync sends: the backbone without its prefix, all six head tensors once each, the decoder weight from the tied parameter"""
    m = _tiny(tie)
    names = [SP.splade_rename(n) for n, _ in m.named_parameters()]
    have = set(names)
    names += [n for n, _ in SP.splade_extra(m) if n not in have]
    assert set(U.MLM) <= set(names)
    if tie:
        assert len(names) == len(set(names))          # (untied, HF keeps cls.predictions.bias and the decoder's own bias apart: the later one, the decoder's, wins)
    assert not [n for n in names if n.startswith("bert.") or n == "cls.predictions.bias"]
    assert "embeddings.word_embeddings.weight" in names and "encoder.layer.1.output.LayerNorm.bias" in names
    sent = dict(SP.splade_extra(m))[SP.DECODER_WEIGHT]
    assert (sent is m.bert.embeddings.word_embeddings.weight) == tie and tuple(sent.shape) == (64, U.H)
    assert type(m)._hip_rename is SP.splade_rename and type(m)._hip_extra is SP.splade_extra and type(m)._pool == 4


def test_refusals_name_the_field(tmp_path):
    from transformers import BertConfig, DistilBertConfig, XLMRobertaConfig
    ok = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=64)
    cases = {"distil": (DistilBertConfig(dim=128, n_layers=1, n_heads=2, hidden_dim=256, vocab_size=64), NotImplementedError, "model_type='distilbert'"),
             "xlmr": (XLMRobertaConfig(**ok), NotImplementedError, "model_type='xlm-roberta'"),
             "act": (BertConfig(**{**ok, "hidden_act": "relu"}), NotImplementedError, "hidden_act='relu'"),
             "hidden": (BertConfig(**{**ok, "hidden_size": 96, "num_attention_heads": 3}), NotImplementedError, "hidden_size=96"),
             "heads": (BertConfig(**{**ok, "num_attention_heads": 8}), NotImplementedError, "num_attention_heads=8"),
             "ff": (BertConfig(**{**ok, "intermediate_size": 200}), NotImplementedError, "intermediate_size=200"),
             "pos": (BertConfig(**{**ok, "position_embedding_type": "relative_key"}), NotImplementedError, "position_embedding_type")}
    for what, (cfg, exc, pattern) in cases.items():
        d = str(tmp_path / what)
        cfg.save_pretrained(d)                      # config.json only: the refusal comes before any weight is read
        with pytest.raises(exc, match=pattern):
            SP.BertSpladeEncoder.from_pretrained(d)
        with pytest.raises(exc, match=pattern):
            RR.load_reranker("SPLADE", d, tokenizer=R.bert_pair_tokenizer(), device="cpu")
    with pytest.raises(KeyError, match="SPLADE"):
        RR.load_reranker("NoSuch", "x")
    # eval mode only, and no CPU fallback; train() mode is HF's own forward
    m = _tiny()
    ids = torch.tensor([[U.CLS, 10, 11, U.SEP]])
    with pytest.raises(RuntimeError, match="eval"):
        m.train().forward_splade(ids)
    with pytest.raises(RuntimeError, match="HIP path only"):
        m.eval().forward_splade(ids)
    assert tuple(m.train()(input_ids=ids).logits.shape) == (1, 4, 64)


def test_save_load_round_trip_and_the_registry(tmp_path):
    m = _tiny()
    d = str(tmp_path / "ckpt")
    m.save_pretrained(d)
    back = SP.BertSpladeEncoder.from_pretrained(d)
    assert not back.training and back.cls.predictions.decoder.weight is back.bert.embeddings.word_embeddings.weight
    for (n, a), (_, b) in zip(m.named_parameters(), back.named_parameters()):
        assert torch.equal(a, b), n
    model = RR.load_reranker("SPLADE", d, tokenizer=R.bert_pair_tokenizer(), device="cpu")
    assert isinstance(model, SP.SpladeModel) and type(model.model) is SP.BertSpladeEncoder
    assert RR.HYBRID_RERANKER_MAP["SPLADE"] is SP.SpladeModel and list(RR.RERANKER_MAP) == ["BGEReranker"]


def test_dict_building_on_hand_made_vectors():
    names = ["[PAD]", "a", "b", "c", "d", "e"]
    tok = names.__getitem__
    v = np.array([9.0, 0.5, 0.0, -1.0, 2.0, 0.5], np.float32)
    assert SP.build_token_weights(v, tok, skip_ids=(0,)) == {"a": 0.5, "d": 2.0, "e": 0.5}          # pad skipped, 0 and the negative dropped
    assert SP.build_token_weights(v, tok) == {"[PAD]": 9.0, "a": 0.5, "d": 2.0, "e": 0.5}
    assert SP.build_token_weights(v, tok, skip_ids=(0, None), top_k=2) == {"d": 2.0, "a": 0.5}      # ties by the smaller id
    assert SP.build_token_weights(v, tok, skip_ids=(0,), top_k=10) == {"a": 0.5, "d": 2.0, "e": 0.5}
    assert SP.build_token_weights(v, tok, skip_ids=(0,), top_k=0) == {}
    assert SP.build_token_weights(np.zeros(6), tok) == {}
    rng = np.random.default_rng(0)
    big = np.where(rng.random(500) < 0.3, rng.random(500), 0.0).astype(np.float32)
    d = SP.build_token_weights(big, str, skip_ids=(7,), top_k=20)
    keep = [i for i in np.argsort(-big, kind="stable") if i != 7 and big[i] > 0][:20]
    assert d == {str(i): float(big[i]) for i in keep}
    a, b = {"x": 2.0, "y": 3.0, "z": 1.0}, {"y": 0.5, "z": 4.0, "w": 7.0}
    assert SP.sparse_dot(a, b) == SP.sparse_dot(b, a) == 3.0 * 0.5 + 1.0 * 4.0 and SP.sparse_dot(a, {}) == 0.0


class _Stub:
    """stands in for the encoder: forward_splade returns the rows of a table, looked up by each row's first real token"""
    def __init__(self, table):
        self.table = table

    def forward_splade(self, ids, mask, tt=None):
        return torch.stack([self.table[int(r[1])] for r in ids])


def test_encode_compute_score_and_rerank_with_the_forward_stubbed():
    tok = R.bert_pair_tokenizer()
    V = tok.vocab_size
    words = R.X.toy_words()[:6]
    rng = np.random.default_rng(3)
    vecs = np.where(rng.random((6, V)) < 0.2, rng.random((6, V)) * 3, 0.0).astype(np.float32)
    vecs[:, tok.pad_token_id] = 5.0                                   # a weight on [PAD]: skipped by encode
    table = {tok.convert_tokens_to_ids(w): torch.from_numpy(vecs[i]) for i, w in enumerate(words)}
    model = SP.SpladeModel(_Stub(table), tokenizer=tok, device="cpu")
    texts = [w + " " + words[0] for w in words]                       # row i starts with word i
    dense = model.encode_dense(texts, batch_size=4)
    assert np.array_equal(dense.numpy(), vecs)
    dicts = model.encode(texts, batch_size=4)
    clean = vecs.copy(); clean[:, tok.pad_token_id] = 0
    for i, d in enumerate(dicts):
        assert d == {tok.convert_ids_to_tokens(int(j)): float(clean[i, j]) for j in np.flatnonzero(clean[i] > 0)}
    assert isinstance(model.encode(texts[0]), dict) and all(len(d) == 3 for d in model.encode(texts, top_k=3))
    pairs = [(texts[i], texts[(i + 1) % 6]) for i in range(6)]
    want = [float(clean[i].astype(np.float64) @ clean[(i + 1) % 6].astype(np.float64)) for i in range(6)]
    assert np.allclose(model.compute_score(pairs), want, rtol=1e-12, atol=0)
    assert np.allclose(model.compute_score(pairs[0]), want[:1], rtol=1e-12, atol=0)
    order, scores = model.rerank(texts[0], texts[1:], top_k=3)
    full = np.array([float(clean[0].astype(np.float64) @ clean[j].astype(np.float64)) for j in range(1, 6)])
    assert order.tolist() == np.lexsort((np.arange(5), -full))[:3].tolist() and np.allclose(scores.numpy(), full[order.numpy()], rtol=1e-6)


@pytest.mark.parametrize("kind,V", [("h32", 1031), ("h64", 1280)])
def test_the_bar_has_teeth_on_the_reference(kind, V):
    """On the CPU reference alone: every parity case's own output holds 30 - 90 % exact zeros, the head restated by hand is the reference, and every mutant of
    the head moves some entry by more than 10 bars."""
    w = {**U.backbone(V), **U.head(V)}
    m = U.hf_mlm(kind, V, w)
    moved = dict.fromkeys(U.MUTATIONS, 0.0)
    for name in U.CASES:
        ids, mask = U.case_batch(name, V)
        ref = U.reference(m, ids, mask)
        assert U.ZERO_SHARE[0] <= U.zero_share(ref) <= U.ZERO_SHARE[1], (name, U.zero_share(ref))
        assert (ref >= 0).all() and (ref[mask.sum(1) == 0] == 0).all()
        assert np.abs(U.by_hand(m, w, ids, mask) - ref).max() < U.BAR / 100
        if name in ("s12_left", "s40_holes", "ragged", "masked"):
            for mut in U.MUTATIONS:
                moved[mut] = max(moved[mut], float(np.abs(U.by_hand(m, w, ids, mask, mut) - ref).max()))
    assert all(v > 10 * U.BAR for v in moved.values()), moved
    assert 0 < U.BAR < 0.01          # under a hundredth of a weight of order 1
