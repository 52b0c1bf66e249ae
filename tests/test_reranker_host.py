"""Host-side tests of the cross-encoder rerankers: the two parameter-name maps on the real HF task classes, the dispatch of BGEReranker.from_pretrained and
its refusals, BaseReranker.score / rerank (shape, order, ties) with the HIP forward stubbed, the two pair collators on toy tokenizers, and the fences of the
C header (one new #define, the same 50 functions, ABI 9)."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reranker_util as R  # noqa: E402

from oracle import encoder_np as E  # noqa: E402
from kirag_amd import _lib  # noqa: E402
from kirag_amd.collators import COLLATOR_MAP, BGEKGChainRerankerCollator, RerankerCollator  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever import rerankers as RR  # noqa: E402
from kirag_amd.retriever.retrievers import RETRIEVER_MAP  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(H=64, layers=2, heads=2, FF=128)


def _tiny(kind, labels=1, cls=None):
    c = R.cfg(kind, TINY["H"], TINY["layers"], TINY["heads"], TINY["FF"], labels)
    return R.hf_classifier(kind, c, R.weights(kind, TINY["H"], TINY["layers"], TINY["FF"], labels), cls=cls)


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_rename_maps_cover_the_hf_task_models(kind):
    """every parameter of the HF class lands on a name the library knows — BERT's backbone names or one of the four head names — each exactly once, and nothing
    containing `pooler.` reaches the library"""
    m = _tiny(kind, labels=3)
    rename = RR.xlmr_rename if kind == "xlmr" else RR.bert_rename
    known = set(E.bert_param_shapes(TINY["H"], TINY["layers"], TINY["FF"], R.VOCAB)) | set(R.HEAD)
    names = [rename(n) for n, _ in m.named_parameters()]
    assert set(names) == known and len(names) == len(known)
    assert not any("pooler." in n for n in names)
    shapes = {rename(n): tuple(p.shape) for n, p in m.named_parameters()}
    assert shapes[R.HEAD[0]] == (64, 64) and shapes[R.HEAD[1]] == (64,) and shapes[R.HEAD[2]] == (3, 64) and shapes[R.HEAD[3]] == (3,)
    twin = RR.XLMRobertaReranker if kind == "xlmr" else RR.BertReranker
    assert twin._hip_rename is rename and twin._pool == ENC.POOL_CLASSIFY == 2
    # the sentence encoders take the unchanged path
    assert ENC.E5Encoder._hip_rename is None and ENC.XLMRobertaBGEEncoder._hip_rename is None


def test_the_mixins_share_one_copy_of_the_weight_sync():
    for name in ("_synced_hip", "_hip_forward", "invalidate_hip_weights", "train", "load_state_dict", "_apply"):
        assert getattr(RR.XLMRobertaReranker, name) is getattr(ENC.E5Encoder, name) is getattr(RR.BertReranker, name), name
    assert set(RETRIEVER_MAP) == set(COLLATOR_MAP) == {"E5Retriever", "BGERetriever"} and set(RR.RERANKER_MAP) == {"BGEReranker"}


def test_dispatch_by_model_type_and_refusals(tmp_path):
    from transformers import BertForSequenceClassification, XLMRobertaForSequenceClassification
    dirs = {}
    for kind in ("xlmr", "bert"):
        dirs[kind] = str(tmp_path / kind)
        _tiny(kind).save_pretrained(dirs[kind])
    x = RR.load_reranker("BGEReranker", dirs["xlmr"])
    assert type(x) is RR.XLMRobertaReranker and isinstance(x, XLMRobertaForSequenceClassification) and not x.training and x.config.num_labels == 1
    b = RR.BGEReranker.from_pretrained(dirs["bert"])
    assert type(b) is RR.BertReranker and isinstance(b, BertForSequenceClassification)
    ref = _tiny("bert")
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(b.named_parameters(), ref.named_parameters()))
    with pytest.raises(KeyError, match="BGEReranker"):
        RR.load_reranker("NoSuchReranker", dirs["bert"])
    # a CPU model in eval mode: no fallback, as for the encoders; train mode is HF's forward
    ids, mask, tt = R.pairs("bert", 3, 16, seed=1)
    args = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), token_type_ids=torch.from_numpy(tt))
    with pytest.raises(RuntimeError, match="HIP path only"):
        b(**args)
    out = b.train()(**args).logits
    assert out.requires_grad and out.shape == (3, 1) and np.abs(out.detach().double().numpy() - R.hf_logits(ref, ids, mask, tt)).max() < 1e-6
    # other families, too many labels: refused by name
    d = str(tmp_path / "modern")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:        # the dispatch reads the checkpoint's config.json and nothing else
        json.dump({"model_type": "modernbert", "architectures": ["ModernBertForSequenceClassification"], "hidden_size": 64}, f)
    with pytest.raises(NotImplementedError, match="modernbert"):
        RR.load_reranker("BGEReranker", d)
    d = str(tmp_path / "many")
    _tiny("bert", labels=65).save_pretrained(d)
    with pytest.raises(NotImplementedError, match="num_labels=65"):
        RR.load_reranker("BGEReranker", d)
    _tiny("xlmr", labels=64, cls=RR.XLMRobertaReranker)


def _stubbed(tmp_path, monkeypatch, labels=1, **kw):
    """a BaseReranker whose HIP forward is replaced by a function of the batch: label l of a pair = (number of attended tokens % 5) + 10 l"""
    d = str(tmp_path / "ckpt")
    _tiny("xlmr", labels=labels).save_pretrained(d)
    rr = RR.BaseReranker("BGEReranker", d, **kw)
    rr.eval()
    calls = []

    def fake(self, input_ids, attention_mask, token_type_ids):
        calls.append(tuple(input_ids.shape))
        n = attention_mask.sum(1, keepdim=True).float() % 5
        return n + 10.0 * torch.arange(self.config.num_labels)[None, :]

    monkeypatch.setattr(RR.XLMRobertaReranker, "_hip_forward", fake)
    return rr, calls


def test_score_and_rerank_with_the_forward_stubbed(tmp_path, monkeypatch):
    tok = R.xlmr_pair_tokenizer()
    rr, calls = _stubbed(tmp_path, monkeypatch, tokenizer=tok, maxlength=48)
    assert isinstance(rr, torch.nn.Module) and rr.device == torch.device("cpu") and rr.to("cpu") is rr
    query, ps = "aa0 bb27", R.passages(23, seed=3, lo=1, hi=30)
    col = rr._collator()
    args = col.encode_pairs([query] * 23, ps)
    s = rr.score(args=args)
    assert s.shape == (23,) and torch.equal(s, args["attention_mask"].sum(1).float() % 5)
    assert len(set(s.tolist())) == 5                                        # many ties
    expect = sorted(range(23), key=lambda i: (-float(s[i]), i))
    del calls[:]
    idx, scores = rr.rerank(query, ps, batch_size=4)
    assert idx.tolist() == expect and torch.equal(scores, s[idx]) and len(calls) == 6
    # length-sorted batches: no batch is wider than its longest pair, and the widths do not decrease
    lens = args["attention_mask"].sum(1).tolist()
    assert [c[1] for c in calls] == [sorted(lens)[min(4 * (b + 1), 23) - 1] for b in range(6)]
    idx1, scores1 = rr.rerank(query, ps, batch_size=64)
    assert torch.equal(idx1, idx) and torch.equal(scores1, scores)
    top, top_s = rr.rerank(query, ps, top_k=3)
    assert top.tolist() == expect[:3] and torch.equal(top_s, scores[:3])
    assert RR.rank_order([1.0, 3.0, 3.0, -1.0, 3.0]).tolist() == [1, 2, 4, 0, 3]
    # save_model / load_model as BaseRetriever has them
    rr.save_model(str(tmp_path / "saved"))
    rr.load_model(str(tmp_path / "saved"))
    assert type(rr.reranker) is RR.XLMRobertaReranker


def test_score_keeps_the_label_axis_for_more_than_one_label(tmp_path, monkeypatch):
    rr, _ = _stubbed(tmp_path, monkeypatch, labels=3, tokenizer=R.xlmr_pair_tokenizer())
    ids, mask, _ = R.pairs("xlmr", 4, 16, seed=2)
    s = rr.score({"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)})
    assert s.shape == (4, 3) and torch.equal(s[:, 2] - s[:, 0], torch.full((4,), 20.0))
    with pytest.raises(ValueError, match="3 labels"):
        rr.rerank("aa0", ["bb27 cc14"])


def test_pair_collators_on_toy_tokenizers():
    words = R.X.toy_words()
    q, p = " ".join(words[:3]), " ".join(words[10:15])
    long_p = " ".join(words[20:80])
    # XLM-R: <s> A </s></s> B </s>, no token types
    tok = R.xlmr_pair_tokenizer()
    col = RerankerCollator(tok, maxlength=24)
    enc = col.encode_pairs([q, q], [p, long_p])
    assert set(enc) == {"input_ids", "attention_mask"} and enc["input_ids"].shape == (2, 24) and enc["input_ids"].dtype == torch.int64
    v = tok.get_vocab()
    row = enc["input_ids"][0].tolist()
    assert row[:12] == [0, *[v[w] for w in words[:3]], 2, 2, *[v[w] for w in words[10:15]], 2] and set(row[12:]) == {1}
    assert enc["attention_mask"][0].tolist() == [1] * 12 + [0] * 12
    # the passage side alone is truncated: the query whole, then </s></s>, 24 - 7 passage words, </s>
    row = enc["input_ids"][1].tolist()
    assert row == [0, *[v[w] for w in words[:3]], 2, 2, *[v[w] for w in words[20:37]], 2]
    # BERT: [CLS] A [SEP] B [SEP] with token types 0...0 1...1
    btok = R.bert_pair_tokenizer()
    bcol = RerankerCollator(btok, maxlength=24)
    benc = bcol.encode_pairs([q, q], [p, long_p])
    bv = btok.get_vocab()
    assert set(benc) == {"input_ids", "attention_mask", "token_type_ids"}
    assert benc["input_ids"][0].tolist()[:11] == [R.B_CLS, *[bv[w] for w in words[:3]], R.B_SEP, *[bv[w] for w in words[10:15]], R.B_SEP]
    assert benc["token_type_ids"][0].tolist() == [0] * 5 + [1] * 6 + [0] * 13
    assert benc["input_ids"][1].tolist() == [R.B_CLS, *[bv[w] for w in words[:3]], R.B_SEP, *[bv[w] for w in words[20:38]], R.B_SEP]
    assert benc["token_type_ids"][1].tolist() == [0] * 5 + [1] * 19
    # the unpadded rows + pad() are the padded call
    rows = bcol.tokenize_pairs([q, q], [p, long_p])
    assert [len(r["input_ids"]) for r in rows] == [11, 24]
    again = bcol.pad(rows)
    assert all(torch.equal(again[k], benc[k]) for k in benc)
    assert bcol.pad(rows[:1])["input_ids"].shape == (1, 11)
    with pytest.raises(ValueError):
        col.encode_pairs([q], [p, p])
    # the chain collator: the call shape of the reference's loop; the passage is the chain's texts joined by one space
    kg = BGEKGChainRerankerCollator(tokenizer=tok, maxlength=24)
    chains = [[" ".join(words[10:12]), " ".join(words[12:15])], [long_p]]
    args, labels, index = kg([{"index": 0, "questions": [q, q], "reasoning_chains": chains, "labels": [0, 1]}])
    assert all(torch.equal(args[k], enc[k]) for k in enc) and labels.tolist() == [0, 1] and index.tolist() == [0]
    args2, labels2, index2 = kg([{"index": 4, "questions": [q], "reasoning_chains": chains[:1], "labels": [1]},
                                 {"index": 9, "questions": [q], "reasoning_chains": chains[1:], "labels": [0]}])
    assert torch.equal(args2["input_ids"], enc["input_ids"]) and labels2.tolist() == [1, 0] and index2.tolist() == [4, 9]


def test_header_gains_one_define_and_no_function():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert re.search(r"^#define KR_POOL_CLASSIFY 2\b", hdr, re.M) and re.search(r"^#define KR_ABI_VERSION 9\b", hdr, re.M)
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50 and _lib.ABI_VERSION == 9
    for name in R.HEAD:
        assert '"%s"' % name in hdr or name.replace("classifier.", "") in hdr
    assert "classifier.dense.weight" in hdr and "classifier.out_proj.weight" in hdr and "KR_ESTATE" in hdr
