"""Host-side tests of bge-m3's heads (no GPU): the header's two flag macros on an unchanged ABI, the layout bookkeeping of a flagged forward, lexical
weights / lexical matching / MaxSim / the hybrid scores on literal values, the ``.pt`` round trip of the two head files, refusals that name the field, the
registry entry, and the preconditions the GPU tests' bars rest on (every mutant of the heads far outside them, the ReLU cutting through the reference's
tokens) checked on the CPU reference."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3_util as M  # noqa: E402
import xlmr_util as X  # noqa: E402

from kirag_amd import _lib  # noqa: E402
from kirag_amd.retriever import encoders as ENC  # noqa: E402
from kirag_amd.retriever import m3 as M3  # noqa: E402
from kirag_amd.retriever import rerankers as RR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_gains_two_flags_and_no_function():
    hdr = open(os.path.join(REPO, "include", "kirag_amd.h")).read()
    assert re.search(r"^#define KR_POOL_WITH_SPARSE 0x10\b", hdr, re.M) and re.search(r"^#define KR_POOL_WITH_COLBERT 0x20\b", hdr, re.M)
    assert re.search(r"^#define KR_ABI_VERSION 9\b", hdr, re.M)
    declared = set(re.findall(r"\b(kr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES) and len(declared) == 50 and _lib.ABI_VERSION == 9
    for name in M.HEADS:
        assert '"%s"' % name in hdr
    assert (ENC.POOL_WITH_SPARSE, ENC.POOL_WITH_COLBERT) == (0x10, 0x20)


def test_layout_of_a_flagged_forward_is_three_views_into_one_tensor():
    h = ENC.HipBertForward.__new__(ENC.HipBertForward)
    h.out_dim, h.num_labels, h.colbert_dim, h._h = 128, 3, 256, None
    B, S = 5, 7
    assert h._out_shape(ENC.POOL_CLS, B, S) == (B, 128) and h._out_shape(ENC.POOL_CLASSIFY, B, S) == (B, 3)
    both = ENC.POOL_CLS | ENC.POOL_WITH_SPARSE | ENC.POOL_WITH_COLBERT
    assert h._out_shape(both, B, S) == (B * 128 + B * S + B * S * 256,)
    assert h._out_shape(ENC.POOL_MEAN | ENC.POOL_WITH_COLBERT, B, S) == (B * 128 + B * S * 256,)
    flat = torch.arange(B * 128 + B * S + B * S * 256, dtype=torch.float32)
    d, s, c = h._blocks(flat, both, B, S)
    assert d.shape == (B, 128) and s.shape == (B, S) and c.shape == (B, S, 256)
    assert d[0, 0] == 0 and s[0, 0] == B * 128 and c[0, 0, 0] == B * 128 + B * S and c[-1, -1, -1] == flat[-1]
    assert d.data_ptr() == flat.data_ptr() and c.data_ptr() == flat.data_ptr() + 4 * (B * 128 + B * S)      # views, not copies
    d, s, c = h._blocks(flat[:B * 128 + B * S], ENC.POOL_CLS | ENC.POOL_WITH_SPARSE, B, S)
    assert s.shape == (B, S) and c is None
    plain = torch.zeros(B, 128)
    assert h._blocks(plain, ENC.POOL_CLS, B, S) is plain


def test_lexical_weights_from_hand_made_weights_and_ids():
    skip = {0, 1, 2, 3}
    ids = [0, 17, 44, 17, 3, 90, 91, 2]
    w = [0.9, 0.25, 0.5, 0.75, 0.8, 0.0, -0.3, 0.6]
    # <s> / <unk> / </s> skipped, the repeated id keeps its max, 0 and negative weights dropped
    assert M3.build_lexical_weights(ids, w, skip) == {"17": 0.75, "44": 0.5}
    assert M3.build_lexical_weights(ids, w, set()) == {"0": 0.9, "17": 0.75, "44": 0.5, "3": 0.8, "2": 0.6}
    assert M3.build_lexical_weights([], [], skip) == {}
    assert M3.build_lexical_weights([5, 5], [0.125, 0.0625], {None, 1}) == {"5": 0.125}


def test_scores_on_literal_arrays():
    a, b = {"17": 0.5, "44": 0.25, "9": 1.0}, {"44": 2.0, "17": 0.5, "8": 4.0}
    assert M3.compute_lexical_matching_score(a, b) == M3.compute_lexical_matching_score(b, a) == 0.75
    assert M3.compute_lexical_matching_score(a, {}) == 0.0 and M3.BGEM3Model.compute_lexical_matching_score(a, b) == 0.75
    q = np.array([[1.0, 0.0], [0.0, 1.0], [0.6, 0.8]])
    p = np.array([[1.0, 0.0], [0.6, 0.8]])
    # row maxima 1.0, 0.8, 1.0 -> mean
    assert M3.colbert_score(q, p) == pytest.approx((1.0 + 0.8 + 1.0) / 3, abs=1e-7)
    assert M3.colbert_score(torch.tensor(p), torch.tensor(q)) == pytest.approx(1.0, abs=1e-7)       # not symmetric: the mean runs over the FIRST argument's rows
    assert M3.colbert_score(np.zeros((0, 2)), p) == 0.0
    s = M3.combine_scores(0.5, 0.25, 1.0, (0.4, 0.2, 0.4))
    assert s["dense"] == 0.5 and s["sparse"] == 0.25 and s["colbert"] == 1.0
    assert s["sparse+dense"] == pytest.approx((0.4 * 0.5 + 0.2 * 0.25) / 0.6) and s["colbert+sparse+dense"] == pytest.approx(0.4 * 0.5 + 0.2 * 0.25 + 0.4 * 1.0)
    assert M3.combine_scores(0.5, 0.25, 1.0, (1, 1, 1))["colbert+sparse+dense"] == pytest.approx(1.75 / 3)


class _Stub:
    """what BGEM3Model needs of a model: forward_m3 on a fixed table of outputs per token id"""
    P = 2

    def forward_m3(self, ids, mask, return_sparse=True, return_colbert=True):
        self.calls = getattr(self, "calls", 0) + 1
        B, S = ids.shape
        dense = torch.zeros(B, 2); dense[:, 0] = 1.0
        sparse = (ids.float() / 100.0) * mask if return_sparse else None
        ang = ids.float() * 0.1
        colbert = torch.stack([torch.cos(ang), torch.sin(ang)], -1) * mask[..., None] if return_colbert else None
        return dense, sparse, colbert


def test_compute_score_and_rerank_on_a_stub_model():
    tok = X.toy_tokenizer()
    m = M3.BGEM3Model(_Stub(), tokenizer=tok, device="cpu")
    words = X.toy_words()
    q, p1, p2 = f"{words[0]} {words[1]}", f"{words[1]} {words[2]} {words[1]}", words[5]
    i0, i1, i2, i5 = (tok.convert_tokens_to_ids(words[i]) for i in (0, 1, 2, 5))
    out = m.encode([q, p1, p2], return_sparse=True, return_colbert_vecs=True)
    assert m.model.calls == 1                                                    # one forward per batch, whatever is asked for
    assert out["lexical_weights"] == [{str(i0): pytest.approx(i0 / 100), str(i1): pytest.approx(i1 / 100)},
                                      {str(i1): pytest.approx(i1 / 100), str(i2): pytest.approx(i2 / 100)}, {str(i5): pytest.approx(i5 / 100)}]
    assert [v.shape for v in out["colbert_vecs"]] == [(3, 2), (4, 2), (2, 2)]     # without <s>, with </s>, without padding
    assert out["colbert_vecs"][0][-1] == pytest.approx([np.cos(0.2), np.sin(0.2)])       # </s> = id 2
    one = m.encode(q, return_sparse=True)
    assert one["dense_vecs"].shape == (2,) and isinstance(one["lexical_weights"], dict) and one["colbert_vecs"] is None
    s = m.compute_score([(q, p1), (q, p2)], weights=(0.4, 0.2, 0.4))
    assert set(s) == {"dense", "sparse", "colbert", "sparse+dense", "colbert+sparse+dense"} and all(len(v) == 2 for v in s.values())
    assert s["dense"] == pytest.approx([1.0, 1.0]) and s["sparse"] == pytest.approx([(i1 / 100) ** 2, 0.0])
    # MaxSim by hand: query tokens i0, i1, </s>; the passage holds i1 and </s>, so two of the three maxima are 1
    best = max(np.cos(0.1 * (i0 - j)) for j in (i1, i2, 2))
    assert s["colbert"][0] == pytest.approx((best + 2.0) / 3, abs=1e-6)
    assert s["colbert+sparse+dense"][0] == pytest.approx(0.4 * 1.0 + 0.2 * (i1 / 100) ** 2 + 0.4 * s["colbert"][0], abs=1e-6)
    order, top = m.rerank(q, [p2, p1], weights=(0.4, 0.2, 0.4))
    assert order.tolist() == [1, 0] and top[0] == pytest.approx(s["colbert+sparse+dense"][0], abs=1e-6) and top[0] > top[1]
    assert m.rerank(q, [p2, p1], top_k=1)[0].tolist() == [1]
    with pytest.raises(ValueError, match="padding_side"):
        M3.BGEM3Model(_Stub(), tokenizer=X.toy_tokenizer(padding_side="left"), device="cpu").encode([q])
    with pytest.raises(ValueError, match="normalize_embeddings"):
        M3.BGEM3Model(_Stub(), tokenizer=tok, normalize_embeddings=False)


def _tiny(kind):
    cls = M3.XLMRobertaM3Encoder if kind == "xlmr" else M3.BertM3Encoder
    return M.hf_backbone(kind, M.backbone(kind), "cpu", cls=cls)


def _states(hw):
    return ({"weight": torch.from_numpy(hw[M.HEADS[0]]), "bias": torch.from_numpy(hw[M.HEADS[1]])},
            {"weight": torch.from_numpy(hw[M.HEADS[2]]), "bias": torch.from_numpy(hw[M.HEADS[3]])})


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_the_two_head_files_round_trip(kind, tmp_path):
    hw = M.heads(128, 256)
    m = _tiny(kind)
    assert m.colbert_linear is None and m.sparse_linear is None and not [n for n, _ in m.named_parameters() if "linear" in n]
    m.set_heads(*_states(hw))
    names = [n for n, _ in m.named_parameters()]
    assert set(M.HEADS) <= set(names)                          # the four names travel through the ordinary weight sync
    d = str(tmp_path / "both")
    m.save_pretrained(d)
    assert {M3.COLBERT_FILE, M3.SPARSE_FILE} <= set(os.listdir(d))
    assert set(torch.load(os.path.join(d, M3.COLBERT_FILE), weights_only=True)) == {"weight", "bias"}
    assert m.colbert_linear is not None                        # save_pretrained puts the heads back
    back = type(m).from_pretrained(d)
    assert type(back) is type(m) and not back.training
    for name in ("colbert_linear", "sparse_linear"):
        a, b = getattr(m, name), getattr(back, name)
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    assert back.colbert_linear.out_features == 256 and back.sparse_linear.out_features == 1
    # the backbone's own files hold the backbone only: the plain HF class loads them without unexpected keys
    from transformers import BertModel, XLMRobertaModel
    plain, info = (XLMRobertaModel if kind == "xlmr" else BertModel).from_pretrained(d, add_pooling_layer=False, output_loading_info=True)
    assert not info["unexpected_keys"] and not info["missing_keys"]
    # either file may be absent: that head is then not offered
    os.remove(os.path.join(d, M3.SPARSE_FILE))
    half = type(m).from_pretrained(d)
    assert half.sparse_linear is None and half.colbert_linear is not None
    assert not [n for n, _ in half.named_parameters() if n.startswith("sparse_linear")]
    with pytest.raises(ValueError, match="sparse_linear"):
        half.forward_m3(torch.zeros(1, 4, dtype=torch.long), torch.ones(1, 4, dtype=torch.long), return_sparse=True, return_colbert=False)
    # the registry reaches it
    model = RR.load_reranker("BGEM3", d, tokenizer=X.toy_tokenizer(), device="cpu")
    assert isinstance(model, M3.BGEM3Model) and type(model.model) is type(m) and RR.HYBRID_RERANKER_MAP["BGEM3"] is M3.BGEM3Model


def test_refusals_name_the_field(tmp_path):
    hw = M.heads(128, 128)
    col, sp = _states(hw)
    x = _tiny("xlmr")
    d = str(tmp_path / "x")
    x.set_heads(col, sp)
    x.save_pretrained(d)
    # another model_type, by name, for both twins and for the front end
    with pytest.raises(NotImplementedError, match="model_type='xlm-roberta'"):
        M3.BertM3Encoder.from_pretrained(d)
    b = str(tmp_path / "b")
    _tiny("bert").save_pretrained(b)
    with pytest.raises(NotImplementedError, match="model_type='bert'"):
        M3.XLMRobertaM3Encoder.from_pretrained(b)
    from transformers import MPNetConfig, MPNetModel
    mp = str(tmp_path / "mp")
    MPNetModel(MPNetConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=64)).save_pretrained(mp)
    with pytest.raises(NotImplementedError, match="model_type='mpnet'"):
        M3.BGEM3Model(mp, tokenizer=X.toy_tokenizer(), device="cpu")
    # a colbert_linear that does not read the hidden size; a P outside the library's rule; a sparse head with two outputs; a missing key
    bad = {"in_features": ({"weight": torch.zeros(128, 64), "bias": torch.zeros(128)}, M3.COLBERT_FILE, r"colbert_linear\.in_features=64"),
           "P": ({"weight": torch.zeros(192, 128), "bias": torch.zeros(192)}, M3.COLBERT_FILE, r"colbert_linear\.out_features=192"),
           "P big": ({"weight": torch.zeros(2176, 128), "bias": torch.zeros(2176)}, M3.COLBERT_FILE, r"colbert_linear\.out_features=2176"),
           "sparse": ({"weight": torch.zeros(2, 128), "bias": torch.zeros(2)}, M3.SPARSE_FILE, r"sparse_linear\.out_features=2"),
           "bias": ({"weight": torch.zeros(128, 128), "bias": torch.zeros(64)}, M3.COLBERT_FILE, r"colbert_linear\.bias"),
           "keys": ({"weight": torch.zeros(128, 128)}, M3.COLBERT_FILE, r"colbert_linear")}
    for what, (state, fname, pattern) in bad.items():
        good = torch.load(os.path.join(d, fname), weights_only=True)
        torch.save(state, os.path.join(d, fname))
        try:
            with pytest.raises(ValueError, match=pattern):
                M3.XLMRobertaM3Encoder.from_pretrained(d)
        finally:
            torch.save(good, os.path.join(d, fname))
    with pytest.raises(ValueError, match="out_features=64"):
        ENC.check_colbert_dim(64)
    for P in (128, 1024, 2048):
        ENC.check_colbert_dim(P)
    # eval mode only, and no CPU fallback
    with pytest.raises(RuntimeError, match="eval"):
        x.train().forward_m3(torch.zeros(1, 4, dtype=torch.long), torch.ones(1, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="HIP path only"):
        x.eval().forward_m3(torch.zeros(1, 4, dtype=torch.long), torch.ones(1, 4, dtype=torch.long))


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_the_bars_have_teeth_on_the_reference(kind):
    """On the CPU reference alone: every mutant of the heads moves the block it touches by more than 10 bars, and the sparse bias leaves at least a quarter of
    the attended tokens positive and a quarter clipped."""
    hw = M.heads_for(kind, 128)
    m = M.hf_backbone(kind, M.backbone(kind))
    pos = att = 0
    for S in (12, 40):
        for variant in ("right", "left", "holes"):
            ids, mask = M.batch(kind, 5, S, variant, seed=S + (0 if kind == "xlmr" else 1000))
            lh = M.last_hidden(m, ids, mask)
            ref_s, ref_c = M.ref_blocks(lh, mask, hw)
            k = mask != 0
            assert (ref_s[~k] == 0).all() and (ref_c[~k] == 0).all()
            pos += int((ref_s[k] > 0).sum()); att += int(k.sum())
            for mut in M.MUTATIONS:
                mut_s, mut_c = M.ref_blocks(lh, mask, hw, broken=mut)
                if mut in ("no_colbert_bias", "no_norm", "neighbour_row"):
                    assert M.colbert_errors(mut_c, ref_c, mask)[1] > 10 * M.BARS["colbert_elem"], (mut, S, variant)
                else:
                    assert np.array_equal(mut_c, ref_c)
                if mut in ("no_sparse_bias", "no_relu", "neighbour_row"):
                    assert np.abs(mut_s - ref_s)[k].max() > 10 * M.BARS["sparse"], (mut, S, variant)
                else:
                    assert np.array_equal(mut_s, ref_s)
    assert 0.25 <= pos / att <= 0.75, pos / att
    assert abs(float(hw[M.HEADS[3]][0])) > 10 * M.BARS["sparse"]
    # the bars stay under the project's ceilings
    assert M.SCORE_BAR == 1e-3 and M.BARS["colbert_elem"] < 1e-3 and M.BARS["sparse"] < 1e-3
