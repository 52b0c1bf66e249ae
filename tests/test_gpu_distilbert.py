"""GPU tests of the DistilBERT family: DistilBertModel's layer stack on a BERT handle without token types (kirag_amd.retriever.encoders.distilbert_rename), against
HF fp32 with eager attention on attended rows; the twins through the registry classes, with and without ``pipeline="checkpoint"``.  Synthetic weights
(oracle.encoder_np's BERT weights under DistilBERT's names, a nonzero position table and token-type row so that dropping the one or adding the other shows);
no DistilBERT checkpoint exists offline."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import has_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
if has_gpu():
    import st_util as U
    from kirag_amd.retriever.encoders import BGEEncoder, DistilBertBGEEncoder, DistilBertE5Encoder, E5Encoder, HipBertForward, distilbert_rename
    from oracle import encoder_np as E

HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
H, FF, VOCAB, MAX_POS = 128, 256, 200, 160


def _case(heads, L=2, seed=13):
    cfg = U.distil_config(H, L, heads, FF, VOCAB, MAX_POS)
    bert = E.synth_weights(H, L, FF, VOCAB, MAX_POS, seed=seed)
    return cfg, bert, U.to_distil_names(bert)


def _handle(cfg, w):
    h = HipBertForward(cfg, 0, rename=distilbert_rename)
    h.load_state(w)
    return h


@pytest.mark.parametrize("heads", [2, 4])
def test_last_hidden_state_against_hf_where_positions_and_token_types_have_teeth(heads):
    cfg, bert, w = _case(heads)
    hf = U.distil_model(cfg, w)
    h = _handle(cfg, w)
    assert h._zero_type_row and not h.is_mpnet and not h.is_decoder      # a BERT handle with a zero token-type row
    # the two mistakes, in the reference: no position table; BERT's token-type row 0 added to every embedding
    no_pos = dict(w); no_pos["embeddings.position_embeddings.weight"] = np.zeros_like(w["embeddings.position_embeddings.weight"])
    typed = dict(w); typed["embeddings.word_embeddings.weight"] = w["embeddings.word_embeddings.weight"] + bert["embeddings.token_type_embeddings.weight"][0]
    hf_no_pos, hf_typed = U.distil_model(cfg, no_pos), U.distil_model(cfg, typed)
    worst, weakest = 0.0, np.inf
    for S in (12, 40, 150):
        for layout, holes in (("R", 0), ("L", 0), ("R", 3)):
            ids, mask = U.tokens(4, S, layout, 3 * S + holes, vocab=VOCAB, holes=holes)
            keep = mask != 0
            ref = U.hf_last_hidden(hf, ids, mask)
            h.forward_np(ids, mask, U.POOL_MEAN)
            lh = h.last_hidden(4, S).numpy()
            err = float(np.abs(lh - ref)[keep].max())
            worst = max(worst, err)
            assert np.isfinite(lh).all() and not lh[~keep].any() and err <= HIDDEN_BAR, (S, layout, holes, err)
            for what, m in (("no position table", hf_no_pos), ("BERT's token-type row", hf_typed)):
                d = float(np.abs(U.hf_last_hidden(m, ids, mask) - ref)[keep].max())
                weakest = min(weakest, d)
                assert d > 10 * HIDDEN_BAR, ("precondition", what, S, layout, d)
    print(f"[distilbert, {heads} heads] worst |last_hidden - HF| {worst:.2e} (bar {HIDDEN_BAR}); weakest precondition distance {weakest:.2f} (required {10 * HIDDEN_BAR})")


def _cos_gap(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((1 - (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)).max())


def test_the_twins_through_the_registry_classes_and_a_dot_product_folder(tmp_path):
    """E5Encoder / BGEEncoder.from_pretrained on a distilbert folder return the family's twins; eval mode runs the HIP path within the project's embedding bars.  With
    ``pipeline="checkpoint"`` a TAS-B-shaped folder (CLS pooling, no Normalize) gives the CLS row itself, within the last_hidden_state bar."""
    cfg, _, w = _case(2)
    hf = U.distil_model(cfg, w)
    d = str(tmp_path / "distil")
    hf.save_pretrained(d)
    ids, mask = U.tokens(6, 40, "R", 5, vocab=VOCAB)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    lh = torch.from_numpy(U.hf_last_hidden(hf, ids, mask))
    for cls, twin, pooling in ((E5Encoder, DistilBertE5Encoder, "mean"), (BGEEncoder, DistilBertBGEEncoder, "cls")):
        m = cls.from_pretrained(d).cuda().eval()
        assert type(m) is twin
        got = m(ti, tm).cpu().numpy()
        want = U.tail_torch(lh, tm, pooling).numpy()
        cos, ds = _cos_gap(got, want), float(np.abs(got @ got.T - want @ want.T).max())
        assert cos <= COS_BAR and ds <= SCORE_BAR, (pooling, cos, ds)
        tok = torch.from_numpy(np.concatenate([ids[r, :int(mask[r].sum())] for r in range(6)]).astype(np.int32)).cuda()
        assert torch.equal(m.forward_packed(tok, torch.from_numpy(mask.sum(1).astype(np.int32)).cuda(), 40), m(ti, tm))
    U.write_pipeline(d, H, pooling=("cls",), normalize=False)
    m = E5Encoder.from_pretrained(d, pipeline="checkpoint").cuda().eval()
    assert type(m) is DistilBertE5Encoder and m._st.pooling == "cls" and not m._st.normalize
    got = m(ti, tm).cpu().numpy()
    want = U.tail_torch(lh, tm, "cls", normalize=False).numpy()
    assert float(np.abs(got - want).max()) <= HIDDEN_BAR and float(np.abs(np.linalg.norm(want, axis=1) - 1).min()) > 0.1
    m.train()
    with torch.no_grad():
        assert float((m(ti.cuda(), tm.cuda()).cpu() - torch.from_numpy(want)).abs().max()) <= 1e-4      # the same tail in torch on HF's forward


def test_checkpoint_check_tool_with_the_folders_own_pipeline(tmp_path):
    """tools/checkpoint_check.py --pipeline checkpoint on a distiluse-shaped folder (CLS -> Dense(tanh) -> Normalize) and on a TAS-B-shaped one (CLS, not normalised),
    without a tokenizer (seeded random tokens): the worst element-wise deviation is reported next to 1 - cos, inside the bars"""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(repo, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    cfg, _, w = _case(2)
    d = str(tmp_path / "distil")
    U.distil_model(cfg, w).save_pretrained(d)
    W, b = U.dense_weights(H, 132, seed=4, scale=2.0)
    U.write_pipeline(d, H, pooling=("cls",), dense=(W, b, U.TANH))
    out = cc.check(d, cc.parse([d, "--n", "8", "--max-length", "48", "--random-tokens", "--pipeline", "checkpoint"]))
    assert out["pipeline"] == {"pooling": "cls", "dense": [132, H], "bias": True, "activation": "tanh", "normalize": True} and out["finite"]
    assert out["worst_1_minus_cos"] <= COS_BAR and out["worst_score_error"] <= SCORE_BAR, out
    U.write_pipeline(d, H, pooling=("cls",), normalize=False)
    out = cc.check(d, cc.parse([d, "--n", "8", "--max-length", "48", "--random-tokens", "--pipeline", "checkpoint"]))
    assert out["pipeline"]["dense"] is None and not out["pipeline"]["normalize"] and out["finite"]
    assert out["worst_elementwise_deviation"] <= HIDDEN_BAR and out["largest_reference_element"] > 1.0, out
