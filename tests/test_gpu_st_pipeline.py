"""GPU tests of the sentence-transformers tail on the HIP path: config.normalize_output / config.pool_tokens / config.st_dense_activation and the head st_dense.*.

k_pool / k_pool_tok are held against the rows kr_encoder_last_hidden returns for the SAME forward (both decode the final rows with lo_decode_final's rule, so the
max is exact and the sums are inside an a-priori fp32 bound); k_st_dense against float64 on the library's own pooled rows; every mode is bit-identical alone, in
a batch, reversed, left-padded and from the ragged entry point; BERT / MPNet / decoder twins against HF fp32 (eager attention) + the tail written in torch
(tests/st_util.py — recalled from sentence-transformers, which is not installed here, not checked against it).  Synthetic weights, one or two layers."""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import has_gpu  # noqa: E402

from kirag_amd.retriever.encoders import StPipeline  # noqa: E402  (a dataclass: the parametrised cases are built from it at collection, without a GPU)

pytestmark = pytest.mark.gpu
if has_gpu():
    import decoder_util as D
    import mpnet_util as M
    import st_util as U
    from kirag_amd import _lib
    from kirag_amd.retriever.encoders import HipBertForward
    from oracle import encoder_np as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u = 2.0 ** -24
HIDDEN_BAR, COS_BAR, SCORE_BAR = 3e-2, 5e-5, 1e-3
# Dense outputs against HF fp32 + the torch tail: twice the worst deviation measured on an MI355X (profiles/st_pipeline/measurements.txt: 7.21e-3, the decoder twin
# with 2 heads of 64, whose rows themselves are 2.9e-3 off; the BERT and MPNet twins: 6.7e-4)
DENSE_BAR = 1.45e-2
FF, VOCAB, MAX_POS = 256, 200, 160
LENS = (1, 15, 16, 17, 63, 64, 65, 129, 0)                 # the wave-count (16) and unroll (64 = 16 x 4) edges of k_pool, more than one step, nothing


def bert_cfg(H, L=1, heads=None, ff=FF, vocab=VOCAB, max_pos=MAX_POS):
    return SimpleNamespace(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads or H // 64, intermediate_size=ff, vocab_size=vocab,
                           max_position_embeddings=max_pos, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", model_type="bert")


def handle(cfg, w, pipe=None, dense=None):
    h = HipBertForward(cfg, 0, pipeline_settings=pipe.settings() if pipe is not None else ())
    w = dict(w)
    if dense is not None:
        w["st_dense.weight"] = dense[0]
        if dense[1] is not None:
            w["st_dense.bias"] = dense[1]
    h.load_state(w)
    return h


def ragged(lens, S, seed=7):
    rng = np.random.default_rng(seed)
    ids = np.zeros((len(lens), S), np.int64); mask = np.zeros((len(lens), S), np.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = rng.integers(3, VOCAB, n); mask[r, :n] = 1
    return ids, mask


def test_the_setting_and_the_head_are_known_and_the_handle_forwards():
    """Fails on a library without the feature: config.normalize_output is an unknown setting and st_dense.weight an unknown tensor there."""
    cfg = bert_cfg(128)
    w = E.synth_weights(128, 1, FF, VOCAB, MAX_POS, seed=5)
    W, b = U.dense_weights(128, 8)
    h = handle(cfg, w, StPipeline("max", normalize=False, activation="tanh"), (W, b))
    assert h.out_dim == 8
    ids, mask = ragged((5, 9), 12)
    out = h.forward_np(ids, mask, U.POOL_MEAN)
    assert out.shape == (2, 8) and np.isfinite(out).all() and np.abs(out).max() <= 1.0
    h.check()
    # after the first finalize: the same values are a no-op, anything else is refused
    one = torch.tensor([1.0])
    assert h._lib.kr_encoder_load_weight(h._h, b"config.pool_tokens", one.data_ptr(), 1) == 0
    assert h._lib.kr_encoder_load_weight(h._h, b"config.normalize_output", one.data_ptr(), 1) != 0
    assert np.array_equal(h.forward_np(ids, mask, U.POOL_MEAN), out)


@pytest.fixture(scope="module")
def pooled():
    """per H: the ragged batch, last_hidden of its forward, and the rows of the four KR_POOL_MEAN variants (one handle each, same weights)"""
    out = {}
    for H in (128, 384, 640):
        cfg = bert_cfg(H)
        w = E.synth_weights(H, 1, FF, VOCAB, MAX_POS, seed=H)
        ids, mask = ragged(LENS, 129, seed=H)
        rows, lh = {}, None
        for name, pipe in (("norm", None), ("mean", StPipeline("mean", normalize=False)), ("max", StPipeline("max", normalize=False)),
                           ("sqrt", StPipeline("mean_sqrt_len", normalize=False)), ("max_norm", StPipeline("max"))):
            h = handle(cfg, w, pipe)
            rows[name] = h.forward_np(ids, mask, U.POOL_MEAN)
            h.check()                                       # the all-masked sequence raises no error bit: KR_OK
            got = h.last_hidden(len(LENS), 129).numpy()
            assert lh is None or np.array_equal(got, lh)    # the stack does not depend on the tail
            lh = got
            if name == "mean":
                rows["cls"] = h.forward_np(ids, mask, U.POOL_CLS)
        out[H] = (rows, lh)
    return out


@pytest.mark.parametrize("H", [128, 384, 640])
def test_pool_variants_against_the_rows_of_the_same_forward(pooled, H):
    rows, lh = pooled[H]
    for b, n in enumerate(LENS):
        if n == 0:      # nothing attended: NaN under all three, like the mean of nothing
            for name in ("norm", "mean", "max", "sqrt", "max_norm"):
                assert np.isnan(rows[name][b]).all(), name
            continue
        x = lh[b, :n].astype(np.float64)
        # max: the numbers themselves (array_equal leaves the sign of a zero open)
        assert np.array_equal(rows["max"][b], lh[b, :n].max(0)), ("max", n)
        # mean, not normalised: n - 1 additions and one division in fp32
        bound = (n + 2) * u * np.abs(x).sum(0)
        err = np.abs(rows["mean"][b] - x.mean(0))
        assert (err <= bound).all(), ("mean", n, float((err / np.maximum(bound, 1e-300)).max()))
        # ... divided by its float64 norm it is the normalised handle's row: a sum of H squares, a root and a division in fp32
        m64 = rows["mean"][b].astype(np.float64)
        unit = m64 / np.linalg.norm(m64)
        assert (np.abs(rows["norm"][b] - unit) <= (H + 2) * u * np.abs(unit)).all(), ("norm", n)
        mx = rows["max"][b].astype(np.float64)
        assert (np.abs(rows["max_norm"][b] - mx / np.linalg.norm(mx)) <= (H + 2) * u * np.abs(mx / np.linalg.norm(mx))).all(), ("max_norm", n)
        # sum / sqrt(n): the kernel's mean times sqrt(n) within two roundings (2 ulp = 2^-22 relative cover the division of the mean, the root and the division by it,
        # half an ulp each)
        ref = m64 * np.sqrt(n)
        assert (np.abs(rows["sqrt"][b] - ref) <= 2 * 2.0 ** -23 * np.abs(ref)).all(), ("sqrt", n)
        # CLS, not normalised: the row itself
        assert np.array_equal(rows["cls"][b], lh[b, 0]), ("cls", n)


def test_last_token_rows_unnormalised_are_the_rows_themselves():
    cfg = D.hf_config("llama-64", L=1, max_pos=MAX_POS)
    h = HipBertForward(cfg, 0, pipeline_settings=StPipeline("last", normalize=False).settings())
    h.load_state(D.weights(cfg))
    ids, mask = ragged((1, 17, 64, 0, 33), 64)
    out = h.forward_np(ids, mask, U.POOL_LAST)
    h.check()
    lh = h.last_hidden(5, 64).numpy()
    for b, n in enumerate((1, 17, 64, 0, 33)):
        if n == 0:
            assert np.isnan(out[b]).all()
        else:
            assert np.array_equal(out[b], lh[b, n - 1]), n
    # config.pool_tokens changes what a KR_POOL_MEAN forward pools and nothing else: the last row under the max setting is the same row
    h2 = HipBertForward(cfg, 0, pipeline_settings=StPipeline("max", normalize=False).settings())
    h2.load_state(D.weights(cfg))
    assert np.array_equal(h2.forward_np(ids, mask, U.POOL_LAST), out, equal_nan=True)
    got = h2.forward_np(ids, mask, U.POOL_MEAN)
    assert np.array_equal(got[2], h2.last_hidden(5, 64).numpy()[2].max(0))


DENSE_CASES = [(H, P) for H in (128, 640, 2048) for P in (4, 132, 512, 2048)]


@pytest.fixture(scope="module")
def raw_rows():
    """per H the library's own pooled rows: the not-normalised mean of a 5-sequence batch (one all-masked), and the sequences' token counts"""
    out = {}
    for H in (128, 640, 2048):
        cfg = bert_cfg(H, ff=128, vocab=50, max_pos=64)
        w = E.synth_weights(H, 1, 128, 50, 64, seed=H + 1)
        rng = np.random.default_rng(H)
        lens = (9, 33, 0, 20, 5)
        ids = np.zeros((5, 40), np.int64); mask = np.zeros((5, 40), np.int64)
        for r, n in enumerate(lens):
            ids[r, :n] = rng.integers(3, 50, n); mask[r, :n] = 1
        h = handle(cfg, w, StPipeline("mean", normalize=False))
        out[H] = (cfg, w, ids, mask, h.forward_np(ids, mask, U.POOL_MEAN))
    return out


@pytest.mark.parametrize("case", range(len(DENSE_CASES)))
def test_st_dense_inside_its_a_priori_fp32_bound(raw_rows, case):
    """k_st_dense alone, whatever the encoder's error: on the library's own pooled rows x, act(W x + b) is within gamma_H (sum |w x| + |b|) of float64 (a sum of
    H products in some order plus the bias: gamma_H = (H + 2) u / (1 - (H + 2) u)), through tanh's Lipschitz constant 1 plus 4 u |y| for tanhf itself (documented
    to 2 ulp); normalised, the bound travels through y / |y| to first order plus the (P + 2) u of the norm's own fp32 arithmetic.  B = 1, 4, 5: a partial group of
    PD_SEQ = 4, a full one, full + 1.  Bias, activation and normalisation are derived from the indices (hi, pi) of H and P so that each of the three takes both its
    values at every H (over its four P) and at every P (over its three H): bias = (hi + pi) odd, tanh = bit 1 of hi + pi, normalised = (hi + 2 pi) % 3 == 0."""
    H, P = DENSE_CASES[case]
    hi, pi = case // 4, case % 4
    bias, tanh, norm = bool((hi + pi) & 1), bool(((hi + pi) >> 1) & 1), (hi + 2 * pi) % 3 == 0
    cfg, w, ids, mask, x = raw_rows[H]
    W, b = U.dense_weights(H, P, seed=case, bias=bias, scale=2.0)
    h = handle(cfg, w, StPipeline("mean", normalize=norm, activation="tanh" if tanh else "identity"), (W, b))
    assert h.out_dim == P
    full = None
    for B in (5, 4, 1):
        got = h.forward_np(ids[:B], mask[:B], U.POOL_MEAN)
        h.check()
        assert got.shape == (B, P)
        if full is None:
            full = got
        assert np.array_equal(got, full[:B], equal_nan=True), B      # a row does not depend on its batch
    g = (H + 2) * u / (1 - (H + 2) * u)
    for r in range(5):
        if not mask[r].any():
            assert np.isnan(full[r]).all()
            continue
        x64, W64 = x[r].astype(np.float64), W.astype(np.float64)
        pre = W64 @ x64 + (b.astype(np.float64) if bias else 0.0)
        bound = g * (np.abs(W64) @ np.abs(x64) + (np.abs(b) if bias else 0.0))
        y = np.tanh(pre) if tanh else pre
        if tanh:
            bound = bound + 4 * u * np.abs(y)
        if norm:
            n2 = np.linalg.norm(y)
            bound = bound / n2 + np.abs(y) * np.linalg.norm(bound) / n2 ** 2 + (P + 2) * u * np.abs(y) / n2
            y = y / n2
        err = np.abs(full[r] - y)
        assert (err <= bound).all(), (H, P, bias, tanh, norm, r, float((err / np.maximum(bound, 1e-300)).max()))


MODES = {"max_norm": (StPipeline("max"), False), "sqrt": (StPipeline("mean_sqrt_len", normalize=False), False),
         "mean_dense_tanh": (StPipeline("mean", normalize=False, activation="tanh"), True), "cls_dense_norm": (StPipeline("cls"), True),
         "max_dense": (StPipeline("max", normalize=False), True), "mean": (StPipeline("mean", normalize=False), False),
         "last": (StPipeline("last", normalize=False), False), "last_dense": (StPipeline("last", activation="tanh"), True)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_sequence_does_not_depend_on_its_surroundings(mode):
    """alone, in a batch, in the reversed batch, right- / left-padded, from kr_encoder_forward_packed: the same bits.  (Left padding on a rotary handle: with a position
    table the column IS the position, and a left-padded sequence another input.)"""
    pipe, with_dense = MODES[mode]
    H = 384
    pool = U.POOL_CLS if pipe.pooling == "cls" else U.POOL_LAST if pipe.pooling == "last" else U.POOL_MEAN
    if pool == U.POOL_CLS:
        cfg = bert_cfg(H, 2)
        w = E.synth_weights(H, 2, FF, VOCAB, MAX_POS, seed=9)
    else:       # a rotary handle (Qwen2-style, 6 heads of 64 over 2 KV heads): no position table, so a left-padded sequence IS the same sequence
        cfg = D.hf_config("qwen2-384", L=2, max_pos=MAX_POS)
        w = D.weights(cfg)
    h = handle(cfg, w, pipe, U.dense_weights(H, 132, seed=2) if with_dense else None)
    lens = (17, 40, 1, 33, 8)
    ids, mask = ragged(lens, 40, seed=3)
    batch = h.forward_np(ids, mask, pool)
    assert np.isfinite(batch).all()
    assert np.array_equal(h.forward_np(ids[::-1], mask[::-1], pool)[::-1], batch)
    for r, n in enumerate(lens):
        assert np.array_equal(h.forward_np(ids[r:r + 1], mask[r:r + 1], pool)[0], batch[r]), ("alone", r)
        assert np.array_equal(h.forward_np(ids[r:r + 1, :n], mask[r:r + 1, :n], pool)[0], batch[r]), ("narrow", r)
    if pool != U.POOL_CLS:      # (the CLS row of a left-padded batch is another row)
        lids = np.zeros_like(ids); lmask = np.zeros_like(mask)
        for r, n in enumerate(lens):
            lids[r, 40 - n:] = ids[r, :n]; lmask[r, 40 - n:] = 1
        assert np.array_equal(h.forward_np(lids, lmask, pool), batch)
    tok = torch.from_numpy(np.concatenate([ids[r, :n] for r, n in enumerate(lens)]).astype(np.int32)).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    packed = h.forward_packed(tok, ln, 40, pool)
    h.check()
    assert np.array_equal(packed.cpu().numpy(), batch)


# ---- parity with HF fp32 (eager attention) + the tail in torch ----
def _twin(kind):
    """(handle config, library weights, HF model on the CPU, extra forward kwargs) of a two-layer twin, H = 128 with 2 heads of 64 or 4 of 32"""
    family, heads = kind.split("-")
    heads = {"64": 2, "32": 4}[heads]
    if family == "bert":
        from transformers import BertConfig, BertModel
        w = E.synth_weights(128, 2, FF, VOCAB, MAX_POS, seed=21)
        cfg = bert_cfg(128, 2, heads)
        hc = BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=heads, intermediate_size=FF, vocab_size=VOCAB, max_position_embeddings=MAX_POS,
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        hc._attn_implementation = "eager"
        m = BertModel(hc, add_pooling_layer=False)
        assert not m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False).missing_keys
        return cfg, w, m.float().eval()
    if family == "mpnet":
        cfg = M.cfg(128, 2, heads, FF, VOCAB, MAX_POS + 2)
        w = M.weights(128, 2, heads, FF, VOCAB, MAX_POS + 2)
        return cfg, w, M.hf_model(cfg, w, device="cpu")
    cfg = D.hf_config("llama-64" if heads == 2 else "qwen2-32", L=2, max_pos=MAX_POS)
    w = D.weights(cfg)
    return cfg, w, D.hf_model(cfg, w)


def _cos_gap(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((1 - (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)).max())


@pytest.mark.parametrize("kind", ["bert-64", "bert-32", "mpnet-64", "mpnet-32", "decoder-64", "decoder-32"])
def test_parity_with_hf_and_the_torch_tail(kind):
    cfg, w, hf = _twin(kind)
    decoder = kind.startswith("decoder")
    W, b = U.dense_weights(128, 132, seed=31, scale=2.0)
    one_row = "last" if decoder else "cls"
    handles = {"max": handle(cfg, w, StPipeline("max", normalize=False)), "mean": handle(cfg, w, StPipeline("mean", normalize=False)),
               "dense": handle(cfg, w, StPipeline("mean_sqrt_len", normalize=False, activation="tanh"), (W, b)),
               "row": handle(cfg, w, StPipeline(one_row), (W, b))}
    worst = {"rows": 0.0, "dense": 0.0, "cos": 0.0, "score": 0.0}
    teeth = {k: 0.0 for k in ("normalising anyway", "mean for max", "masked columns in the max", "no Dense bias", "identity for tanh", "Normalize in front of the Dense")}
    for S in (12, 40, 150):
        for layout, holes in (("R", 0), ("L", 0), ("R", 3)):
            ids, mask = U.tokens(4, S, layout, S + holes, vocab=VOCAB, holes=holes)
            lh = torch.from_numpy(U.hf_last_hidden(hf, ids, mask))
            tm = torch.from_numpy(mask)
            ref = {"max": U.tail_torch(lh, tm, "max", normalize=False), "mean": U.tail_torch(lh, tm, "mean", normalize=False),
                   "dense": U.tail_torch(lh, tm, "mean_sqrt_len", W, b, "tanh", normalize=False)}
            for name in ("max", "mean", "dense"):
                got = handles[name].forward_np(ids, mask, U.POOL_MEAN)
                err = float(np.abs(got - ref[name].numpy()).max())
                key = "dense" if name == "dense" else "rows"
                worst[key] = max(worst[key], err)
                print(f"[{kind}] S {S} {layout} holes {holes} {name}: |out - ref| {err:.2e}")
                assert np.isfinite(got).all() and err <= (DENSE_BAR if name == "dense" else HIDDEN_BAR), (name, S, layout, holes, err)
            if layout == "R" or decoder:      # (the first column of a left-padded batch is masked: HF's row there is an artefact of its finite mask value)
                got = handles["row"].forward_np(ids, mask, U.POOL_LAST if decoder else U.POOL_CLS)
                want = U.tail_torch(lh, tm, one_row, W, b).numpy()
                cos, ds = _cos_gap(got, want), float(np.abs(got @ got.T - want @ want.T).max())
                worst["cos"], worst["score"] = max(worst["cos"], cos), max(worst["score"], ds)
                assert cos <= COS_BAR and ds <= SCORE_BAR, (S, layout, holes, cos, ds)
            # what each mistake would move, in the reference (every attended row is compared: 100 %)
            d = lambda a, c: float((a - c).abs().max())
            teeth["normalising anyway"] = max(teeth["normalising anyway"], d(ref["max"], U.tail_torch(lh, tm, "max")) / HIDDEN_BAR)
            teeth["mean for max"] = max(teeth["mean for max"], d(ref["max"], ref["mean"]) / HIDDEN_BAR)
            if layout == "R" and holes == 0 and S > 12:     # (right padding: HF's rows at the masked columns are ordinary finite values, which the broken max lets in)
                teeth["masked columns in the max"] = max(teeth["masked columns in the max"], d(ref["max"], U.tail_torch(lh, tm, "max", normalize=False, masked_in_max=True)) / HIDDEN_BAR)
            teeth["no Dense bias"] = max(teeth["no Dense bias"], d(ref["dense"], U.tail_torch(lh, tm, "mean_sqrt_len", W, None, "tanh", normalize=False)) / DENSE_BAR)
            teeth["identity for tanh"] = max(teeth["identity for tanh"], d(ref["dense"], U.tail_torch(lh, tm, "mean_sqrt_len", W, b, "identity", normalize=False)) / DENSE_BAR)
            teeth["Normalize in front of the Dense"] = max(teeth["Normalize in front of the Dense"],
                                                           d(ref["dense"], U.tail_torch(lh, tm, "mean_sqrt_len", W, b, "tanh", normalize=False, normalize_first=True)) / DENSE_BAR)
    print(f"[{kind}] worst: rows {worst['rows']:.2e} (bar {HIDDEN_BAR}), dense {worst['dense']:.2e} (bar {DENSE_BAR}), 1 - cos {worst['cos']:.2e} (bar {COS_BAR}), "
          f"score {worst['score']:.2e} (bar {SCORE_BAR}); teeth in bars: " + ", ".join(f"{k} {v:.0f}" for k, v in teeth.items()))
    for k, v in teeth.items():
        assert v > 10, ("precondition", k, v)


def test_unnormalised_passages_in_an_indexer_keep_hfs_dot_product_order():
    """64 passages and 8 queries of a BERT handle with config.normalize_output = 0 (a dot-product checkpoint): Indexer.search_knn returns HF's order wherever HF's
    scores differ by more than twice the score bar.  The bar: the project's 1e-3 on unit vectors, scaled by the two lengths |q| |d| of each pair."""
    from kirag_amd.retriever.index import Indexer
    cfg, w, hf = _twin("bert-64")
    h = handle(cfg, w, StPipeline("mean", normalize=False))
    ids, mask = U.tokens(72, 40, "R", 77, vocab=VOCAB)
    got = h.forward_np(ids, mask, U.POOL_MEAN)
    ref = U.tail_torch(torch.from_numpy(U.hf_last_hidden(hf, ids, mask)), torch.from_numpy(mask), "mean", normalize=False).numpy().astype(np.float64)
    q, d, rq, rd = got[:8], got[8:], ref[:8], ref[8:]
    assert float(np.abs(np.linalg.norm(rd, axis=1) - 1).min()) > 0.1            # not unit vectors
    index = Indexer(128)
    index.index_data(list(range(64)), d)
    hits = index.search_knn(q, 64, verbose=False)
    want = rq @ rd.T
    bar = SCORE_BAR * np.linalg.norm(rq, axis=1)[:, None] * np.linalg.norm(rd, axis=1)[None, :]
    decided = 0
    for i, (names, scores) in enumerate(hits):
        order = [int(x) for x in names]
        assert sorted(order) == list(range(64))
        assert (np.abs(np.asarray(scores) - want[i, order]) <= bar[i, order]).all(), float(np.abs(np.asarray(scores) - want[i, order]).max())
        rank = np.empty(64, np.int64); rank[order] = np.arange(64)
        for j in range(64):
            for k in range(64):
                if want[i, j] - want[i, k] > 2 * max(bar[i, j], bar[i, k]):
                    decided += 1
                    assert rank[j] < rank[k], (i, j, k)
    assert decided > 8 * 64 * 63 // 4      # the bar leaves most pairs decided


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def unchanged_handle_digests():
    """sha256 of one forward each of four handles that carry none of the feature: an e5-large-shaped BERT (two of its 24 layers), an MPNet, a T5 with dense.weight,
    a Qwen2-style decoder — what tools and this test share, so that the parent commit's library can be asked the same question"""
    import t5_util as T
    out = {}
    cfg = bert_cfg(1024, 2, ff=4096)
    ids, mask = U.tokens(8, 64, "R", 1, vocab=VOCAB)
    h = handle(cfg, E.synth_weights(1024, 2, 4096, VOCAB, MAX_POS, seed=1))
    out["e5_large_shape_mean"] = _digest(h.forward_np(ids, mask, U.POOL_MEAN)); out["e5_large_shape_cls"] = _digest(h.forward_np(ids, mask, U.POOL_CLS))
    mc = M.cfg(128, 2, 2, FF, VOCAB, MAX_POS + 2)
    h = handle(mc, M.weights(128, 2, 2, FF, VOCAB, MAX_POS + 2))
    out["mpnet_mean"] = _digest(h.forward_np(ids, mask, U.POOL_MEAN))
    tw = T.weights(128, 2, 2, FF, VOCAB)
    tw["dense.weight"] = T.dense_weight(64, 128)
    h = handle(T.cfg(128, 2, 2, FF, VOCAB), tw)
    out["t5_dense_mean"] = _digest(h.forward_np(ids, mask, U.POOL_MEAN))
    dc = D.hf_config("qwen2-32", L=2, max_pos=MAX_POS)
    h = handle(dc, D.weights(dc))
    out["qwen2_last"] = _digest(h.forward_np(ids, mask, U.POOL_LAST)); out["qwen2_mean"] = _digest(h.forward_np(ids, mask, U.POOL_MEAN))
    return out


def test_handles_without_the_feature_compute_what_the_parent_commit_computed():
    """profiles/st_pipeline/unchanged_handles.json holds the digests of the PARENT commit's library (recorded on an MI355X by running unchanged_handle_digests with
    that library loaded); this library must give the same bits"""
    with open(os.path.join(REPO, "profiles", "st_pipeline", "unchanged_handles.json")) as f:
        recorded = json.load(f)["digests"]
    assert unchanged_handle_digests() == recorded


if __name__ == "__main__":      # python tests/test_gpu_st_pipeline.py: the digests as JSON (run with KIRAG_AMD_LIB naming the parent commit's library to record them)
    print(json.dumps({"library": _lib.LIB_PATH, "digests": unchanged_handle_digests()}, indent=1))
