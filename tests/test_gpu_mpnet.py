"""GPU tests of MPNet checkpoints (sentence-transformers/all-mpnet-base-v2, multi-qa-mpnet-*: MPNetModel = BERT's post-LN stack, fairseq's position rule with
padding index 1, and a learned bias per (head, bucket of the column distance) added to every attention score inside the attention kernels).  The reference is
transformers.MPNetModel in fp32 on synthetic weights.  Pooled embeddings barely see the bias (dropping an N(0, 1) table moves a mean-pooled embedding by
1 - cos ~ 1e-6), so the bias is tested on last_hidden_state, element-wise, with preconditions asserted on the reference: a zeroed table, a mirrored sign of the
distance and each bucket boundary move the compared rows by at least 10 x the bar."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpnet_util as M  # noqa: E402
import xlmr_util as X  # noqa: E402

pytestmark = pytest.mark.gpu

P = M.PAD
KR_EINVAL = -22
COS_BAR, SCORE_BAR = 5e-5, 1e-3
HIDDEN_BAR = 3e-2                        # test_g1_last_hidden_state, default mode (LayerNorm outputs of |x| <= ~4)
WIDTHS = {64: (768, 12), 32: (384, 12)}  # head width -> (H, heads)


def _hip(cfg, w):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(cfg, 0)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


def _tokens(B, S, layout, seed, vocab, lo=None):
    """(ids, mask) [B,S] int64: <s> = 0 first, real ids in [5, vocab), the pad id in every column that is not attended.  R = right-padded ragged lengths
    (S/2 .. S, one of them S), L = left-padded, F = full length."""
    rng = np.random.default_rng(seed)
    real = rng.integers(5, vocab, (B, S)); real[:, 0] = 0
    lens = rng.integers(max(2, S // 2) if lo is None else lo, S + 1, B)
    lens[0] = S
    if layout == "F":
        lens[:] = S
    ids = np.full((B, S), P, np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        n = int(lens[r])
        if layout == "L":
            ids[r, S - n:] = real[r, :n]; mask[r, S - n:] = 1
        else:
            ids[r, :n] = real[r, :n]; mask[r, :n] = 1
    return ids, mask


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


def _model(dh, L=3, sigma=4.0, vocab=1000, wname="benign", bias=None):
    H, heads = WIDTHS[dh]
    cfg = M.cfg(H, L, heads, 4 * H, vocab, 514)
    return cfg, M.weights(H, L, heads, 4 * H, vocab, 514, wname, seed=11, bias_sigma=sigma, bias=bias)


@pytest.mark.parametrize("dh", [64, 32])
def test_last_hidden_state_parity_where_the_bias_has_teeth(dh, monkeypatch):
    """kr_encoder_last_hidden against HF's last_hidden_state, element-wise on attended rows, bar 3e-2, table N(0, 4^2), benign weights, 3 layers: right-padded,
    left-padded, full-length and ragged (forward_packed) batches at S = 32, 128 (k_attn_lds), 200, 512 (k_attn_dma), both pools (CLS with a masked column 0:
    the extra query row).  Precondition per sequence, on the reference: the table zeroed and the distance mirrored are each >= 10 x the bar away."""
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")          # read at handle creation: every row of the last layer is kept under CLS pooling too
    cfg, w = _model(dh)
    h, m = _hip(cfg, w), M.hf_model(cfg, w)
    W = w[M.BIAS_NAME]
    worst, weakest = 0.0, np.inf
    for S in (32, 128, 200, 512):
        for layout in ("R", "L", "F"):
            B = 3 if S >= 200 else 5
            ids, mask = _tokens(B, S, layout, 1000 + S + ord(layout), cfg.vocab_size)
            keep = mask.astype(bool)
            M.set_bias(m, W); ref = M.hf_last_hidden(m, ids, mask)
            M.set_bias(m, 0 * W); zeroed = M.hf_last_hidden(m, ids, mask)
            M.set_bias(m, M.mirrored(W)); mirrored = M.hf_last_hidden(m, ids, mask)
            M.set_bias(m, W)
            for r in range(B):
                dz, dm = float(np.abs(ref[r] - zeroed[r])[keep[r]].max()), float(np.abs(ref[r] - mirrored[r])[keep[r]].max())
                weakest = min(weakest, dz, dm)
                assert dz >= 10 * HIDDEN_BAR and dm >= 10 * HIDDEN_BAR, ("precondition", S, layout, r, dz, dm)
            for pool in (0, 1):
                h.forward_np(ids, mask, pool)
                lh = h.last_hidden(B, S).numpy()
                err = float(np.abs(lh - ref)[keep].max())
                worst = max(worst, err)
                print(f"[d_h {dh}] S {S} {layout} pool {pool}: max |last_hidden - HF| {err:.2e}")
                assert np.isfinite(lh).all() and err <= HIDDEN_BAR, (S, layout, pool, err)
                if pool == 1 and layout == "L":
                    # the CLS row of a sequence whose column 0 is masked: a query-only row with column 0
                    e0 = float(np.abs(lh[:, 0] - ref[:, 0]).max())
                    print(f"[d_h {dh}] S {S} L cls rows (column 0, masked in {int((mask[:, 0] == 0).sum())} of {B}): {e0:.2e}")
                    assert (mask[:, 0] == 0).any() and e0 <= HIDDEN_BAR, (S, e0)
                if layout == "R":
                    rag, lens = _rag(ids, mask)
                    h.forward_packed(rag, lens, S, pool)
                    assert _same(h.last_hidden(B, S).numpy()[keep], lh[keep]), (S, pool)
    print(f"[d_h {dh}] worst |last_hidden - HF| {worst:.2e} (bar {HIDDEN_BAR}); weakest precondition distance {weakest:.2f}")


INSIDE = {8: 11, 12: 15, 16: 22, 23: 31, 32: 45, 46: 63, 64: 90}     # boundary -> the last distance of its bucket


@pytest.mark.parametrize("dh", [64, 32])
def test_every_bucket_boundary_and_the_distance_as_a_column_difference(dh):
    """Sequences of S = 256 with two attended columns c0 < c1 (<s> at c0, one word at c1, the pad id elsewhere): both tokens get positions 2 and 3 wherever they
    stand, so only the bias sees c1 - c0.  Table 2 (-1)^b (b < 16) / -2 (-1)^b (b >= 16).  Across every boundary n0 the rows for distances n0 - 1 and n0 each
    match HF within 3e-2 and differ from each other, in the reference, by >= 10 x the bar; two distances inside one bucket give bit-identical rows."""
    S = 256
    H, heads = WIDTHS[dh]
    cfg, w = _model(dh, bias=M.boundary_table(heads))
    h, m = _hip(cfg, w), M.hf_model(cfg, w)
    weakest, worst = np.inf, 0.0
    for c0 in (0, 37, 120):
        dist = sorted({n for n0 in (2, 3, 4, 5, 6, 7) + M.BOUNDARIES for n in (n0 - 1, n0)} | set(INSIDE.values()) | {219 - c0})
        assert c0 + max(dist) < S
        ids = np.full((len(dist), S), P, np.int64); mask = np.zeros((len(dist), S), np.int64)
        for r, n in enumerate(dist):
            ids[r, c0], ids[r, c0 + n] = 0, 7
            mask[r, c0] = mask[r, c0 + n] = 1
        assert (X.fairseq_positions(ids)[mask != 0].reshape(-1, 2) == [2, 3]).all()
        ref = M.hf_last_hidden(m, ids, mask)
        h.forward_np(ids, mask, 0)
        lh = h.last_hidden(len(dist), S).numpy()
        rows = {n: (lh[r, [c0, c0 + n]], ref[r, [c0, c0 + n]]) for r, n in enumerate(dist)}
        for n, (got, exp) in rows.items():
            err = float(np.abs(got - exp).max())
            worst = max(worst, err)
            assert err <= HIDDEN_BAR, (c0, n, err)
        for n0 in (2, 3, 4, 5, 6, 7) + M.BOUNDARIES:
            assert M.bucket(n0 - 1) != M.bucket(n0)
            sep = np.abs(rows[n0 - 1][1] - rows[n0][1]).max(axis=1)          # per row (the token at c0, the token at c1), in the reference
            weakest = min(weakest, float(sep.min()))
            assert (sep >= 10 * HIDDEN_BAR).all(), ("precondition", c0, n0, sep)
        for n0, n1 in list(INSIDE.items()) + [(91, 219 - c0)]:
            assert M.bucket(n0) == M.bucket(n1) and n0 != n1
            assert _same(rows[n0][0], rows[n1][0]), (c0, n0, n1)
    print(f"[d_h {dh}] worst |row - HF| {worst:.2e}; smallest separation across a boundary {weakest:.2f}")


@pytest.mark.parametrize("dh", [64, 32])
def test_one_arithmetic(dh, monkeypatch):
    """(a) a 100-token sequence alone (k_attn_lds) and next to a 300-token one (k_attn_dma): same bits.  (b) consecutive key columns and the gathered ones
    (KIRAG_AMD_ATTN_BIAS_GATHER=1 at creation forces the path of masks with holes): same bits.  (c) forward_packed == padded forward, a row does not depend on
    its batch.  (d) a zero table == a RoBERTa handle filled with the same weights under BERT's names."""
    cfg, w = _model(dh, L=2)
    h = _hip(cfg, w)
    monkeypatch.setenv("KIRAG_AMD_ATTN_BIAS_GATHER", "1")
    hg = _hip(cfg, w)
    monkeypatch.delenv("KIRAG_AMD_ATTN_BIAS_GATHER")
    rng = np.random.default_rng(5)
    for pool in (0, 1):
        # (a)
        ids = np.full((2, 300), P, np.int64); mask = np.zeros((2, 300), np.int64)
        ids[0, :100] = rng.integers(5, 1000, 100); ids[1] = rng.integers(5, 1000, 300); ids[:, 0] = 0
        mask[0, :100] = 1; mask[1] = 1
        alone = h.forward_np(ids[:1, :100], mask[:1, :100], pool)
        both = h.forward_np(ids, mask, pool)
        assert np.isfinite(both).all() and _same(alone[0], both[0]), pool
        # (b) right-padded, left-padded (the CLS row of a masked column 0) and full batches through both ways of finding the distance
        for S, layout in ((100, "R"), (300, "R"), (64, "L"), (300, "L"), (32, "F")):
            i2, m2 = _tokens(6, S, layout, 40 + S, 1000)
            a, b = h.forward_np(i2, m2, pool), hg.forward_np(i2, m2, pool)
            assert np.isfinite(a).all() and _same(a, b), (S, layout, pool)
            # (c)
            if layout == "R":
                rag, lens = _rag(i2, m2)
                assert _same(h.forward_packed(rag, lens, S, pool).cpu().numpy(), a), (S, pool)
                assert _same(h.forward_np(i2[2:5], m2[2:5], pool), a[2:5]), (S, pool)
    # (d)
    wz = dict(w); wz[M.BIAS_NAME] = np.zeros_like(w[M.BIAS_NAME])
    hz = _hip(cfg, wz)
    cr = SimpleNamespace(**{**vars(cfg), "model_type": "xlm-roberta", "type_vocab_size": 1})
    hr = _hip(cr, M.to_bert_names(w))
    assert hr.position_padding_idx == P and not hr.is_mpnet and hz.is_mpnet
    for S, layout in ((32, "R"), (128, "R"), (200, "L"), (512, "R")):
        i2, m2 = _tokens(4, S, layout, 70 + S, 1000)
        for pool in (0, 1):
            a, b = hz.forward_np(i2, m2, pool), hr.forward_np(i2, m2, pool)
            assert np.isfinite(a).all() and _same(a, b), (S, layout, pool)
    # ... and the table matters: the biased handle differs
    assert not _same(h.forward_np(i2, m2, 0), hr.forward_np(i2, m2, 0))


SHAPES = {"mpnet-base": (768, 3, 12, 3072, 30527), "tiny": (128, 2, 4, 512, 3000)}      # (H, L, heads, FF, vocab)
CASES = {"e5": [(16, 128, "R", 1), (8, 32, "R", 2), (2, 512, "R", 3), (4, 256, "L", 4), (4, 200, "F", 5)],
         "bge": [(8, 128, "R", 7), (4, 256, "L", 8), (2, 512, "F", 9)]}


@pytest.mark.parametrize("shape", ["mpnet-base", "tiny"])
@pytest.mark.parametrize("wname", ["benign", "out3"])
@pytest.mark.parametrize("sigma", [1.0, 4.0])
def test_parity_with_hf_mpnet_fp32(shape, wname, sigma):
    """The default mode against HF MPNetModel in fp32 with the encoders' pooling.  Bars: 1 - cos <= 5e-5, every e5 query x passage score
    within 1e-3 of the fp32 scores.  Measured values: profiles/mpnet/measurements.txt."""
    H, L, heads, FF, vocab = SHAPES[shape]
    cfg = M.cfg(H, L, heads, FF, vocab, 514)
    w = M.weights(H, L, heads, FF, vocab, 514, wname, bias_sigma=sigma)
    h, m = _hip(cfg, w), M.hf_model(cfg, w)
    assert h.position_padding_idx == P and h.is_mpnet
    outs, refs = {}, {}
    worst_cos = 0.0
    for tag, pool in (("e5", 0), ("bge", 1)):
        for B, S, layout, seed in CASES[tag]:
            ids, mask = _tokens(B, S, layout, seed, vocab, lo=4)
            out, ref = h.forward_np(ids, mask, pool), M.hf_encode(m, ids, mask, pool)
            assert out.shape == ref.shape and np.isfinite(out).all()
            cos = _cos_gap(out, ref)
            worst_cos = max(worst_cos, cos)
            assert cos <= COS_BAR, (tag, B, S, layout, cos)
            outs[(tag, B, S, layout)] = out; refs[(tag, B, S, layout)] = ref
    worst = 0.0
    for a in outs:
        for b in outs:
            if a[0] == b[0] == "e5":
                worst = max(worst, float(np.abs(outs[a] @ outs[b].T - refs[a] @ refs[b].T).max()))
    print(f"[{shape} {wname} sigma {sigma}] worst |q.d - ref| {worst:.2e}, worst 1 - cos {worst_cos:.2e}")
    assert worst <= SCORE_BAR, worst


def _raw_handle(max_pos=514):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(128, 1, 4, 512, 100, max_pos, 1, 1e-5)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _load(lib, h, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.kr_encoder_load_weight(h, name.encode(), a.ctypes.data, a.size)


def test_limits_and_errors():
    from kirag_amd import _lib
    from kirag_amd.retriever.encoders import HipBertForward
    H, heads = 128, 4
    cfg = M.cfg(H, 1, heads, 512, 100, 514)
    w = M.weights(H, 1, heads, 512, 100, 514)
    h = _hip(cfg, w)
    # S = 513: one more than 514 position rows allow under fairseq's rule; nothing is launched
    ids = np.full((2, 513), 7, np.int64); mask = np.ones((2, 513), np.int64)
    with pytest.raises(_lib.KiragAmdError) as ei:
        h.forward_np(ids, mask, 0)
    assert ei.value.code == KR_EINVAL and "513" in str(ei.value) and "514" in str(ei.value)
    good = h.forward_np(ids[:, :512], mask[:, :512], 0)
    assert np.isfinite(good).all()
    # a same-size reload updates the values (the weight sync reloads every parameter); another size is refused
    assert _load(h._lib, h._h, M.BIAS_NAME, np.zeros((16, heads))) == KR_EINVAL
    assert b"128" in h._lib.kr_last_error() and b"32" in h._lib.kr_last_error()
    h.load_state(w)
    assert _same(h.forward_np(ids[:, :512], mask[:, :512], 0), good)
    w2 = dict(w); w2[M.BIAS_NAME] = -w[M.BIAS_NAME]
    h.load_state(w2)
    assert not _same(h.forward_np(ids[:, :512], mask[:, :512], 0), good)
    # 64 buckets from Python: refused before a handle exists
    with pytest.raises(ValueError, match="32"):
        HipBertForward(M.cfg(H, 1, heads, 512, 100, buckets=64), 0)
    # a handle finalized without the table stays a BERT handle: MPNet's layer names are fine, the bias name is refused
    lib, raw = _raw_handle()
    try:
        assert _load(lib, raw, M.BIAS_NAME, np.zeros((16, heads))) == KR_EINVAL          # wrong size, before any finalize
        for k, v in M.to_bert_names(w).items():
            assert _load(lib, raw, k, v) == 0, k
        assert _load(lib, raw, "encoder.layer.0.attention.attn.q.weight", w["encoder.layer.0.attention.attn.q.weight"]) == 0
        assert lib.kr_encoder_finalize(raw) == 0
        assert _load(lib, raw, M.BIAS_NAME, w[M.BIAS_NAME]) == KR_EINVAL
        assert b"finalize" in lib.kr_last_error()
        out = np.empty((2, H), np.float32)
        i16, m16 = np.ascontiguousarray(ids[:, :16]), np.ascontiguousarray(mask[:, :16])
        assert lib.kr_encoder_forward(raw, i16.ctypes.data, m16.ctypes.data, 2, 16, 0, out.ctypes.data, None) == 0 and np.isfinite(out).all()
    finally:
        lib.kr_encoder_destroy(raw)
    # an unfinished MPNet handle: a slot never written is still finalize's "never loaded"
    lib, raw = _raw_handle()
    try:
        assert _load(lib, raw, M.BIAS_NAME, w[M.BIAS_NAME]) == 0
        assert lib.kr_encoder_finalize(raw) != 0 and b"never loaded" in lib.kr_last_error()
    finally:
        lib.kr_encoder_destroy(raw)


def test_graph_replay_and_both_operand_types(monkeypatch):
    """kr_encoder_forward_tt (types all 0), the hipGraph replay option and bf16 operands on an MPNet handle"""
    from kirag_amd.retriever.encoders import HipBertForward
    cfg, w = _model(32, L=2)
    h = _hip(cfg, w)
    ids, mask = _tokens(4, 64, "R", 3, 1000)
    a = h.forward_np(ids, mask, 0)
    assert _same(h.forward_np(ids, mask, 0, token_type_ids=np.zeros_like(ids)), a)
    monkeypatch.setenv("KIRAG_AMD_GRAPH", "1")
    hgr = _hip(cfg, w)
    monkeypatch.delenv("KIRAG_AMD_GRAPH")
    for _ in range(4):                                        # the first forward of a shape runs eagerly, the second captures, later ones replay
        assert _same(hgr.forward_np(ids, mask, 0), a)
    hb = HipBertForward(cfg, 0, operand_dtype="bf16")
    hb.load_state(w)
    m = M.hf_model(cfg, w)
    # bf16 operands round every stored activation to 8 significand bits (relative 2^-9 = 2e-3 per element); 1 - cos is quadratic in the relative error of the
    # pooled vector, so 1e-4 leaves a factor of ~25 over (2e-3)^2 for the accumulation over two layers
    b = hb.forward_np(ids, mask, 0)
    assert np.isfinite(b).all() and _cos_gap(b, M.hf_encode(m, ids, mask, 0)) <= 1e-4


class _Corpus:
    def __init__(self, n, words, rng):
        self.p = ["title:  " + " ".join(rng.choice(words, 2)) + ", text:  " + " ".join(rng.choice(words, int(rng.integers(3, 40)))) for _ in range(n)]
        self.index_to_passage_id = {i: str(2 * i + 5) for i in range(n)}
    def __len__(self): return len(self.p)
    def __getitem__(self, i): return {"index": i, "passage": self.p[i]}
    def get_document(self, docid): return {"id": docid, "text": self.p[(int(docid) - 5) // 2]}


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_reference_entry_points_on_a_saved_mpnet_checkpoint(tmp_path, name, pool):
    """save_pretrained a tiny MPNetModel + a fast tokenizer with MPNet's special ids; load_retriever(<existing name>, dir) returns the MPNet twin;
    cal_doc_embeddings from text -> shard files -> Indexer -> DenseRetriever(queries, topk).  The written rows equal the padded forward bit for bit and the HF
    fp32 embeddings within the bars; the hits are the exact top-k over the written rows."""
    import indep_check as IC
    from kirag_amd import compute_corpus_embeddings as CC
    from kirag_amd import faiss_index_corpus as FI
    from kirag_amd.collators import COLLATOR_MAP
    from kirag_amd.retrieve import setup_retriever_model
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import InBatchRetriever, load_retriever
    words = X.toy_words(400)
    tok = X.toy_tokenizer(words)
    vocab = tok.vocab_size
    H, L, heads, FF = 128, 2, 4, 512
    cfg = M.cfg(H, L, heads, FF, vocab, 514)
    w = M.weights(H, L, heads, FF, vocab, 514, "out3", bias_sigma=2.0)
    td = str(tmp_path / "model")
    m = M.hf_model(cfg, w, device="cpu")
    m.save_pretrained(td)
    tok.save_pretrained(td)
    twin = {"E5Retriever": ENC.MPNetE5Encoder, "BGERetriever": ENC.MPNetBGEEncoder}[name]
    assert type(load_retriever(name, td)) is twin
    rng = np.random.default_rng(9)
    corpus = _Corpus(1500, words, rng)
    tag = name.lower()
    enc_args = CC.setup_parser(["--retriever_name", name, "--retriever_model_name_or_path", td, "--tokenizer_name_or_path", td, "--save_dir", str(tmp_path),
                                "--name", tag, "--index_folder", "c", "--doc_maxlength", "48", "--per_gpu_batch_size", "8",
                                "--num_passage_per_index_file", "500", "--encode_batch_size", "256", "--tokenizer_workers", "0"])
    ret = InBatchRetriever(name, td, temperature=0.01)
    assert type(ret.encoder) is twin and ret.hidden_size == H
    col = COLLATOR_MAP[name](tokenizer=tok, query_maxlength=24, doc_maxlength=48)
    CC.cal_doc_embeddings(enc_args, ret, corpus, col)
    assert ret.encoder._hip.position_padding_idx == 1 and ret.encoder._hip.is_mpnet
    folder = os.path.join(str(tmp_path), tag, "c")
    assert len([f for f in os.listdir(folder) if f.startswith("corpus_embeddings_")]) == 3
    FI.build_faiss_index(FI.setup_parser(["--index_folder", folder, "--embedding_size", str(H)]))
    args = SimpleNamespace(retriever_name=name, tokenizer_name_or_path=td, query_maxlength=24, doc_maxlength=48, retriever_model_name_or_path=td, local_rank=-1,
                           corpus="unused", index_folder=folder, embedding_size=H, per_gpu_batch_size=8)
    dr, _ = setup_retriever_model(args, corpus_dataset=corpus, tokenizer=tok)
    assert type(dr.retriever.encoder) is twin
    x = dr.indexer.index.reconstruct_n(0, 1500)
    assert x.shape == (1500, H)
    a = col.encode_doc(corpus.p[:256])
    ids, mask = a["input_ids"].numpy(), a["attention_mask"].numpy()
    assert (ids[mask == 0] == 1).all() and (mask == 0).any()
    padded = dr.retriever.doc({"input_ids": a["input_ids"].cuda(), "attention_mask": a["attention_mask"].cuda()}).cpu().numpy()
    assert _same(padded, np.ascontiguousarray(x[:256]))
    mg = m.float().eval().cuda()
    ref = M.hf_encode(mg, ids, mask, pool)
    cos = _cos_gap(x[:256], ref)
    dscore = float(np.abs(x[:256] @ x[:256].T - ref @ ref.T).max())
    print(f"[{name}] written rows vs HF fp32: 1 - cos {cos:.2e}, |q.d - ref| {dscore:.2e}")
    assert cos <= COS_BAR and dscore <= SCORE_BAR
    qs = [corpus.p[40].split("text:  ")[1], corpus.p[1499].split("text:  ")[1][:40], " ".join(words[:5])]
    k = 10
    out = dr(qs, topk=k)
    qv = dr.calculate_query_embeddings(qs).numpy()
    qa = col.encode_query(qs)
    assert _cos_gap(qv, M.hf_encode(mg, qa["input_ids"].numpy(), qa["attention_mask"].numpy(), pool)) <= COS_BAR
    rs, ri = IC.torch_topk_fp32(torch.from_numpy(qv).cuda(), [(0, torch.from_numpy(x).cuda())], k + 8)
    rows = np.array([[(int(d["id"]) - 5) // 2 for d in out[r]] for r in range(len(qs))])
    s = np.array([[d["score"] for d in out[r]] for r in range(len(qs))], np.float32)
    IC.check_membership(s, rows, rs.cpu().numpy(), ri.cpu().numpy(), k)
