"""GPU tests of RoBERTa-family checkpoints (intfloat/multilingual-e5-*, the dense head of BAAI/bge-m3: XLMRobertaModel, fairseq's position rule with padding
index P = 1, 250 002 tokens, 514 / 8194 position rows): parity with HF XLMRobertaModel in fp32 with the encoders' pooling at the project's bars (DESIGN.md §2:
1 - cos <= 5e-5 per embedding, every query x passage score within 1e-3 of the fp32 scores), the new position rule tied bit for bit to BERT's rule on a
shifted position table, ragged == padded and batch invariance under the new rule, sequences up to 8192 tokens, the limits, and the reference's entry points
(load_retriever -> cal_doc_embeddings -> shard files -> Indexer -> DenseRetriever) on a saved XLM-R checkpoint under the two existing registry names."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xlmr_util as X  # noqa: E402

pytestmark = pytest.mark.gpu

P = X.PAD
KR_EINVAL = -22
COS_BAR, SCORE_BAR = 5e-5, 1e-3
SHAPES = {                          # (H, L, heads, FF, vocab)
    "xlmr-base": (768, 3, 12, 3072, 30000),
    "xlmr-large": (1024, 4, 16, 4096, 250002),
    "tiny": (128, 2, 4, 512, 30000),
}


def _hip(cfg, w):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(cfg, 0)
    h.load_state(w)
    return h


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cos_gap(out, ref):
    return float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())


def _tokens(B, S, layout, seed, vocab):
    """(ids, mask) [B,S] int64.  Real ids come from the top of the vocabulary down to 5 (never P); every column that is not a real token holds P unless the
    layout says otherwise.  R = right-padded ragged, L = left-padded, F = full length, and the layouts only fairseq's rule tells apart: a = P inside an
    attended sequence, b = a masked column holding a non-P id in front of the attended ones (left-padded), c = an attended tail of P."""
    rng = np.random.default_rng(seed)
    real = rng.integers(5, vocab, (B, S)); real[:, 1] = vocab - 1; real[:, 0] = 0      # <s> first, the top of the vocabulary next
    lo = 4 if layout in "abc" else 1
    lens = rng.integers(lo, S + 1 - (2 if layout in "bc" else 0), B)
    if layout not in "bc":
        lens[0] = S
    if layout == "F":
        lens[:] = S
    ids = np.full((B, S), P, np.int64); mask = np.zeros((B, S), np.int64)
    for r in range(B):
        n = int(lens[r])
        if layout in ("L", "b"):
            ids[r, S - n:] = real[r, :n]; mask[r, S - n:] = 1
            if layout == "b":
                ids[r, 0] = 7                                  # masked, not P: it counts
        else:
            ids[r, :n] = real[r, :n]; mask[r, :n] = 1
            if layout == "a":
                ids[r, rng.integers(1, n - 1)] = P             # attended P: position P, does not advance the count
            if layout == "c":
                mask[r, n:n + 1 + r % 2] = 1                   # attended tail of P
    if layout in "abc":
        assert all(X.differs_from_simple_rules(ids[r], mask[r]) for r in range(B)), layout
    return ids, mask


# (B, S, layout, seed)
CASES = {"e5": [(64, 128, "R", 1), (16, 32, "R", 2), (2, 512, "R", 3), (4, 256, "L", 4), (8, 128, "F", 5), (6, 64, "a", 11), (6, 64, "b", 12), (6, 200, "c", 13)],
         "bge": [(8, 128, "R", 7), (4, 256, "L", 8), (2, 512, "F", 9), (6, 200, "a", 14), (6, 64, "b", 15), (6, 64, "c", 16)]}


@pytest.mark.parametrize("shape", ["xlmr-base", "xlmr-large", "tiny"])
@pytest.mark.parametrize("wname", ["benign", "out3"])
def test_parity_with_hf_xlm_roberta_fp32(shape, wname):
    """The default mode (f16 operands + residual low half) against HF XLMRobertaModel in fp32 with the encoders' pooling; HF's own position_ids are the
    expectation in every layout.  Bars: 1 - cos <= 5e-5, every e5 query x passage score within 1e-3 of the fp32 scores.
    Measured on MI355X (worst |q.d - ref| / worst 1 - cos): xlmr-base benign 2.5e-5 / 1.2e-7, out3 4.9e-5 / 1.2e-7; xlmr-large benign 2.7e-5 / 1.8e-7,
    out3 1.1e-4 / 1.2e-7; tiny benign 5.1e-6 / 1.2e-7, out3 1.3e-5 / 1.8e-7 (profiles/xlmr/measurements.txt)."""
    H, L, heads, FF, vocab = SHAPES[shape]
    cfg = X.cfg(H, L, heads, FF, vocab, 514)
    w = X.weights(H, L, FF, vocab, 514, wname)
    h, m = _hip(cfg, w), X.hf_model(cfg, w)
    assert h.position_padding_idx == P
    outs, refs = {}, {}
    worst_cos = 0.0
    for tag, pool in (("e5", 0), ("bge", 1)):
        for B, S, layout, seed in CASES[tag]:
            ids, mask = _tokens(B, S, layout, seed, vocab)
            out, ref = h.forward_np(ids, mask, pool), X.hf_encode(m, ids, mask, pool)
            assert out.shape == ref.shape and np.isfinite(out).all()
            cos = _cos_gap(out, ref)
            worst_cos = max(worst_cos, cos)
            print(f"[{shape} {wname}] {tag} {B}x{S} {layout}: 1 - cos {cos:.2e}")
            assert cos <= COS_BAR, (tag, B, S, layout, cos)
            outs[(tag, B, S, layout)] = out; refs[(tag, B, S, layout)] = ref
    worst = 0.0
    for a in outs:
        for b in outs:
            if a[0] == b[0] == "e5":
                worst = max(worst, float(np.abs(outs[a] @ outs[b].T - refs[a] @ refs[b].T).max()))
    print(f"[{shape} {wname}] worst |q.d - ref| {worst:.2e}, worst 1 - cos {worst_cos:.2e}")
    assert worst <= SCORE_BAR, worst


def _small(L=2, max_pos=514, heads=12, H=384):
    cfg = X.cfg(H, L, heads, 4 * H, 1000, max_pos)
    return cfg, X.weights(H, L, 4 * H, 1000, max_pos, "benign", seed=11)


def _rag(ids, mask):
    return torch.from_numpy(np.ascontiguousarray(ids[mask != 0].astype(np.int32))), torch.from_numpy(mask.sum(1).astype(np.int32))


@pytest.mark.parametrize("S", [32, 128, 512])
def test_fairseq_rule_equals_berts_rule_on_a_shifted_position_table_bit_for_bit(S):
    """Right-padded input without P inside: position = column + P + 1, so a fairseq-rule handle equals, in every output bit, a BERT-rule handle loaded with the
    same weights and the position table shifted by P + 1 rows.  Both pools, padded and ragged entry point."""
    cfg, w = _small()
    h = _hip(cfg, w)
    k = [n for n in w if n.endswith("position_embeddings.weight")][0]
    wb = dict(w); wb[k] = np.ascontiguousarray(w[k][P + 1:])
    cb = SimpleNamespace(**{**vars(cfg), "model_type": "bert", "max_position_embeddings": 514 - P - 1})
    hb = _hip(cb, wb)
    assert h.position_padding_idx == P and hb.position_padding_idx is None
    for B in (9, 70):
        ids, mask = _tokens(B, S, "R", 100 + S + B, 1000)
        assert np.array_equal(X.fairseq_positions(ids)[mask != 0], (np.arange(S)[None, :] + P + 1).repeat(B, 0)[mask != 0])
        rag, lens = _rag(ids, mask)
        for pool in (0, 1):
            a, b = h.forward_np(ids, mask, pool), hb.forward_np(ids, mask, pool)
            assert np.isfinite(a).all() and _same(a, b), (B, S, pool)
            ar = h.forward_packed(rag, lens, S, pool).cpu().numpy(); br = hb.forward_packed(rag, lens, S, pool).cpu().numpy()
            assert _same(ar, a) and _same(br, a), (B, S, pool)


@pytest.mark.parametrize("B,S", [(1, 32), (5, 300), (9, 96), (64, 40), (65, 64), (300, 33)])
def test_forward_packed_is_bit_identical_to_the_padded_forward_under_the_fairseq_rule(B, S, monkeypatch):
    """Both packers (B <= 64: one launch; B > 64), both attention kernels, P inside sequences, empty sequences under both pools, host / pinned / device input."""
    cfg, w = _small()
    h, m = _hip(cfg, w), X.hf_model(cfg, w)
    rng = np.random.default_rng(B * 977 + S)
    lens = rng.integers(1, S + 1, B).astype(np.int32); lens[0] = S
    if B > 2:
        lens[B // 2] = 0
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    ids = rng.integers(0, 1000, (B, S)); ids[rng.random((B, S)) < 0.05] = P            # P (and id 0) inside attended sequences
    ids = np.where(mask != 0, ids, P)
    rag, lens_t = _rag(ids, mask)
    live = lens > 0
    for pool in (0, 1):
        padded = h.forward_np(ids, mask, pool)
        for src in ((rag, lens_t), (rag.pin_memory(), lens_t.pin_memory()), (rag.cuda(), lens_t.cuda())):
            out = h.forward_packed(src[0], src[1], S, pool)
            h.check()
            assert _same(out.cpu().numpy(), padded), pool
        if S > 128:                                                                   # the register-staged attention kernel on the same input
            monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
            assert _same(h.forward_packed(rag, lens_t, S, pool).cpu().numpy(), padded) and _same(h.forward_np(ids, mask, pool), padded)
            monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
        ref = X.hf_encode(m, ids[live], mask[live], pool)
        assert _cos_gap(padded[live], ref) <= COS_BAR


def test_a_row_does_not_depend_on_its_batch_under_the_fairseq_rule():
    cfg, w = _small()
    h = _hip(cfg, w)
    rng = np.random.default_rng(5)
    for B, S in ((6, 40), (40, 128), (9, 300), (100, 160)):
        ids = rng.integers(0, 1000, (B, S)); mask = np.zeros((B, S), np.int64)
        lens = rng.integers(1, S + 1, B); lens[0] = S
        for b in range(B):
            if b % 4 == 3: mask[b, S - lens[b]:] = 1
            else: mask[b, :lens[b]] = 1
        ids = np.where(mask != 0, ids, P); ids[3, 0] = 9                               # a masked non-P id in front of a left-padded row
        for pool in (0, 1):
            full = h.forward_np(ids, mask, pool)
            for b in (0, 1, 3, B - 1):
                assert _same(h.forward_np(ids[[b]], mask[[b]], pool)[0], full[b]), (B, S, b, pool)
                n = int(mask[b].sum())
                if b % 4 != 3:                                                         # right-padded: the sequence alone, unpadded
                    assert _same(h.forward_np(ids[[b], :n], mask[[b], :n], pool)[0], full[b]), (B, S, b, pool, n)


@pytest.mark.parametrize("heads", [4, 2])
@pytest.mark.parametrize("S", [1024, 2048, 8192])
def test_long_sequences_up_to_8192_tokens(S, heads):
    """A bge-m3-like handle (8194 position rows), tiny 32-wide and 64-wide-head shapes: one full-length row, one right-padded and one left-padded row; mean and
    CLS pooling at the usual bars, the ragged entry point bit-identical, and kr_encoder_last_hidden rows at their columns.
    Measured on MI355X (worst over S = 1024 / 2048 / 8192 and both head widths): mean pooling 1 - cos 6.0e-8, |q.d - ref| 4.8e-7; CLS 1 - cos 1.2e-7,
    |q.d - ref| 9.3e-6 (profiles/xlmr/measurements.txt): no drift with the length."""
    H = 128
    cfg = X.cfg(H, 2, heads, 512, 1000, 8194)
    w = X.weights(H, 2, 512, 1000, 8194, "benign", seed=21)
    h, m = _hip(cfg, w), X.hf_model(cfg, w)
    rng = np.random.default_rng(S + heads)
    ids = rng.integers(5, 1000, (3, S)); mask = np.zeros((3, S), np.int64)
    n1, n2 = S // 2 + 37, S // 3 + 5
    mask[0] = 1; mask[1, :n1] = 1; mask[2, S - n2:] = 1
    ids = np.where(mask != 0, ids, P)
    for pool in (0, 1):
        out, ref = h.forward_np(ids, mask, pool), X.hf_encode(m, ids, mask, pool, chunk=1)
        cos = _cos_gap(out, ref)
        dscore = float(np.abs(out @ out.T - ref @ ref.T).max())
        print(f"[S={S} heads={heads} pool={pool}] 1 - cos {cos:.2e}, |q.d - ref| {dscore:.2e}")
        assert np.isfinite(out).all() and cos <= COS_BAR and dscore <= SCORE_BAR, (S, heads, pool, cos, dscore)
        ids_r = ids[:2]; mask_r = mask[:2]
        rag, lens = _rag(ids_r, mask_r)
        assert _same(h.forward_packed(rag, lens, S, pool).cpu().numpy(), h.forward_np(ids_r, mask_r, pool))
        assert _same(h.forward_np(ids_r, mask_r, pool), out[:2])
    h.forward_np(ids, mask, 0)
    lh = h.last_hidden(3, S).numpy()
    assert not lh[mask == 0].any() and np.abs(lh[mask != 0]).sum(1).min() > 0
    with torch.no_grad():
        for r in range(3):
            ref = m(input_ids=torch.from_numpy(ids[[r]]).cuda(), attention_mask=torch.from_numpy(mask[[r]]).cuda()).last_hidden_state[0].cpu().numpy()
            on = mask[r] != 0
            assert _cos_gap(lh[r][on], ref[on]) <= COS_BAR, r


def _raw_handle(max_pos=514):
    from kirag_amd import _lib
    lib = _lib.load()
    cfg = _lib.BertCfg(128, 1, 4, 512, 100, max_pos, 1, 1e-5)
    h = C.c_void_p()
    _lib.check(lib.kr_encoder_create_ex(C.byref(cfg), 0, -1, -1, C.byref(h)))
    return lib, h


def _set(lib, h, name, *vals):
    a = (C.c_float * len(vals))(*vals)
    return lib.kr_encoder_load_weight(h, name.encode(), C.addressof(a), len(vals))


def test_limits_and_errors():
    from kirag_amd import _lib
    cfg, w = _small(H=128, heads=4)
    h = _hip(cfg, w)
    ids = np.full((2, 513), 7, np.int64); mask = np.ones((2, 513), np.int64)
    for call in (lambda: h.forward_np(ids, mask, 0), lambda: h.forward_packed(torch.full((1026,), 7, dtype=torch.int32), torch.tensor([513, 513], dtype=torch.int32), 513, 0)):
        with pytest.raises(_lib.KiragAmdError) as ei:
            call()
        assert ei.value.code == KR_EINVAL and "513" in str(ei.value) and "514" in str(ei.value)
    assert np.isfinite(h.forward_np(ids[:, :512], mask[:, :512], 0)).all()           # 512 tokens is the limit, not below it
    # token id = vocab: the deferred KR_EINVAL, as under BERT's rule; the handle works on afterwards
    bad = ids[:, :16].copy(); bad[1, 3] = 1000
    with pytest.raises(_lib.KiragAmdError) as ei:
        h.forward_np(bad, mask[:, :16], 0)
    assert ei.value.code == KR_EINVAL and "1000" in str(ei.value)
    good = h.forward_np(ids[:, :16], mask[:, :16], 0)
    assert np.isfinite(good).all()
    # the rule holds for the handle's life: the same value again is a no-op, another one is refused, a weight re-sync keeps it
    assert _set(h._lib, h._h, "config.position_padding_idx", 1.0) == 0
    assert _set(h._lib, h._h, "config.position_padding_idx", 0.0) == KR_EINVAL
    h.load_state(w)
    assert _same(h.forward_np(ids[:, :16], mask[:, :16], 0), good)
    lib, raw = _raw_handle()
    try:
        for v in (1.5, -1.0, 513.0, float("nan")):
            assert _set(lib, raw, "config.position_padding_idx", v) == KR_EINVAL, v
        assert b"512" in lib.kr_last_error() or b"position_padding_idx" in lib.kr_last_error()
        assert _set(lib, raw, "config.position_padding_idx", 1.0, 1.0) == KR_EINVAL      # one value
        assert _set(lib, raw, "config.no_such_setting", 1.0) == KR_EINVAL
        assert _set(lib, raw, "config.position_padding_idx", 512.0) == 0                # max_pos - 2 is the largest
        assert _set(lib, raw, "config.position_padding_idx", 1.0) == 0                  # before the first finalize the value may still change
    finally:
        lib.kr_encoder_destroy(raw)


def test_checkpoint_check_tool_on_an_xlm_roberta_model():
    """tools/checkpoint_check.py on a RoBERTa-family model: the reference is XLMRobertaModel in fp32, the tested path the HIP encoder under fairseq's rule."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(repo, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    cfg = X.cfg(384, 2, 12, 1536, 3000, 514)
    m = X.hf_model(cfg, X.weights(384, 2, 1536, 3000, 514, "out3"))
    out = cc.check_model(m, cc.parse(["(xlm-r, 384 wide)", "--n", "8", "--max-length", "64", "--random-tokens"]))
    assert out["tested_path"] == "hip" and len(out["modes"]) == 4 and all(r["finite"] for r in out["modes"])
    print("checkpoint_check xlm-r out3 (HIP):", out["modes"][0])
    assert out["modes"][0]["worst_score_error"] <= SCORE_BAR and out["modes"][0]["worst_1_minus_cos"] <= COS_BAR


class _Corpus:
    def __init__(self, n, words, rng):
        self.p = ["title:  " + " ".join(rng.choice(words, 2)) + ", text:  " + " ".join(rng.choice(words, int(rng.integers(3, 40)))) for _ in range(n)]
        self.index_to_passage_id = {i: str(2 * i + 5) for i in range(n)}
    def __len__(self): return len(self.p)
    def __getitem__(self, i): return {"index": i, "passage": self.p[i]}
    def get_document(self, docid): return {"id": docid, "text": self.p[(int(docid) - 5) // 2]}


@pytest.mark.parametrize("name,pool", [("E5Retriever", 0), ("BGERetriever", 1)])
def test_reference_entry_points_on_a_saved_xlm_roberta_checkpoint(tmp_path, name, pool):
    """save_pretrained a tiny XLMRobertaModel + a fast tokenizer whose pad id is 1; load_retriever(<existing name>, dir) returns the XLM-R twin;
    cal_doc_embeddings from text -> shard files -> Indexer -> DenseRetriever(queries, topk).  The written rows equal the padded forward bit for bit and the HF
    fp32 embeddings within the bars; the hits are the exact top-k over the written rows.
    Measured on MI355X (written rows vs HF fp32, 1 - cos / |q.d - ref|): E5Retriever 2.4e-7 / 1.0e-5, BGERetriever 1.2e-7 / 8.3e-7."""
    import indep_check as IC
    from kirag_amd import compute_corpus_embeddings as CC
    from kirag_amd import faiss_index_corpus as FI
    from kirag_amd.collators import COLLATOR_MAP
    from kirag_amd.retrieve import setup_retriever_model
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever.retrievers import InBatchRetriever, load_retriever
    from transformers import XLMRobertaConfig, XLMRobertaModel
    words = X.toy_words(400)
    tok = X.toy_tokenizer(words)
    vocab = tok.vocab_size
    H, L, heads, FF = 128, 2, 4, 512
    w = X.weights(H, L, FF, vocab, 514, "out3")
    td = str(tmp_path / "model")
    m = XLMRobertaModel(XLMRobertaConfig(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF,
                                         max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2),
                        add_pooling_layer=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    m.save_pretrained(td)
    tok.save_pretrained(td)
    twin = {"E5Retriever": ENC.XLMRobertaE5Encoder, "BGERetriever": ENC.XLMRobertaBGEEncoder}[name]
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
    assert CC.cal_doc_embeddings.last_feed["packed_forward"]
    assert ret.encoder._hip.position_padding_idx == 1
    folder = os.path.join(str(tmp_path), tag, "c")
    assert len([f for f in os.listdir(folder) if f.startswith("corpus_embeddings_")]) == 3
    FI.build_faiss_index(FI.setup_parser(["--index_folder", folder, "--embedding_size", str(H)]))
    args = SimpleNamespace(retriever_name=name, tokenizer_name_or_path=td, query_maxlength=24, doc_maxlength=48, retriever_model_name_or_path=td, local_rank=-1,
                           corpus="unused", index_folder=folder, embedding_size=H, per_gpu_batch_size=8)
    dr, _ = setup_retriever_model(args, corpus_dataset=corpus, tokenizer=tok)
    assert type(dr.retriever.encoder) is twin
    x = dr.indexer.index.reconstruct_n(0, 1500)
    assert x.shape == (1500, H)
    # the written rows (ragged feed) against the module's padded forward, bit for bit, and against HF fp32 on the collator's own ids
    a = col.encode_doc(corpus.p[:256])
    ids, mask = a["input_ids"].numpy(), a["attention_mask"].numpy()
    assert (ids[mask == 0] == 1).all() and (mask == 0).any()
    padded = dr.retriever.doc({"input_ids": a["input_ids"].cuda(), "attention_mask": a["attention_mask"].cuda()}).cpu().numpy()
    assert _same(padded, np.ascontiguousarray(x[:256]))
    ref = X.hf_encode(m.float().eval().cuda(), ids, mask, pool)
    cos = _cos_gap(x[:256], ref)
    dscore = float(np.abs(x[:256] @ x[:256].T - ref @ ref.T).max())
    print(f"[{name}] written rows vs HF fp32: 1 - cos {cos:.2e}, |q.d - ref| {dscore:.2e}")
    assert cos <= COS_BAR and dscore <= SCORE_BAR
    # one retrieval hop: hits = exact top-k over the written embeddings
    qs = [corpus.p[40].split("text:  ")[1], corpus.p[1499].split("text:  ")[1][:40], " ".join(words[:5])]
    k = 10
    out = dr(qs, topk=k)
    qv = dr.calculate_query_embeddings(qs).numpy()
    qa = col.encode_query(qs)
    assert _cos_gap(qv, X.hf_encode(m, qa["input_ids"].numpy(), qa["attention_mask"].numpy(), pool)) <= COS_BAR
    rs, ri = IC.torch_topk_fp32(torch.from_numpy(qv).cuda(), [(0, torch.from_numpy(x).cuda())], k + 8)
    rows = np.array([[(int(d["id"]) - 5) // 2 for d in out[r]] for r in range(len(qs))])
    s = np.array([[d["score"] for d in out[r]] for r in range(len(qs))], np.float32)
    IC.check_membership(s, rows, rs.cpu().numpy(), ri.cpu().numpy(), k)
    assert all(d["text"] == corpus.p[(int(d["id"]) - 5) // 2] for r in out for d in r)
