"""GPU tests of BERT checkpoints with 32-wide attention heads (e5-small-v2, bge-small-en-v1.5, gte-small, all-MiniLM-L6/L12: hidden 384, 12 heads of 32):
parity with HF BertModel in fp32, the bit-identity properties the embedding cache relies on (both attention kernels, every projection path, the packed
forward, batch composition, the CLS-rows-only last layer), and the reference's corpus-encode -> index -> retrieve entry points at 384 wide."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import encoder_np as E

pytestmark = pytest.mark.gpu

SHAPES = {                          # (H, L, heads, FF)
    "e5-small": (384, 12, 12, 1536),
    "minilm-l6": (384, 6, 12, 1536),
    "tiny": (128, 2, 4, 512),
}
VOCAB, MAX_POS = 30522, 512


def _cfg(H, L, heads, FF, vocab=VOCAB, max_pos=MAX_POS):
    return SimpleNamespace(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=vocab,
                           max_position_embeddings=max_pos, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")


def _weights(shape, wname):
    H, L, heads, FF = SHAPES[shape]
    if wname == "benign":
        return E.synth_weights(H, L, FF, VOCAB, MAX_POS, seed=3)
    return E.synth_weights_outlier(H, L, FF, VOCAB, MAX_POS, seed=7, gamma_lo=1.5, gamma_hi=3.0)    # out3 (tests/golden/g10_spec.py)


def _hip(cfg, w):
    from kirag_amd.retriever.encoders import HipBertForward
    h = HipBertForward(cfg, 0)
    h.load_state(w)
    return h


def _hf(cfg, w):
    from transformers import BertConfig, BertModel
    m = BertModel(BertConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                             intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size, max_position_embeddings=cfg.max_position_embeddings,
                             type_vocab_size=2, layer_norm_eps=1e-12), add_pooling_layer=False)
    assert not m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False).missing_keys
    return m.float().eval().cuda()


@torch.no_grad()
def _hf_encode(m, ids, mask, pool, chunk=16):
    """E5Encoder (masked mean) / BGEEncoder (CLS) on HF's fp32 last_hidden_state, L2-normalised (encoders.py:56-58, 67-77, 106-118)"""
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(ids[i:i + chunk]).cuda(); k = torch.from_numpy(mask[i:i + chunk]).cuda()
        lh = m(input_ids=a, attention_mask=k).last_hidden_state
        if pool == 0:
            lh = lh.masked_fill(~k[..., None].bool(), 0.0)
            v = lh.sum(1) / k.sum(1)[..., None]
        else:
            v = lh[:, 0]
        outs.append(torch.nn.functional.normalize(v, dim=-1).cpu().numpy())
    return np.concatenate(outs)


def _tokens(B, S, layout, seed, vocab_hi=30000):
    ids, mask = E.synth_tokens(B, S, seed=seed, ragged=layout != "F", vocab_hi=vocab_hi)
    if layout == "L":
        ids = np.ascontiguousarray(ids[:, ::-1]); mask = np.ascontiguousarray(mask[:, ::-1])
    return ids, mask


# (B, S, layout, seed): R = ragged right-padded, L = ragged left-padded, F = full length
CASES = {"e5": [(64, 128, "R", 1), (16, 32, "R", 2), (2, 512, "R", 3), (4, 256, "L", 4), (8, 128, "F", 5), (32, 32, "F", 6)],
         "bge": [(8, 128, "R", 7), (4, 256, "L", 8), (2, 512, "F", 9), (16, 32, "L", 10)]}


@pytest.mark.parametrize("shape", ["e5-small", "minilm-l6", "tiny"])
@pytest.mark.parametrize("wname", ["benign", "out3"])
def test_parity_with_hf_bert_fp32(shape, wname):
    """The default mode (f16 operands + residual low half) against HF BertModel in fp32 with the encoders' pooling, at G10's bars: every query x passage
    score within 1e-3 of the fp32 scores, 1 - cos <= 5e-5.
    Measured on MI355X (worst |q.d - ref| / worst 1 - cos): e5-small benign 8.6e-6 / 1.2e-7, out3 3.6e-5 / 1.8e-7; minilm-l6 benign 6.6e-6 / 1.2e-7,
    out3 1.7e-5 / 1.8e-7; tiny benign 1.7e-6 / 1.2e-7, out3 9.4e-6 / 1.2e-7."""
    H, L, heads, FF = SHAPES[shape]
    cfg = _cfg(H, L, heads, FF)
    w = _weights(shape, wname)
    h, m = _hip(cfg, w), _hf(cfg, w)
    outs, refs = {}, {}
    worst_cos = 0.0
    for tag, pool in (("e5", 0), ("bge", 1)):
        for B, S, layout, seed in CASES[tag]:
            ids, mask = _tokens(B, S, layout, seed)
            out, ref = h.forward_np(ids, mask, pool), _hf_encode(m, ids, mask, pool)
            assert out.shape == ref.shape and np.isfinite(out).all()
            cos = float((1 - (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))).max())
            worst_cos = max(worst_cos, cos)
            assert cos <= 5e-5, (tag, B, S, layout, cos)
            outs[(tag, B, S, layout)] = out; refs[(tag, B, S, layout)] = ref
    worst = 0.0
    for a in outs:
        for b in outs:
            if a[0] == b[0] == "e5":
                worst = max(worst, float(np.abs(outs[a] @ outs[b].T - refs[a] @ refs[b].T).max()))
    print(f"[{shape} {wname}] worst |q.d - ref| {worst:.2e}, worst 1 - cos {worst_cos:.2e}")
    assert worst <= 1e-3, worst


def _small(L=2):
    cfg = _cfg(384, L, 12, 1536, vocab=1000)
    return cfg, E.synth_weights(384, L, 1536, 1000, MAX_POS, seed=11)


def _ragged(rng, B, S, left_every=4):
    ids = rng.integers(5, 1000, (B, S)); mask = np.zeros((B, S), np.int64)
    lens = rng.integers(1, S + 1, B); lens[0] = S
    for b in range(B):
        if b % left_every == left_every - 1: mask[b, S - lens[b]:] = 1
        else: mask[b, :lens[b]] = 1
    return ids, mask


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_both_attention_kernels_give_the_same_bits(monkeypatch):
    """Head width 32: the register-staged kernel (short batches, or forced by KIRAG_AMD_ATTN_LDS=1) and the LDS-DMA ring kernel give the same bits."""
    cfg, w = _small()
    h = _hip(cfg, w)
    rng = np.random.default_rng(7)
    B = 24
    ids = rng.integers(5, 1000, (B, 100)); mask = np.zeros((B, 100), np.int64)
    lens = rng.integers(1, 101, B); lens[0] = 100; lens[1] = 64; lens[2] = 65; lens[3] = 32; lens[4] = 33
    for b in range(B):
        mask[b, :lens[b]] = 1
    wide_ids = np.concatenate([ids, np.zeros((B, 100), np.int64)], 1); wide_mask = np.concatenate([mask, np.zeros((B, 100), np.int64)], 1)
    for pool in (0, 1):
        assert _same(h.forward_np(ids, mask, pool), h.forward_np(wide_ids, wide_mask, pool)), pool
    for S in (129, 200, 300, 512):
        ids = rng.integers(5, 1000, (9, S)); mask = np.zeros((9, S), np.int64)
        lens = rng.integers(1, S + 1, 9); lens[0] = S; lens[1] = 128; lens[2] = 129; lens[3] = 64
        for b in range(9):
            if b % 4 == 3: mask[b, S - lens[b]:] = 1
            else: mask[b, :lens[b]] = 1
        a = h.forward_np(ids, mask, 0)
        monkeypatch.setenv("KIRAG_AMD_ATTN_LDS", "1")
        b_ = h.forward_np(ids, mask, 0)
        monkeypatch.delenv("KIRAG_AMD_ATTN_LDS")
        assert _same(a, b_), S
        ref = E.e5_encode(w, ids, mask, 12)
        assert np.abs(a - ref).max() <= 4e-3, S


def test_projection_paths_are_bit_identical(monkeypatch):
    """H = 384 (K = 384 / 1536, N = 384 / 1152 / 1536): the 256x256, both 128x128 and both skinny loops agree bit for bit, mean and CLS pooling."""
    cfg, w = _small()
    h = _hip(cfg, w)
    ids, mask = E.synth_tokens(700, 48, seed=3, ragged=True, vocab_lo=5, vocab_hi=1000, min_len=3)
    ids2, mask2 = E.synth_tokens(5, 200, seed=4, ragged=True, vocab_lo=5, vocab_hi=1000, min_len=3)
    outs = {}
    for tile in ("256", "128", "130", "32", "64"):
        monkeypatch.setenv("KIRAG_AMD_PROJ_TILE", tile)
        outs[tile] = (h.forward_np(ids, mask, 0), h.forward_np(ids, mask, 1), h.forward_np(ids2, mask2, 0))
    monkeypatch.delenv("KIRAG_AMD_PROJ_TILE")
    for tile in outs:
        for i in range(3):
            assert _same(outs[tile][i], outs["256"][i]), (tile, i)
    assert _same(h.forward_np(ids, mask, 0), outs["256"][0])          # the launcher's own choice is one of them
    assert np.abs(outs["256"][0] - E.e5_encode(w, ids, mask, 12)).max() <= 4e-3


@pytest.mark.parametrize("B,S", [(1, 32), (5, 300), (9, 96), (64, 40), (65, 64), (300, 33), (513, 128)])
def test_forward_packed_is_bit_identical_to_the_padded_forward(B, S):
    cfg, w = _small()
    h = _hip(cfg, w)
    rng = np.random.default_rng(B * 977 + S)
    lens = rng.integers(1, S + 1, B).astype(np.int32); lens[0] = S
    if B > 2:
        lens[B // 2] = 0
    ids = rng.integers(5, 1000, (B, S)); mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    ids = ids * mask
    rag = np.ascontiguousarray(ids[mask != 0].astype(np.int32))
    for pool, fn in ((0, E.e5_encode), (1, E.bge_encode)):
        padded = h.forward_np(ids, mask, pool)
        out = h.forward_packed(torch.from_numpy(rag), torch.from_numpy(lens), S, pool).cpu().numpy()
        assert _same(out, padded), pool
        dev = h.forward_packed(torch.from_numpy(rag).cuda(), torch.from_numpy(lens).cuda(), S, pool)
        h.check()
        assert _same(dev.cpu().numpy(), padded), pool
        live = lens > 0
        assert np.abs(out[live] - fn(w, ids, mask, 12)[live]).max() <= 4e-3


def test_a_sequence_alone_equals_the_same_sequence_in_a_batch():
    """A row alone (same padding, and right-padded rows also trimmed to their length, which may select the other attention kernel) gives the bits it has
    inside a batch of other sequences."""
    cfg, w = _small()
    h = _hip(cfg, w)
    rng = np.random.default_rng(5)
    for B, S in ((6, 40), (40, 128), (9, 300), (100, 160)):
        ids, mask = _ragged(rng, B, S)
        for pool in (0, 1):
            full = h.forward_np(ids, mask, pool)
            for b in (0, 1, 3, B - 1):
                assert _same(h.forward_np(ids[[b]], mask[[b]], pool)[0], full[b]), (B, S, b, pool)
                n = int(mask[b].sum())
                if b % 4 != 3 and n > 0:                                                # right-padded: the sequence alone, unpadded
                    assert _same(h.forward_np(ids[[b], :n], mask[[b], :n], pool)[0], full[b]), (B, S, b, pool, n)


def test_cls_rows_only_last_layer_is_bit_identical(monkeypatch):
    cfg, w = _small()
    rng = np.random.default_rng(3)
    h_short = _hip(cfg, w)
    monkeypatch.setenv("KIRAG_AMD_CLS_FULL", "1")
    h_full = _hip(cfg, w)
    monkeypatch.delenv("KIRAG_AMD_CLS_FULL")
    for B, S in ((6, 40), (3, 200), (300, 33), (70, 64)):
        ids, mask = _ragged(rng, B, S, left_every=3)
        mask[2, 2:5] = 0
        a, b = h_short.forward_np(ids, mask, 1), h_full.forward_np(ids, mask, 1)
        assert _same(a, b), (B, S)
        ref = E.bge_encode(w, ids, mask, 12)
        ok = ~np.isnan(ref).any(1)
        assert np.abs(a[ok] - ref[ok]).max() <= 4e-3


def test_reference_entry_points_end_to_end_at_384_wide(golden, tmp_path):
    """save_pretrained a 384-wide, 12-head E5 model + a WordPiece tokenizer; compute_corpus_embeddings on 3000 passages -> .pkl shards;
    faiss_index_corpus --embedding_size 384; setup_retriever_model + one DenseRetriever hop.  Embeddings within the G10 bars of HF fp32, hits equal
    an exact top-k over the written embeddings."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import indep_check as IC
    from kirag_amd import compute_corpus_embeddings as CC
    from kirag_amd import faiss_index_corpus as FI
    from kirag_amd.bench_support import wordpiece_tokenizer
    from kirag_amd.collators import E5Collator
    from kirag_amd.retrieve import setup_retriever_model
    from kirag_amd.retriever.encoders import E5Encoder
    from kirag_amd.retriever.retrievers import InBatchRetriever
    from transformers import BertConfig
    g = golden("g4_g8_retriever.npz")
    vocab = [str(v) for v in g["vocab"]]
    td = str(tmp_path / "model")
    os.makedirs(td)
    hf_cfg = BertConfig(vocab_size=len(vocab), hidden_size=384, num_hidden_layers=4, num_attention_heads=12, intermediate_size=1536, max_position_embeddings=512)
    w = E.synth_weights_outlier(384, 4, 1536, len(vocab), 512, seed=7, gamma_lo=1.5, gamma_hi=3.0)
    m = E5Encoder(hf_cfg, add_pooling_layer=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    m.save_pretrained(td)
    with open(os.path.join(td, "vocab.txt"), "w") as f:
        f.write("\n".join(vocab) + "\n")
    tok = wordpiece_tokenizer(os.path.join(td, "vocab.txt"))
    rng = np.random.default_rng(9)
    words = [v for v in vocab if v.isalpha() and len(v) > 1]

    class Corpus:
        def __init__(self, n):
            self.p = ["title:  " + " ".join(rng.choice(words, 2)) + ", text:  " + " ".join(rng.choice(words, int(rng.integers(3, 60)))) for _ in range(n)]
            self.index_to_passage_id = {i: str(2 * i + 5) for i in range(n)}
        def __len__(self): return len(self.p)
        def __getitem__(self, i): return {"index": i, "passage": self.p[i]}
        def get_document(self, docid): return {"id": docid, "text": self.p[(int(docid) - 5) // 2]}
    corpus = Corpus(3000)
    enc_args = CC.setup_parser(["--retriever_name", "E5Retriever", "--retriever_model_name_or_path", td, "--tokenizer_name_or_path", td,
                                "--save_dir", str(tmp_path), "--name", "e5small", "--index_folder", "c", "--doc_maxlength", "64",
                                "--per_gpu_batch_size", "8", "--num_passage_per_index_file", "1000", "--encode_batch_size", "256", "--tokenizer_workers", "0"])
    ret = InBatchRetriever("E5Retriever", td, temperature=0.01)
    assert ret.hidden_size == 384
    col = E5Collator(tokenizer=tok, query_maxlength=16, doc_maxlength=64)
    CC.cal_doc_embeddings(enc_args, ret, corpus, col)
    folder = os.path.join(str(tmp_path), "e5small", "c")
    assert len([f for f in os.listdir(folder) if f.startswith("corpus_embeddings_")]) == 3
    FI.build_faiss_index(FI.setup_parser(["--index_folder", folder, "--embedding_size", "384"]))
    args = SimpleNamespace(retriever_name="E5Retriever", tokenizer_name_or_path=td, query_maxlength=16, doc_maxlength=64,
                           retriever_model_name_or_path=td, local_rank=-1, corpus="unused", index_folder=folder, embedding_size=384, per_gpu_batch_size=8)
    dr, _ = setup_retriever_model(args, corpus_dataset=corpus, tokenizer=tok)
    x = dr.indexer.index.reconstruct_n(0, 3000)
    assert x.shape == (3000, 384)
    # the written embeddings against HF fp32 on the collator's own ids
    hf = _hf(_cfg(384, 4, 12, 1536, vocab=len(vocab)), w)
    a = col.encode_doc(corpus.p[:128])
    ref = _hf_encode(hf, a["input_ids"].numpy(), a["attention_mask"].numpy(), 0)
    cos = 1 - (x[:128] * ref).sum(1) / (np.linalg.norm(x[:128], axis=1) * np.linalg.norm(ref, axis=1))
    assert cos.max() <= 5e-5 and np.abs(x[:128] @ x[:128].T - ref @ ref.T).max() <= 1e-3, (float(cos.max()))
    # one retrieval hop: hits = exact top-k over the written embeddings
    qs = [corpus.p[40].split("text:  ")[1], corpus.p[2999].split("text:  ")[1][:40], " ".join(words[:5])]
    k = 10
    out = dr(qs, topk=k)
    qv = dr.calculate_query_embeddings(qs).numpy()
    rs, ri = IC.torch_topk_fp32(torch.from_numpy(qv).cuda(), [(0, torch.from_numpy(x).cuda())], k + 8)
    rows = np.array([[(int(d["id"]) - 5) // 2 for d in out[r]] for r in range(len(qs))])
    s = np.array([[d["score"] for d in out[r]] for r in range(len(qs))], np.float32)
    IC.check_membership(s, rows, rs.cpu().numpy(), ri.cpu().numpy(), k)
    assert all(d["text"] == corpus.p[(int(d["id"]) - 5) // 2] for r in out for d in r)
