"""GPU tests of MultiDeviceIndexer: row shards driven from one process give, bit for bit, what a one-device Indexer fed the same index_data calls
gives (ids, order, score bits, ties included) and what the oracle gives; entry points, formats, streamed builds and the error paths."""
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import search_np as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indep_check as IC  # noqa: E402

pytestmark = pytest.mark.gpu

N, D = 20000, 256
BATCHES = [1, 3000, 777, 5000, 29, 6000, 5193]          # uneven index_data calls (sum N)


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _feed(ix, x, batches, id0=100):
    o = 0
    for m in batches:
        ix.index_data([id0 + 3 * (o + j) for j in range(m)], x[o:o + m])
        o += m
    assert o == len(x)
    return ix


def _pair(x, batches, devices, reserve=None, **kw):
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    one = Indexer(x.shape[1], **kw)
    many = MultiDeviceIndexer(x.shape[1], devices=devices, **kw)
    for ix in (one, many):
        if reserve is not None:
            ix.index.reserve(reserve)
        _feed(ix, x, batches)
    return one, many


def _same(a, b):
    assert len(a) == len(b)
    for (ia, sa), (ib, sb) in zip(a, b):
        assert ia == ib
        assert np.asarray(sa).dtype == np.float32 and np.array_equal(np.asarray(sa).view(np.uint32), np.asarray(sb).view(np.uint32))


def _pending_zero(ix):
    assert ix.index.pending() == [0] * len(ix.index.shards)


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(2024)
    x = _unit(rng, N, D)
    q = _unit(rng, 4096, D)
    q[:2048] = x[rng.integers(0, N, 2048)] + 0.3 * q[:2048]          # half near corpus rows, half random
    return x, np.ascontiguousarray(q, dtype=np.float32)


@pytest.fixture(scope="module")
def reference(corpus):
    from kirag_amd.retriever.index import Indexer
    x, q = corpus
    one = _feed(Indexer(D), x, BATCHES)
    cache = {}

    def get(nq, k):
        if (nq, k) not in cache:
            cache[(nq, k)] = one.search_knn(q[:nq], k)
        return cache[(nq, k)]
    return get


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_bit_equal_to_one_device_indexer(corpus, reference, W):
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    x, q = corpus
    many = _feed(MultiDeviceIndexer(D, devices=[0] * W), x, BATCHES)
    assert many.index.ntotal == N and len(many.index_id_to_db_id) == N
    assert sum(sh.ntotal for sh in many.index.shards) == N
    qd = torch.from_numpy(q).to("cuda:0")
    for nq in (1, 2, 32, 33, 1024, 1030, 4096):
        for k in (1, 10, 100, 1024):
            want = reference(nq, k)
            _same(many.search_knn(q[:nq], k), want)
            _same(many.search_knn(qd[:nq], k), want)
            if nq <= 33 and k <= 100:
                so, io = S.search_canonical(q[:nq], x, k)
                got = many.search_knn(q[:nq], k)
                for r in range(nq):
                    assert got[r][0] == [str(100 + 3 * j) for j in io[r]] and np.array_equal(got[r][1].view(np.uint32), so[r].view(np.uint32))
    _pending_zero(many)


def test_reserved_build_and_ties_across_shards():
    """duplicate rows in different shards (exact ties across a shard boundary), with a reservation as faiss_index_corpus makes it"""
    from kirag_amd.retriever.formats import shard_range
    rng = np.random.default_rng(5)
    base = _unit(rng, 3000, 128)
    x = np.concatenate([base, base[::-1], base[:1000]])           # every row at least twice, the copies far apart
    q = np.ascontiguousarray(np.concatenate([base[[5, 17, 2999]], _unit(rng, 61, 128)]))
    for W in (2, 3):
        one, many = _pair(x, [2000, 4000, 1000], [0] * W, reserve=len(x))
        assert [sh.ntotal for sh in many.index.shards] == [b - a for a, b in (shard_range(len(x), s, W) for s in range(W))]
        for nq, k in ((3, 10), (64, 100), (64, 10)):
            a, b = one.search_knn(q[:nq], k), many.search_knn(q[:nq], k)
            _same(b, a)
            so, io = S.search_canonical(q[:nq], x, k)
            for r in range(nq):
                assert b[r][0] == [str(100 + 3 * j) for j in io[r]]


def test_nan_rows():
    rng = np.random.default_rng(6)
    x = _unit(rng, 5000, 256)
    x[[3, 1700, 2500, 4999]] = np.nan
    q = _unit(rng, 40, 256)
    one, many = _pair(x, [2500, 2500], [0, 0, 0])
    for nq, k in ((1, 10), (40, 100)):
        _same(many.search_knn(q[:nq], k), one.search_knn(q[:nq], k))


def test_shard_below_k_and_empty_shard():
    """batches smaller than the shard count: shards 0 and 1 above k, shard 2 below k, shard 3 empty"""
    rng = np.random.default_rng(7)
    x = _unit(rng, 420, 64)
    one, many = _pair(x, [3] * 100 + [2] * 60, [0] * 4)
    assert [sh.ntotal for sh in many.index.shards] == [160, 160, 100, 0]
    q = _unit(rng, 64, 64)
    for nq, k in ((1, 150), (64, 150), (64, 10), (2, 420), (40, 300)):
        _same(many.search_knn(q[:nq], k), one.search_knn(q[:nq], k))
        so, io = S.search_canonical(q[:nq], x, k)
        got = many.search_knn(q[:nq], k)
        assert [g[0] for g in got] == [[str(100 + 3 * j) for j in r] for r in io]
    _pending_zero(many)


def test_uncertifiable_corpus_falls_back_inside_the_shards():
    rng = np.random.default_rng(11)
    base = _unit(rng, 1, 256)
    x = base + 2e-4 * rng.standard_normal((18000, 256)).astype(np.float32)        # rows closer together than the bf16 error bound
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = _unit(rng, 40, 256) * 0.2 + base
    q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=np.float32)
    one, many = _pair(x, [3000, 15000], [0, 0, 0])
    many.index.stats(reset=True); one.index.stats(reset=True)
    for nq, k in ((2, 50), (40, 50)):
        got = many.search_knn(q[:nq], k)
        _same(got, one.search_knn(q[:nq], k))
        so, io = S.search_canonical(q[:nq], x, k)
        for r in range(nq):
            assert got[r][0] == [str(100 + 3 * j) for j in io[r]] and np.array_equal(got[r][1].view(np.uint32), so[r].view(np.uint32))
    assert many.index.stats()["fallback"] > 0, (many.index.shard_stats(), one.index.stats())
    _pending_zero(many)


def test_byte_path_on_every_shard():
    """d = 1024, two shards of >= 2^19 rows each: small blocks take the int8 pre-scan on every shard; results equal the one-device Indexer and the
    kernel-independent check"""
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    d, n = 1024, (1 << 20) + 4096
    g = torch.Generator(device="cuda:0").manual_seed(3)
    one = Indexer(d, device=0)
    many = MultiDeviceIndexer(d, devices=[0, 0])
    for ix in (one, many):
        ix.index.reserve(n)
    chunks = []
    for s0 in range(0, n, 1 << 18):
        m = min(1 << 18, n - s0)
        xb = torch.randn((m, d), generator=g, device="cuda:0")
        xb = xb / xb.norm(dim=1, keepdim=True)
        for ix in (one, many):
            ix.index_data(list(range(s0, s0 + m)), xb)
        chunks.append((s0, xb))
    assert [sh.ntotal for sh in many.index.shards] == [n // 2, n // 2]
    qd = chunks[1][1][:8] + 0.5 * torch.randn((8, d), generator=g, device="cuda:0")
    qd = (qd / qd.norm(dim=1, keepdim=True)).contiguous()
    many.index.stats(reset=True)
    for nq in (1, 8):
        got = many.search_knn(qd[:nq], 10)
        _same(got, one.search_knn(qd[:nq], 10))
        ref_s, ref_i = IC.torch_topk_fp32(qd[:nq], chunks, 10 + 8)
        s = np.stack([r[1] for r in got]); i = np.stack([[int(v) for v in r[0]] for r in got])
        IC.check_membership(s, i, ref_s.cpu().numpy(), ref_i.cpu().numpy(), 10)
    for st in many.index.shard_stats():
        assert st["byte_scans"] > 0, st
    _pending_zero(many)


def _golden_setup(td, golden):
    from transformers import BertConfig
    from oracle import encoder_np as E
    from kirag_amd.bench_support import wordpiece_tokenizer
    from kirag_amd.retriever.encoders import E5Encoder
    g = golden("g4_g8_retriever.npz")
    H, L, heads, FF, vocab, max_pos = [int(v) for v in g["cfg"]]
    cfg = BertConfig(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF,
                     max_position_embeddings=max_pos)
    m = E5Encoder(cfg, add_pooling_layer=False)
    w = E.synth_weights(H, L, FF, vocab, max_pos, seed=int(g["weight_seed"]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    m.save_pretrained(td)
    with open(os.path.join(td, "vocab.txt"), "w") as f:
        f.write("\n".join(str(v) for v in g["vocab"]) + "\n")
    return g, wordpiece_tokenizer(os.path.join(td, "vocab.txt"))


class _Corpus:
    def __init__(self, words, n, seed):
        rng = np.random.default_rng(seed)
        self.p = ["title:  " + " ".join(rng.choice(words, 2)) + ", text:  " + " ".join(rng.choice(words, int(rng.integers(3, 25)))) for _ in range(n)]
        self.index_to_passage_id = {i: str(7 * i + 1) for i in range(n)}

    def __len__(self): return len(self.p)
    def __getitem__(self, i): return {"index": i, "passage": self.p[i]}
    def get_document(self, docid): return {"id": docid, "text": self.p[(int(docid) - 1) // 7]}


def test_streamed_build_and_setup_retriever_model(golden, tmp_path, monkeypatch):
    """cal_doc_embeddings(..., indexer=MultiDeviceIndexer) equals the same streamed build into an Indexer; setup_retriever_model with
    index_devices=[0, 0] answers DenseRetriever(queries, k) and the one-query hop exactly as with index_devices unset"""
    from kirag_amd import compute_corpus_embeddings as CC
    from kirag_amd import faiss_index_corpus as FI
    from kirag_amd.collators import E5Collator
    from kirag_amd.retrieve import setup_retriever_model
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    from kirag_amd.retriever.retrievers import InBatchRetriever
    monkeypatch.delenv("KIRAG_AMD_INDEX_DEVICES", raising=False)
    with tempfile.TemporaryDirectory() as td:
        g, tok = _golden_setup(td, golden)
        words = [str(v) for v in g["vocab"] if str(v).isalpha() and len(str(v)) > 1]
        corpus = _Corpus(words, 150, 3)
        ret = InBatchRetriever("E5Retriever", td, temperature=0.01)
        col = E5Collator(tokenizer=tok, query_maxlength=16, doc_maxlength=32)
        # streamed build straight into the resident index (no files): three shards vs one device
        built = []
        for ix in (Indexer(ret.hidden_size), MultiDeviceIndexer(ret.hidden_size, devices=[0, 0, 0])):
            a = SimpleNamespace(local_rank=-1, save_dir=str(tmp_path / type(ix).__name__), name="e5", index_folder="c", per_gpu_batch_size=8,
                                num_passage_per_index_file=1000, encode_batch_size=16)
            CC.cal_doc_embeddings(a, ret, corpus, col, indexer=ix)
            built.append(ix)
        one, many = built
        assert many.index.ntotal == one.index.ntotal == 150 and np.array_equal(many.index_id_to_db_id, one.index_id_to_db_id)
        assert np.array_equal(many.index.reconstruct_n(0, 150), one.index.reconstruct_n(0, 150))
        qv = one.index.reconstruct_n(0, 37) * 0.5 + one.index.reconstruct_n(100, 37)
        _same(many.search_knn(qv, 12), one.search_knn(qv, 12))
        # the entry points: faiss_index_corpus over two devices writes the files the one-device build writes
        enc = SimpleNamespace(local_rank=-1, save_dir=str(tmp_path), name="e5", index_folder="c", per_gpu_batch_size=8, num_passage_per_index_file=60,
                              encode_batch_size=64)
        CC.cal_doc_embeddings(enc, ret, corpus, col)
        folder = os.path.join(str(tmp_path), "e5", "c")
        FI.build_faiss_index(SimpleNamespace(index_folder=folder, embedding_size=ret.hidden_size, index_devices="0,0"))
        base = dict(retriever_name="E5Retriever", tokenizer_name_or_path=td, query_maxlength=16, doc_maxlength=32, retriever_model_name_or_path=td,
                    local_rank=-1, corpus="unused", index_folder=folder, embedding_size=ret.hidden_size, per_gpu_batch_size=8)
        dr1, _ = setup_retriever_model(SimpleNamespace(**base), corpus_dataset=corpus, tokenizer=tok)
        drw, _ = setup_retriever_model(SimpleNamespace(index_devices=[0, 0], **base), corpus_dataset=corpus, tokenizer=tok)
        assert type(dr1.indexer) is Indexer and isinstance(drw.indexer, MultiDeviceIndexer) and drw.indexer.devices == [0, 0]
        qs = [corpus.p[40].split("text:  ")[1], "capital of france", corpus.p[3].split("text:  ")[1]] + [corpus.p[i][:40] for i in range(40)]
        for k in (4, 10):
            assert drw(qs, topk=k) == dr1(qs, topk=k)
        assert drw([qs[0]], 10) == dr1([qs[0]], 10)
        assert drw(qs[2], topk=10) == dr1(qs[2], topk=10)
        monkeypatch.setenv("KIRAG_AMD_INDEX_DEVICES", "0,0,0")
        dre, _ = setup_retriever_model(SimpleNamespace(**base), corpus_dataset=corpus, tokenizer=tok)
        assert isinstance(dre.indexer, MultiDeviceIndexer) and dre.indexer.devices == [0, 0, 0]
        assert dre(qs, topk=10) == dr1(qs, topk=10)


def test_format_round_trips(tmp_path):
    from kirag_amd.retriever.formats import SHARD_MANIFEST, _ids_crc32, shard_file_name, shard_range, write_native_shard
    from kirag_amd.retriever.flat_index import FlatIPIndex
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    rng = np.random.default_rng(9)
    x = _unit(rng, 7001, 128)
    q = _unit(rng, 50, 128)
    one, many = _pair(x, [1234, 5000, 767], [0, 0, 0])
    want = one.search_knn(q, 20)
    # MultiDeviceIndexer.serialize -> Indexer.deserialize_from
    d1 = tmp_path / "a"; d1.mkdir()
    many.serialize(str(d1))
    back = Indexer(128); back.deserialize_from(str(d1))
    assert np.array_equal(back.index.reconstruct_n(0, len(x)), x) and np.array_equal(back.index_id_to_db_id, one.index_id_to_db_id)
    _same(back.search_knn(q, 20), want)
    # Indexer.serialize -> MultiDeviceIndexer.deserialize_from
    d2 = tmp_path / "b"; d2.mkdir()
    one.serialize(str(d2))
    m2 = MultiDeviceIndexer(128, devices=[0, 0]); m2.deserialize_from(str(d2))
    assert [sh.ntotal for sh in m2.index.shards] == [3501, 3500]
    _same(m2.search_knn(q, 20), want)
    _same(m2.search_knn(q[:1], 20), want[:1])
    # native shards written for world 2 -> three shards
    d3 = tmp_path / "c"; d3.mkdir()
    ids = one.index_id_to_db_id
    info = []
    for r in range(2):
        a, b = shard_range(len(x), r, 2)
        sh = FlatIPIndex(128, device=0); sh.add(x[a:b])
        write_native_shard(sh, str(d3 / shard_file_name(r, 2)), a, len(x))
        info.append({"rank": r, "row0": a, "rows": b - a, "file": shard_file_name(r, 2)})
    with open(d3 / SHARD_MANIFEST, "w") as f:
        json.dump({"format": "krshard-1", "meta_crc32": _ids_crc32(ids), "d": 128, "coarse_dim": sh.coarse_dim, "coarse_dtype": "bf16",
                   "ntotal": len(x), "world": 2, "shards": info}, f)
    import pickle
    with open(d3 / "index_meta.faiss", "wb") as f:
        pickle.dump(ids, f)
    m3 = MultiDeviceIndexer(128, devices=[0, 0, 0]); m3.deserialize_from(str(d3))
    assert [sh.ntotal for sh in m3.index.shards] == [2334, 2334, 2333]
    _same(m3.search_knn(q, 20), want)
    # rows appended after a reload go on in global order
    extra = _unit(rng, 10, 128)
    m3.index_data(list(range(9000, 9010)), extra); one.index_data(list(range(9000, 9010)), extra)
    _same(m3.search_knn(q, 30), one.search_knn(q, 30))


def test_errors_leave_nothing_pending():
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    rng = np.random.default_rng(1)
    x = _unit(rng, 3000, 64)
    q = _unit(rng, 3000, 64)
    many = _feed(MultiDeviceIndexer(64, devices=[0, 0, 0]), x, [1000, 2000])
    for nq in (1, 40, 3000):
        with pytest.raises(ValueError):
            many.search_knn(q[:nq], 3001)
        _pending_zero(many)
        with pytest.raises(ValueError):
            many.search_knn(q[:nq], 1025)
        _pending_zero(many)
        with pytest.raises(ValueError):
            many.search_knn(q[:nq], 0)
        _pending_zero(many)
    with pytest.raises(NotImplementedError):
        MultiDeviceIndexer(64, metric="l2", devices=[0, 0])
    with pytest.raises(NotImplementedError):
        MultiDeviceIndexer(64, n_subquantizers=8, devices=[0, 0])
    assert len(many.search_knn(q[:5], 10)) == 5                      # still usable
    _pending_zero(many)


def test_faiss_padding():
    from kirag_amd.retriever.index import Indexer
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    rng = np.random.default_rng(4)
    x = _unit(rng, 30, 32)
    q = _unit(rng, 3, 32)
    one = _feed(Indexer(32, faiss_padding=True), x, [10, 20])
    many = _feed(MultiDeviceIndexer(32, devices=[0, 0, 0], faiss_padding=True), x, [10, 20])
    _same(many.search_knn(q, 40), one.search_knn(q, 40))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_devices_queries_on_cuda1(corpus, reference):
    from kirag_amd.retriever.multi_device import MultiDeviceIndexer
    x, q = corpus
    many = _feed(MultiDeviceIndexer(D, devices=[0, 1, 1, 0]), x, BATCHES)
    qd = torch.from_numpy(q).to("cuda:1")
    for nq, k in ((1, 10), (33, 100), (1030, 100)):
        _same(many.search_knn(qd[:nq], k), reference(nq, k))
        _same(many.search_knn(q[:nq], k), reference(nq, k))
    _pending_zero(many)
