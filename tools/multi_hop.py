#!/usr/bin/env python3
"""One KiRAG hop and one large block over W row shards driven from ONE process (``MultiDeviceIndexer``) next to one ``Indexer`` over the same rows:
  * the one-query top-10 hop through ``search_knn`` and through ``DenseRetriever([q], 10)`` (tokenizer, E5 encoder, search, parsing);
  * a 1000-query top-100 ``search_knn``.
Medians of repeated calls; the W-shard results are checked equal to the one-device ones; per-shard ``stats()`` show which path each shard took
(``byte_scans``: the int8 pre-scan of small blocks).
Usage: python tools/multi_hop.py [--rows 5000000] [--shards 1,2,8] [--devices 0] [--reps 50]
  --devices 0      every shard on GPU 0 (W shards: [0] * W);  --devices 0,1,...  shard s on devices[s % len(devices)]"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from kirag_amd.retriever.index import Indexer  # noqa: E402
from kirag_amd.retriever.multi_device import MultiDeviceIndexer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=5_000_000)
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--shards", default="1,2,8")
ap.add_argument("--devices", default="0")
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
N, D = args.rows, args.dim
devs = [int(v) for v in args.devices.split(",")]
dev0 = torch.device("cuda", devs[0])
CHUNK = 250_000


def fill(ix):
    """the same N rows (seeded on the device) into any indexer, in CHUNK-row index_data calls after one reservation"""
    g = torch.Generator(device=dev0); g.manual_seed(3)
    ix.index.reserve(N)
    for s0 in range(0, N, CHUNK):
        m = min(CHUNK, N - s0)
        ix.index_data(np.arange(s0, s0 + m, dtype=np.int64) * 3 + 1_000_000, torch.nn.functional.normalize(torch.randn(m, D, generator=g, device=dev0), dim=1))
    torch.cuda.synchronize(dev0)
    return ix


def med(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.percentile(ts, 90))


# the retriever surface: tokenizer + collator + an E5-large-shaped encoder (random weights) on dev0, as tools/hop_surface.py
from transformers import BertConfig  # noqa: E402
from kirag_amd.bench_support import synthetic_text_corpus, wordpiece_tokenizer  # noqa: E402
from kirag_amd.collators import E5Collator  # noqa: E402
from kirag_amd.retriever.encoders import E5Encoder  # noqa: E402
from kirag_amd.retriever.retrievers import BaseRetriever, DenseRetriever  # noqa: E402

td = tempfile.mkdtemp()
vocab_file, _ = synthetic_text_corpus(8, td, seed=5)
tok = wordpiece_tokenizer(vocab_file)
words = np.array([ln.strip() for ln in open(vocab_file) if ln.strip().isalpha()])
cfg = BertConfig(vocab_size=30522, hidden_size=D, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4 * D, max_position_embeddings=512)
enc = E5Encoder(cfg, add_pooling_layer=False).to(dev0).eval()


class Ret(BaseRetriever):
    def __init__(self, encoder):
        nn.Module.__init__(self)
        self.encoder = encoder
        self.norm_query = self.norm_doc = False
        self.temperature, self.local_rank, self.world_size = 1.0, -1, 1


col = E5Collator(tokenizer=tok, query_maxlength=256, doc_maxlength=128)
rng = np.random.default_rng(0)
query = "which " + " ".join(rng.choice(words, 12)) + " ?\nknowledge triples: " + ". ".join("<" + " ".join(rng.choice(words, 9)) + ">" for _ in range(16))
gq = torch.Generator(device=dev0); gq.manual_seed(11)
q1 = torch.nn.functional.normalize(torch.randn(1, D, generator=gq, device=dev0), dim=1).cpu().numpy()
q1000 = torch.nn.functional.normalize(torch.randn(1000, D, generator=gq, device=dev0), dim=1).cpu().numpy()


def measure(ix, label):
    dr = DenseRetriever(retriever=Ret(enc), collator=col, indexer=ix, corpus=None, batch_size=4)
    hop, hop90 = med(lambda: ix.search_knn(q1, 10), args.reps)
    surf, surf90 = med(lambda: dr([query], 10), args.reps)
    big, big90 = med(lambda: ix.search_knn(q1000, 100), max(5, args.reps // 10))
    print(f"{label:>28}  hop search_knn(1, 10) {hop:7.3f} ms (p90 {hop90:.3f})   DenseRetriever([q], 10) {surf:7.3f} ms (p90 {surf90:.3f})   "
          f"search_knn(1000, 100) {big:8.2f} ms (p90 {big90:.2f})", flush=True)
    return dr


print(f"rows {N} x {D}, devices {devs}, medians of {args.reps} calls (large block: {max(5, args.reps // 10)})", flush=True)
one = fill(Indexer(D, device=devs[0]))
dr1 = measure(one, "Indexer (one device)")
want = (one.search_knn(q1, 10), one.search_knn(q1000, 100), dr1([query], 10))
for W in [int(v) for v in args.shards.split(",")]:
    ix = fill(MultiDeviceIndexer(D, devices=[devs[s % len(devs)] for s in range(W)]))
    ix.index.stats(reset=True)
    drw = measure(ix, f"MultiDeviceIndexer W={W}")
    got = (ix.search_knn(q1, 10), ix.search_knn(q1000, 100), drw([query], 10))
    same = all(a[0] == b[0] and np.array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32)) for a, b in zip(got[0] + got[1], want[0] + want[1]))
    print(f"{'':>28}  results equal to the one-device Indexer: {same and got[2] == want[2]}")
    for s, st in enumerate(ix.index.shard_stats()):
        print(f"{'':>28}  shard {s} (device {ix.index.devices[s]}): rows {ix.index.shards[s].ntotal}  queries {st['queries']}  byte_scans {st['byte_scans']}  "
              f"byte_rows {st['byte_rows']}  fallback {st['fallback']}  reranked_rows {st['reranked_rows']}")
    del ix, drw
    torch.cuda.empty_cache()
