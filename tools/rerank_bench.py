#!/usr/bin/env python3
"""What the classification head costs: KR_POOL_CLASSIFY against KR_POOL_CLS on ONE handle with a head (synthetic weights), alternated in one process.

    python tools/rerank_bench.py [--shape xlmr-large|modernbert-base|deberta-v3-base|qwen2-0.5b] [--pooling cls|mean] [--batches 100x256,1000x128,1x64] [--rounds 6] [--labels 1] [--once] [--digest]

The two forwards differ behind the last LayerNorm only (k_pool's raw rows + k_cls_head instead of the normalising k_pool), so the difference of the medians is
the head.  --once runs one classify forward per batch shape and nothing else: the run to put under a kernel trace (the k_cls_head row is the head's launch).
--shape modernbert-base (22 layers, H 768, 12 heads of 64, FF 1152, vocab 50368): ModernBertForSequenceClassification's head, dense -> gelu -> LayerNorm ->
classifier; --pooling mean makes it read the masked mean, and the plain pool it is compared with is then KR_POOL_MEAN.
--shape deberta-v3-base (12 layers, H 768, 12 heads of 64, FF 3072, 256 buckets): DebertaV2ForSequenceClassification's head under the library's classifier.* names,
dense -> gelu -> classifier.  --digest appends the first 16 hex digits of the sha256 of the classify logits (to compare two builds of the library, each in
its own process under KIRAG_AMD_LIB).
--shape qwen2-0.5b (24 layers, H 896, 14 heads of 64 over 2 KV heads, FF 4864; llama-1b likewise): a decoder handle with the score head ("score.weight", no
bias) read at the last attended token; the plain pool it is compared with is KR_POOL_LAST, which keeps every row of the last layer while the classify
forward finishes it on the B last rows.  A second handle created under KIRAG_AMD_CLS_FULL=1 then gives the shortcut's own A/B: classify on both handles in
turns, logits compared bit for bit (k_score_head is the head's launch in a kernel trace)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from kirag_amd import bench_support as BS
from kirag_amd.retriever.encoders import POOL_CLASSIFY, POOL_CLS, POOL_LAST, POOL_MEAN, HipBertForward

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="xlmr-large")
ap.add_argument("--batches", default="100x256,1000x128,1x64")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--labels", type=int, default=1)
ap.add_argument("--once", action="store_true")
ap.add_argument("--digest", action="store_true")
ap.add_argument("--pooling", default="cls", choices=["cls", "mean"])
args = ap.parse_args()
sys.argv = sys.argv[:1]
import enc_bench as EB  # noqa: E402  (its shape table)

dev = torch.device("cuda:0")
cfg = EB.SHAPES[args.shape]
modern = cfg.get("model_type", "bert") == "modernbert"
deberta = cfg.get("model_type", "bert") == "deberta-v2"
decoder = cfg.get("model_type", "bert") in ("qwen2", "llama", "mistral")
assert modern or deberta or decoder or cfg.get("model_type", "bert") in ("bert", "xlm-roberta", "roberta", "camembert"), "the heads run on BERT / RoBERTa, DeBERTa, ModernBert and decoder handles"
assert modern or args.pooling == "cls", "--pooling mean is ModernBERT's"
H = cfg["hidden_size"]
g = torch.Generator(device=dev); g.manual_seed(31)
randn = lambda *s: torch.randn(*s, generator=g, device=dev)
PLAIN = POOL_LAST if decoder else POOL_MEAN if args.pooling == "mean" else POOL_CLS
PLAIN_NAME = "last" if decoder else args.pooling
enc_full = None
if decoder:
    head = {"score.weight": 4 * randn(args.labels, H) / H ** 0.5}
    enc = EB.make_encoder(cfg, extra_state=head)
    if not args.once:       # the same weights on a handle whose last layer runs on every row
        os.environ["KIRAG_AMD_CLS_FULL"] = "1"
        enc_full = EB.make_encoder(cfg, extra_state=head)
        del os.environ["KIRAG_AMD_CLS_FULL"]
elif modern:
    head = {"head.dense.weight": randn(H, H) / H ** 0.5, "head.norm.weight": 1 + 0.5 * randn(H), "classifier.weight": 4 * randn(args.labels, H) / H ** 0.5,
            "classifier.bias": randn(args.labels), "config.classifier_pooling": torch.tensor([float(args.pooling == "mean")])}
    enc = EB.make_encoder(cfg, extra_state=head)
elif deberta:
    head = {"classifier.dense.weight": randn(H, H) / H ** 0.5, "classifier.dense.bias": 0.5 * randn(H), "classifier.out_proj.weight": 4 * randn(args.labels, H) / H ** 0.5,
            "classifier.out_proj.bias": randn(args.labels)}
    enc = EB.make_encoder(cfg, extra_state=head)
else:
    ns = BS.SimpleNamespace(**cfg)
    state = dict(BS.synthetic_state(ns, dev, 0))
    state.update({"classifier.dense.weight": randn(H, H) / H ** 0.5, "classifier.dense.bias": 0.5 * randn(H),
                  "classifier.out_proj.weight": 4 * randn(args.labels, H) / H ** 0.5, "classifier.out_proj.bias": randn(args.labels)})
    enc = HipBertForward(ns, 0)
    enc.load_state(state)
for B, S in (tuple(int(v) for v in t.split("x")) for t in args.batches.split(",")):
    ids, mask = BS.synthetic_tokens(dev, B, S, seed=1)
    if "pad_token_id" in cfg:
        ids = torch.where(mask != 0, ids, torch.full_like(ids, cfg["pad_token_id"]))
    if args.once:
        enc.forward(ids, mask, POOL_CLASSIFY); torch.cuda.synchronize()
        print(f"{args.shape} {B} x {S}: one classify forward", flush=True)
        continue
    res = {POOL_CLASSIFY: [], PLAIN: []}
    reps = 5 if B * S > 20000 else 20
    for rnd in range(args.rounds):
        for pool in (POOL_CLASSIFY, PLAIN):
            for _ in range(2):
                enc.forward(ids, mask, pool)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps):
                enc.forward(ids, mask, pool)
            torch.cuda.synchronize()
            res[pool].append((time.perf_counter() - t0) / reps * 1e3)
    c, e = np.array(res[POOL_CLASSIFY]), np.array(res[PLAIN])
    print(f"{args.shape} {B} x {S} labels={args.labels}: classify median {np.median(c):.3f} ms (min {c.min():.3f}, max {c.max():.3f})  {PLAIN_NAME} median {np.median(e):.3f} ms "
          f"(min {e.min():.3f}, max {e.max():.3f})  difference of medians {1e3 * (np.median(c) - np.median(e)):+.1f} us"
          + (f"  sha256 {EB.digest(enc.forward(ids, mask, POOL_CLASSIFY))}" if args.digest else ""), flush=True)
    if enc_full is not None:
        same = torch.equal(enc.forward(ids, mask, POOL_CLASSIFY).view(torch.int32), enc_full.forward(ids, mask, POOL_CLASSIFY).view(torch.int32))
        res = {0: [], 1: []}
        for rnd in range(args.rounds):
            for which, handle in enumerate((enc, enc_full)):
                for _ in range(2):
                    handle.forward(ids, mask, POOL_CLASSIFY)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(reps):
                    handle.forward(ids, mask, POOL_CLASSIFY)
                torch.cuda.synchronize()
                res[which].append((time.perf_counter() - t0) / reps * 1e3)
        a, f = np.array(res[0]), np.array(res[1])
        print(f"{args.shape} {B} x {S} labels={args.labels}: last-row shortcut median {np.median(a):.3f} ms (min {a.min():.3f}, max {a.max():.3f})  KIRAG_AMD_CLS_FULL=1 median "
              f"{np.median(f):.3f} ms (min {f.min():.3f}, max {f.max():.3f})  shortcut {100 * (np.median(a) / np.median(f) - 1):+.2f} %  logits bit-identical: {same}", flush=True)
enc.check()
if enc_full is not None:
    enc_full.check()
