#!/usr/bin/env python3
"""What bge-m3's token-level heads cost: flagged (KR_POOL_WITH_SPARSE | KR_POOL_WITH_COLBERT) against unflagged CLS forwards on ONE handle with the heads
(synthetic weights), alternated in one process, device output.

    python tools/m3_bench.py [--shape xlmr-large] [--batches 1x64,100x256,1000x128] [--P 1024] [--rounds 6] [--once [--digest]]
    KIRAG_AMD_LIB=<another build> KIRAG_AMD_LIB_OLDER=1 python tools/m3_bench.py --plain [--shape e5-large] [--batches 1024x128] [--dump out.npy]

A flagged forward differs from the unflagged one in three things: its last layer runs on every row instead of the CLS rows, one more [T, H] x [H, P] product,
and the two token kernels (k_m3_sparse, k_m3_rows: 2 x B S P 4 bytes of traffic).  --once runs one flagged forward per batch shape and nothing else: the run
to put under a kernel trace.  --plain times the unflagged forward of a handle WITHOUT the heads (any build of the library: the A/B against the parent commit)
and with --dump writes its embeddings for a bit-for-bit comparison."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from kirag_amd import bench_support as BS
from kirag_amd.retriever.encoders import POOL_CLS, POOL_MEAN, POOL_WITH_COLBERT, POOL_WITH_SPARSE, HipBertForward

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="xlmr-large")
ap.add_argument("--batches", default="1x64,100x256,1000x128")
ap.add_argument("--P", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--once", action="store_true")
ap.add_argument("--plain", action="store_true")
ap.add_argument("--dump", default=None)
ap.add_argument("--digest", action="store_true", help="with --once: append the sha256 (16 hex digits) of the flagged forward's three blocks")
args = ap.parse_args()
sys.argv = sys.argv[:1]
import enc_bench as EB  # noqa: E402  (its shape table)

dev = torch.device("cuda:0")
cfg = EB.SHAPES[args.shape]
ns = BS.SimpleNamespace(**cfg)
H = cfg["hidden_size"]
state = dict(BS.synthetic_state(ns, dev, 0))
if not args.plain:
    assert cfg.get("model_type", "bert") in ("bert", "xlm-roberta", "roberta", "camembert"), "the heads run on BERT / RoBERTa handles"
    g = torch.Generator(device=dev); g.manual_seed(31)
    state.update({"colbert_linear.weight": torch.randn(args.P, H, generator=g, device=dev) / H ** 0.5, "colbert_linear.bias": 0.5 * torch.randn(args.P, generator=g, device=dev),
                  "sparse_linear.weight": 0.1 * torch.randn(1, H, generator=g, device=dev) / H ** 0.5, "sparse_linear.bias": torch.zeros(1, device=dev)})
enc = HipBertForward(ns, 0)
enc.load_state(state)
FLAGGED = POOL_CLS | POOL_WITH_SPARSE | POOL_WITH_COLBERT
dumps = []
for B, S in (tuple(int(v) for v in t.split("x")) for t in args.batches.split(",")):
    ids, mask = BS.synthetic_tokens(dev, B, S, seed=1)
    if "pad_token_id" in cfg:
        ids = torch.where(mask != 0, ids, torch.full_like(ids, cfg["pad_token_id"]))
    if args.once:
        blocks = enc.forward(ids, mask, FLAGGED); torch.cuda.synchronize()
        print(f"{args.shape} {B} x {S} P={args.P}: one flagged forward" + (f"  sha256 dense {EB.digest(blocks[0])} sparse {EB.digest(blocks[1])} colbert {EB.digest(blocks[2])}"
                                                                         if args.digest else ""), flush=True)
        continue
    pools = (POOL_MEAN,) if args.plain else (FLAGGED, POOL_CLS)
    res = {p: [] for p in pools}
    reps = 5 if B * S > 20000 else 20
    for rnd in range(args.rounds):
        for pool in pools:
            for _ in range(2):
                enc.forward(ids, mask, pool)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps):
                enc.forward(ids, mask, pool)
            torch.cuda.synchronize()
            res[pool].append((time.perf_counter() - t0) / reps * 1e3)
    if args.plain:
        e = np.array(res[POOL_MEAN])
        print(f"{args.shape} {B} x {S} unflagged mean pool, lib {os.environ.get('KIRAG_AMD_LIB', '(this build)')}: median {np.median(e):.3f} ms (min {e.min():.3f}, max {e.max():.3f})",
              flush=True)
        dumps.append(enc.forward(ids, mask, POOL_MEAN).cpu().numpy())
        continue
    f, e = np.array(res[FLAGGED]), np.array(res[POOL_CLS])
    print(f"{args.shape} {B} x {S} P={args.P}: flagged median {np.median(f):.3f} ms (min {f.min():.3f}, max {f.max():.3f})  cls median {np.median(e):.3f} ms "
          f"(min {e.min():.3f}, max {e.max():.3f})  difference of medians {1e3 * (np.median(f) - np.median(e)):+.1f} us  "
          f"(token blocks {B * S * (args.P + 1) * 4 / 2 ** 20:.1f} MiB)", flush=True)
enc.check()
if args.dump and dumps:
    np.save(args.dump, np.concatenate([d.reshape(-1) for d in dumps]))
