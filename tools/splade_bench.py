#!/usr/bin/env python3
"""What the SPLADE head costs: KR_POOL_SPLADE against mean-pool forwards on ONE handle with the MLM head (synthetic weights, bert-base shape: 12 layers,
H 768, V 30522), alternated in one process, device output.

    python tools/splade_bench.py [--batches 1x32,100x256,1024x128] [--rounds 6] [--once [--digest]]
    python tools/splade_bench.py --trace <directory of a rocprofv3 --kernel-trace run of --once>

A SPLADE forward differs from the mean-pool one in: its last layer is the same (mean pooling runs it on every row too), no k_pool, one H -> H EPI_GELU
projection, the transform LayerNorm, and the decoder launch [T] x [Vpad, H]^T with the EPI_SPLADE epilogue (2 T H Vpad FLOP: 6.2 TFLOP at 1024 x 128) plus the
[B, V] zero-fill and k_splade_finish.  --once runs one SPLADE forward per batch shape and nothing else: the run to put under a kernel trace; --trace prints,
from that trace, the decoder launch's time per FLOP next to the FF1 + GELU launches of the same forward.
The unflagged A/B against the parent commit's library is tools/m3_bench.py --plain (KIRAG_AMD_LIB, --dump for the bit-for-bit comparison)."""
import argparse, csv, glob, hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

BERT_BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=30522, max_position_embeddings=512,
                 type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1x32,100x256,1024x128")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--once", action="store_true")
ap.add_argument("--trace", default=None)
ap.add_argument("--digest", action="store_true", help="with --once: append the sha256 (16 hex digits) of the [B, V] result")
args = ap.parse_args()


def trace_summary(d):
    """per forward of the trace: decoder (k_proj epilogue 9) and FF1 + GELU (epilogue 2, all but the transform's, which is the last) time per FLOP"""
    H, FF, Vpad = BERT_BASE["hidden_size"], BERT_BASE["intermediate_size"], -(-BERT_BASE["vocab_size"] // 128) * 128
    rows = list(csv.DictReader(open(glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0])))
    seq = sorted(((r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), int(r["Start_Timestamp"])) for r in rows), key=lambda x: x[2])
    epi = lambda name: name.split("k_proj", 1)[1].split("<", 1)[1].split(",", 1)[0].strip() if "k_proj" in name else None
    starts = [i for i, s in enumerate(seq) if "k_embed_ln" in s[0]] + [len(seq)]
    for a, b in zip(starts[:-1], starts[1:]):
        fwd = seq[a:b]
        dec = [s for s in fwd if epi(s[0]) == "9"]
        gelu = [s for s in fwd if epi(s[0]) == "2"]
        if not dec or len(gelu) < 2:
            continue
        ff1 = np.array([s[1] for s in gelu[:-1]], dtype=np.float64)
        ratio_f = Vpad / FF                        # FLOP ratio decoder : one FF1 launch, whatever the token count
        other = {k: sum(s[1] for s in fwd if k in s[0]) / 1e3 for k in ("k_splade_finish", "k_splade_rowseq", "k_ln16_head")}
        print(f"forward: {len(fwd)} kernels, {sum(s[1] for s in fwd) / 1e6:.3f} ms of kernel time;  decoder launch {dec[0][1] / 1e3:.1f} us ({dec[0][0].split('(')[0][-60:]});  "
              f"FF1 + GELU median {np.median(ff1) / 1e3:.1f} us over {len(ff1)} launches;  FLOP ratio {ratio_f:.2f};  time per FLOP, decoder / FF1 = "
              f"{dec[0][1] / np.median(ff1) / ratio_f:.2f};  transform GELU {gelu[-1][1] / 1e3:.1f} us, " + ", ".join(f"{k} {v:.1f} us" for k, v in other.items()))


if args.trace:
    trace_summary(args.trace)
    sys.exit(0)

import torch
from kirag_amd import bench_support as BS
from kirag_amd.retriever.encoders import POOL_MEAN, POOL_SPLADE, HipBertForward

dev = torch.device("cuda:0")
ns = BS.SimpleNamespace(**BERT_BASE)
H, V = BERT_BASE["hidden_size"], BERT_BASE["vocab_size"]
state = dict(BS.synthetic_state(ns, dev, 0))
g = torch.Generator(device=dev); g.manual_seed(41)
rn = lambda *s: torch.randn(*s, generator=g, device=dev)
# logits of standard deviation ~2 under a bias in [-8, -0.5]: about half of the [B, V] entries end up zero, as in tests/splade_util.py
state.update({"cls.predictions.transform.dense.weight": rn(H, H) * 1.5 / H ** 0.5, "cls.predictions.transform.dense.bias": 0.3 * rn(H),
              "cls.predictions.transform.LayerNorm.weight": 1.0 + 0.1 * rn(H), "cls.predictions.transform.LayerNorm.bias": 0.1 * rn(H),
              "cls.predictions.decoder.weight": rn(V, H) * 2.0 / H ** 0.5, "cls.predictions.decoder.bias": -0.5 - 7.5 * torch.rand(V, generator=g, device=dev)})
enc = HipBertForward(ns, 0)
enc.load_state(state)
for B, S in (tuple(int(v) for v in t.split("x")) for t in args.batches.split(",")):
    ids, mask = BS.synthetic_tokens(dev, B, S, seed=1)
    if args.once:
        out = enc.forward(ids, mask, POOL_SPLADE); torch.cuda.synchronize()
        print(f"bert-base {B} x {S}: one SPLADE forward, zero share {float((out == 0).float().mean()):.3f}"
              + (f"  sha256 {hashlib.sha256(out.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]}" if args.digest else ""), flush=True)
        continue
    pools = (POOL_SPLADE, POOL_MEAN)
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
    f, e = np.array(res[POOL_SPLADE]), np.array(res[POOL_MEAN])
    out = enc.forward(ids, mask, POOL_SPLADE)
    print(f"bert-base {B} x {S} V={V}: splade median {np.median(f):.3f} ms (min {f.min():.3f}, max {f.max():.3f})  mean-pool median {np.median(e):.3f} ms "
          f"(min {e.min():.3f}, max {e.max():.3f})  difference of medians {1e3 * (np.median(f) - np.median(e)):+.1f} us  "
          f"(out {B * V * 4 / 2 ** 20:.1f} MiB, zero share {float((out == 0).float().mean()):.3f})", flush=True)
enc.check()
