#!/usr/bin/env python3
"""Encode-leg micro benchmark: passages/s of the HIP encoder (synthetic weights) at a BERT shape.

    python tools/enc_bench.py [n] [S] [ragged] [--shape e5-large|e5-small|minilm-l6 ...] [--hf-fp16]

Several --shape values run one after the other in the same process (default: e5-large).  --hf-fp16 also times HF BertModel in fp16 under torch on the
same batch: a yardstick, not a product path."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from kirag_amd import bench_support as BS

PEAK_MFMA_DENSE_16BIT = 2.5e15   # MI355X_MICROARCH.md: bf16/f16 dense MFMA peak

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int, nargs="?", default=1024)
ap.add_argument("S", type=int, nargs="?", default=128)
ap.add_argument("ragged", nargs="?", default="")
ap.add_argument("--shape", action="append", choices=sorted(BS.ENCODER_SHAPES))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hf-fp16", action="store_true")
args = ap.parse_args()
n, S, ragged = args.n, args.S, args.ragged == "ragged"
dev = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for shape in args.shape or ["e5-large"]:
    cfg = BS.ENCODER_SHAPES[shape]
    enc = BS.make_hip_encoder(dev, cfg)
    ids, mask = BS.synthetic_tokens(dev, n, S, seed=1, ragged=ragged)
    fl = BS.encoder_flops(enc.cfg, mask.sum(1))
    dt = timed(lambda: enc.forward(ids, mask, 0), args.reps)
    print(f"{shape} (H {cfg['hidden_size']}, {cfg['num_attention_heads']} heads of {cfg['hidden_size'] // cfg['num_attention_heads']}, L {cfg['num_hidden_layers']}) "
          f"tile={os.environ.get('KIRAG_AMD_PROJ_TILE','auto')} n={n} S={S} ragged={ragged}: {dt*1e3:.2f} ms  {n/dt:.0f} seq/s  {fl/dt/1e12:.0f} TFLOP/s  "
          f"{fl/dt/PEAK_MFMA_DENSE_16BIT:.3f} of MFMA peak  ({fl/n/1e9:.2f} GFLOP per sequence)", flush=True)
    del enc
    if args.hf_fp16:
        from transformers import BertConfig, BertModel
        m = BertModel(BertConfig(**{k: v for k, v in cfg.items() if k != "hidden_act"}), add_pooling_layer=False).to(dev).half().eval()
        with torch.no_grad():
            dt = timed(lambda: m(input_ids=ids, attention_mask=mask).last_hidden_state, args.reps)
        print(f"{shape} HF BertModel fp16 (yardstick) n={n} S={S} ragged={ragged}: {dt*1e3:.2f} ms  {n/dt:.0f} seq/s  {fl/dt/1e12:.0f} TFLOP/s", flush=True)
        del m
    torch.cuda.empty_cache()
