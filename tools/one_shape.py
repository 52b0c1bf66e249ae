#!/usr/bin/env python3
"""Runs REPS forwards of one batch shape (python tools/one_shape.py B S [reps] [shape]) — a fixed workload to put under rocprofv3 --kernel-trace --stats.
shape (or the environment variable ONE_SHAPE): a name of tools/enc_bench.py's SHAPES (default: e5-large)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from kirag_amd import bench_support as BS
B, S = int(sys.argv[1]), int(sys.argv[2]); reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = torch.device("cuda:0")
shape = sys.argv[4] if len(sys.argv) > 4 else os.environ.get("ONE_SHAPE")      # the environment variable reaches it through tools/shape_trace.sh
if shape:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import enc_bench as EB
    enc = EB.make_encoder(EB.SHAPES[shape])
else:
    enc = BS.make_hip_encoder(dev)
ids, mask = BS.synthetic_tokens(dev, B, S, seed=1)
if shape and "pad_token_id" in EB.SHAPES[shape]:
    ids = torch.where(mask != 0, ids, torch.full_like(ids, EB.SHAPES[shape]["pad_token_id"]))
for _ in range(reps):
    enc.forward(ids, mask, 0)
torch.cuda.synchronize()
