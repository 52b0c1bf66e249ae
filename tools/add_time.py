#!/usr/bin/env python3
"""Device time of kr_index_add (k_add_rows: fp32 rows -> 16-bit copy + error bounds) per 250k x 1024 chunk, rows resident on the device.
Usage: [KIRAG_AMD_LIB=<another build>] python tools/add_time.py [chunks] [rows_per_chunk] [dim]   -> one line: median / min / max ms per chunk"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from kirag_amd.bench_support import CorpusDist
from kirag_amd.retriever.index import FlatIPIndex
chunks = int(sys.argv[1]) if len(sys.argv) > 1 else 12
m = int(sys.argv[2]) if len(sys.argv) > 2 else 250_000
d = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
dev = torch.device("cuda:0")
cd = CorpusDist("gaussian", d, dev)
g = torch.Generator(device=dev); g.manual_seed(3)
x = cd.rows(m, g)
ix = FlatIPIndex(d, device=0); ix.reserve(m * (chunks + 2))
for _ in range(2):                                   # warm-up: first-touch of the mapped chunks, kernel load
    ix.add(x)
torch.cuda.synchronize()
ms = []
for _ in range(chunks):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); ix.add(x); b.record(); b.synchronize()
    ms.append(a.elapsed_time(b))
ms = np.array(ms)
print(f"kr_index_add {m} x {d}: median {np.median(ms):.4f} ms, min {ms.min():.4f}, max {ms.max():.4f} over {chunks} chunks (device copy of the rows included); bounds {ix.bounds().tolist()}")
