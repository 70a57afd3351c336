"""Changed factor words per iteration on the bench's trajectory: the fraction of rows whose ubits word and of columns whose vbits word
differ from the previous iteration's -- what the incremental cover count (bmf_cover_delta) pays for.  Outside any timing: one
iteration per call, the words read back in between.

    python scripts/cover_changed_words.py [--m 100000 --n 20000 --k 64 --iters 65 --operands i8x3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from pybmf_amd import _lib as L
from pybmf_amd.engine import BitMatrix, MUEngine
from pybmf_amd.generators import PlantedBooleanOnDevice

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=100_000)
ap.add_argument("--n", type=int, default=20_000)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--iters", type=int, default=65)
ap.add_argument("--operands", default="i8x3", choices=sorted(bench.OPND))
a = ap.parse_args()
panel, terms = bench.OPND[a.operands]
device = torch.device("cuda", 0)
m, n, k = a.m, a.n, a.k
dens = 0.067 if k >= 32 else 0.2
X = BitMatrix(PlantedBooleanOnDevice(m, n, k, density=(dens, dens), seed=1000, noise=(0.05, 0.01), noise_seed=2000, device=device), device)
eng = MUEngine(X, k=k, mode=L.MODE_PENALTY, terms=terms, with_mae=False, tol=-1.0, min_diff=-1.0, max_iter=a.iters + 1, panel=panel)
U0, V0 = bench.host_init(eng.sum_x / (float(m) * n), m, n, k, seed=2024)
eng.load_factors(U0, V0)
eng.prepare(1.0)
print(f"{m} x {n}, k = {k}, {a.operands}; reg 1.0 x 1.02^t, host_init(seed 2024)")
print("iter  rows_changed  cols_changed  rows_nonzero  TP")
reg = np.float64(1.0)
for it in range(1, a.iters + 1):
    ub, vb = eng.ubits.clone(), eng.vbits.clone()
    eng.run([float(reg)], it0=it)
    reg = min(reg * np.float64(1.02), np.float64(1e10))
    rows, cols = int((eng.ubits[:m] != ub[:m]).sum()), int((eng.vbits[:n] != vb[:n]).sum())
    log, _ = eng.read_log()
    print(f"{it:4d}  {rows / m:12.5f}  {cols / n:12.5f}  {int((eng.ubits[:m] != 0).sum()) / m:12.5f}  {int(log[-1, L.LOG_TP])}")
