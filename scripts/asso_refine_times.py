"""Time the two refiners of Asso at the MovieLens-1M shape: one AssoIter column visit (bmf_asso_refine_column) at k = 8 and k = 64, one
AssoOpt pass over all rows (bmf_asso_refine_rows) at k = 8, 12 and the limit 16; warm, median of repeated launches by device events.
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/asso_refine_times.py` for the per-kernel split.

    python scripts/asso_refine_times.py [output file]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pybmf_amd.asso_refine import AssoRefineEngine
from pybmf_amd.engine import BitMatrix
from pybmf_amd.generators import PlantedBooleanOnDevice

m, n = 6040, 3706
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(launch, reps):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


X = PlantedBooleanOnDevice(m, n, 10, density=(0.15, 0.15), seed=2410, noise=(0.05, 0.005), noise_seed=2411)
bits = BitMatrix(X, "cuda:0")
eng = AssoRefineEngine(bits)
say(f"matrix: {m} x {n}, density {bits.sum_local / (m * n):.4f} (PlantedBooleanOnDevice, 10 factors, seed 2410); one MI355X; ldx = {eng.ldx} words")
rng = np.random.RandomState(2512)
for k in (8, 64):
    U, V = rng.rand(m, k) < 1.5 / k, rng.rand(n, k) < 0.15
    eng.load_factors(U, V)
    ones = int(U.sum())
    med, lo, hi = timed(lambda: eng.refine_column(k // 2, 0.5, 0.5), 20)
    say(f"AssoIter column visit, k = {k} ({ones / m:.2f} factors per row): median {med:.0f} us (min {lo:.0f}, max {hi:.0f}) per "
        f"bmf_asso_refine_column with its record read (device events, 20 launches)")
    say(f"    X read once: {m * eng.ldx * 4 / 1e6:.2f} MB; V staged per workgroup: {k * eng.ldx * 4 / 1024:.0f} KiB x {-(-m // 32)} workgroups; "
        f"LDS words read: about {(ones + m) * eng.ldx:.3e}; popcounts: {4 * m * eng.ldx:.3e}")
for k in (8, 12, 16):
    U, V = rng.rand(m, k) < 1.5 / k, rng.rand(n, k) < 0.15
    eng.load_factors(U, V)
    med, lo, hi = timed(lambda: eng.optimal_rows(1.0, 1.0), 5 if k < 16 else 3)
    pops = 2.0 * m * eng.ldx * 2 ** k
    say(f"AssoOpt all rows, k = {k}: median {med:.0f} us (min {lo:.0f}, max {hi:.0f}) per bmf_asso_refine_rows with its record read; "
        f"{pops:.3e} popcounts = {pops / (med * 1e-6):.3e} per second")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
