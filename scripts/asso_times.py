"""Time one best() sweep of Asso over all candidates at the MovieLens-1M shape: launches of bmf_asso_score + bmf_asso_pick on the
first factor's state and on the eighth's, warm, median of repeated launches by device events.  Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/asso_times.py` for the per-kernel split.

    python scripts/asso_times.py [output file]
"""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pybmf_amd.asso import AssoEngine
from pybmf_amd.engine import BitMatrix
from pybmf_amd.generators import PlantedBooleanOnDevice
from pybmf_amd.models import Asso

m, n, tau, w_fp, w_fn, REPS = 6040, 3706, 0.5, 0.5, 0.5, 20
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(eng, count, best_score):
    ts = []
    for _ in range(3):
        eng.launch_score(0, count, best_score, w_fp, w_fn)
    torch.cuda.synchronize()
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.launch_score(0, count, best_score, w_fp, w_fn)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


X = PlantedBooleanOnDevice(m, n, 10, density=(0.15, 0.15), seed=2410, noise=(0.05, 0.005), noise_seed=2411)
bits = BitMatrix(X, "cuda:0")
eng = AssoEngine(bits)
say(f"matrix: {m} x {n}, density {bits.sum_local / (m * n):.4f} (PlantedBooleanOnDevice, 10 factors, seed 2410); one MI355X")
t0 = time.time()
count = eng.build_basis(tau)
torch.cuda.synchronize()
say(f"bmf_asso_basis (tau {tau}): {count} candidates, {time.time() - t0:.3f} s with the first-call overhead")
ops = (-(-m // 64) * 64) * count * eng.ldx * 2
say(f"ldx = n_pad / 32 = {eng.ldx} words per bit row; 64 rows x 64 candidates per workgroup, 16-word stages")
say(f"AND-popcount word pairs per sweep, padded rows x candidates x ldx x 2 = {ops:.3e} (each one v_and_b32 + one v_bcnt_u32_b32)")
best = 0.0
for f in range(8):
    eng.row_counts()
    eng._cand[: eng.list.size].copy_(torch.from_numpy(eng.list))
    if f in (0, 7):
        med, lo, hi = timed(eng, int(eng.list.size), best)
        rate = 2 * ops * (eng.list.size / count) / (med * 1e-6)
        say(f"factor {f + 1}: {eng.list.size} candidates, best() sweep in one launch: median {med:.0f} us (min {lo:.0f}, max {hi:.0f}) per "
            f"bmf_asso_score + bmf_asso_pick (device events, {REPS} launches)")
        say(f"    {rate:.3e} VALU lane-operations per second in the word loop")
    hit = eng.best(best, w_fp, w_fn)
    assert hit is not None
    best = hit[2]
    u, v = eng.column(hit[1])
    eng.apply(u, v)
    eng.remove(hit[1])
with contextlib.redirect_stdout(io.StringIO()):
    model = Asso(tau=tau, k=8, w_fp=w_fp)
    t0 = time.time()
    model.fit(X, task="reconstruction", show_logs=False, show_result=False, save_model=False)
    wall = time.time() - t0
say(f"Asso(tau={tau}, k=8).fit wall time: {wall:.2f} s (packing X, candidates, 8 sweeps, lil factor updates, one log row per factor)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
