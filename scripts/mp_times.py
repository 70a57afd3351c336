"""Timing of the MessagePassing iteration (bmf_mp_step, csrc/mp.hip) on one MI355X at 10 000 x 2 000, W = 'full': k = 8 and k = 16 (the
register tiers: every plane read once and written once, 4 x 8 k bytes per cell) and k = 32 (the two-sweep form, 6 x 8 k), plus k = 16
under a 70 % pattern.  Warm chip (WARM untimed iterations), then STEPS iterations enqueued back to back without a host read between
device events; REPS such windows, median, min and max stated; beside them the engine's own step() (one 8-byte synchronising read per
iteration, what a fit pays).  Bytes per second are the traffic model's bytes over the measured time.  For scale: the NumPy
restatement's iterations per second at 1 000 x 500, k = 16 on the host.

    python scripts/mp_times.py [out.txt]        (profiles/mp_times.txt is its output)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from pybmf_amd._lib import check, lib, ptr
from pybmf_amd.engine import BitMatrix
from pybmf_amd.mp import MessagePassingEngine

WARM, STEPS, REPS = 5, 20, 5
out = open(sys.argv[1] if len(sys.argv) > 1 else "mp_times.txt", "w")


def say(*parts):
    line = " ".join(str(x) for x in parts)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def planted(m, n, k, rs):
    U, V = rs.rand(m, k) < 0.2, rs.rand(n, k) < 0.2
    X = (U.astype(np.float32) @ V.astype(np.float32).T) > 0
    return (X ^ (rs.rand(m, n) < 0.03)).astype(np.uint8)


def enqueue(eng):
    check(lib.bmf_mp_step(ptr(eng.bits.bits), eng._wbits(), eng.bits.ldx, eng.m, eng.n, eng.k, eng.ldn, eng.co1, eng.co0, eng.lr, eng.cx, eng.cy,
                          ptr(eng.Phi), ptr(eng.Psi), ptr(eng.work), ptr(eng.Xi), ptr(eng.Ups), ptr(eng._d_dev), ptr(eng.ubits), ptr(eng.vbits),
                          eng._stream), "bmf_mp_step")


def run(m, n, k, masked, rs):
    X = planted(m, n, 8, rs)
    bits = BitMatrix(X, "cuda:0")
    pat = BitMatrix((rs.rand(m, n) < 0.7).astype(np.uint8), "cuda:0") if masked else None
    eng = MessagePassingEngine(bits, k, pattern=pat, prior_u=0.3, prior_v=0.3)
    eng.start(0)
    for _ in range(WARM):
        eng.step()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            enqueue(eng)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / STEPS)
    ts.sort()
    med = ts[len(ts) // 2]
    t0 = time.perf_counter()
    for _ in range(STEPS):
        d = eng.step()
    wall = (time.perf_counter() - t0) / STEPS
    sweeps = 4 if k <= 16 else 6
    model = sweeps * 8.0 * k * m * n
    say(f"{m} x {n}  k = {k:2d}  {'70 % pattern' if masked else 'full pattern':12s}  enqueued: {med * 1e3:8.3f} ms / iteration (min {ts[0] * 1e3:.3f}, max {ts[-1] * 1e3:.3f})"
        f" = {1 / med:7.1f} iterations/s, {model / med / 1e12:5.2f} TB/s of the model's {sweeps} x 8 k bytes per cell;"
        f"  step() with its read: {wall * 1e3:8.3f} ms = {1 / wall:7.1f} iterations/s;  d after {WARM + (REPS + 1) * STEPS} iterations = {d:.3e}")
    del eng, bits, pat
    torch.cuda.empty_cache()


say(f"# MessagePassing iteration times; device: {torch.cuda.get_device_name(0)}; warm {WARM}, {REPS} windows of {STEPS} iterations, median")
rs = np.random.RandomState(1)
for k, masked in ((8, False), (16, False), (16, True), (32, False)):
    run(10_000, 2_000, k, masked, rs)

import mp_ref as R  # noqa: E402
X = planted(1000, 500, 8, rs) != 0
ref = R.RefEngine(X, 16, None, prior_u=0.3, prior_v=0.3)
ref.start(0)
ref.step()
t0 = time.perf_counter()
for _ in range(3):
    ref.step()
say(f"NumPy restatement (tests/mp_ref.py) on the host, 1000 x 500, k = 16: {3 / (time.perf_counter() - t0):.2f} iterations/s")
out.close()
