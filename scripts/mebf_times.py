"""Timing of the MEBF engine on one MI355X at 6040 x 3706 (the planted matrix of scripts/grecond_times.py) and, memory allowing, at
100 000 x 20 000: device-event medians of one growth chain (select + grow for both axes) and of one apply, the bytes each reads and
the fraction of 8 TB/s that gives, wall time of a k = 20 fit, and fixture case a on the device beside the reference's CPU time.

    python scripts/mebf_times.py [out.txt]        (profiles/mebf_times.txt is its output)
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from scipy.sparse import csr_matrix

from pybmf_amd.engine import BitMatrix
from pybmf_amd.mebf import MedianEngine
from pybmf_amd.models import MEBF

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
PEAK = 8e12
out = open(sys.argv[1] if len(sys.argv) > 1 else "mebf_times.txt", "w")


def say(*parts):
    line = " ".join(str(x) for x in parts)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def planted_ml1m():
    rng = np.random.RandomState(2310)
    m, n, k = 6040, 3706, 26
    U, V = rng.rand(m, k) < 0.06, rng.rand(n, k) < 0.03
    X = (U.astype(np.float32) @ V.astype(np.float32).T) > 0
    X ^= rng.rand(m, n) < 0.001
    return X.astype(np.uint8)


def planted_on_device(m, n, k, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    U = (torch.rand((m, k), device="cuda:0", generator=g) < 0.03).to(torch.float16)
    V = (torch.rand((n, k), device="cuda:0", generator=g) < 0.03).to(torch.float16)
    X = torch.empty((m, n), dtype=torch.uint8, device="cuda:0")
    for r0 in range(0, m, 8192):
        X[r0:r0 + 8192] = (U[r0:r0 + 8192] @ V.T > 0).to(torch.uint8)
    return X


def median_us(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def measure(X, label, t=0.7):
    m, n = X.shape
    eng = MedianEngine(BitMatrix(X, "cuda:0"))
    say(f"matrix {label}: {m} x {n}, {eng.sum_x} ones (density {eng.sum_x / (m * n):.4f}); one bit matrix = {eng.matrix_bytes / 2 ** 20:.1f} MiB; one MI355X")
    for step in range(2):
        cands = eng.growth(t)
        # bytes: the residual of both orientations once, and for the rows of b also x and pd (16-byte loads); the vector a per wave is cached
        read = sum(eng.N[c["axis"]] * eng.ld[c["axis"]] * 4 + 2 * c["nb"] * eng.ld[c["axis"]] * 4 for c in cands)
        us, lo, hi = median_us(lambda: eng.growth(t))
        say(f"  growth {step} (select + grow, both axes, one pinned read; includes the host's wait): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); "
            f"|a|, |b| per axis {[(c['na'], c['nb']) for c in cands]}; bytes read {read:.3e} = {read / (us * 1e-6) / PEAK:.3f} of 8 TB/s")
        cands = eng.growth(t)
        c = cands[0] if cands[0]["na"] and cands[0]["nb"] else cands[1]
        touched = 2 * 2 * 4 * (c["nb"] * eng.ld[c["axis"]] + c["na"] * eng.ld[1 - c["axis"]])     # rs and pd, read and written, of the hit rows
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.apply(c["u"], c["v"], c)
        b.record()
        b.synchronize()
        say(f"  apply {step} (both orientations, rows hit {c['nb']} + {c['na']}; a single call: it changes the state): {a.elapsed_time(b) * 1e3:.0f} us; "
            f"bytes read and written {touched:.3e}; residual {eng.residual_sum()}")
    del eng
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.time()
        model = MEBF(k=20, t=t)
        model.fit(X, **QUIET)
        wall = time.time() - t0
    say(f"  MEBF(k=20, t={t}).fit wall time: {wall:.2f} s, {len(model.logs['updates']) if 'updates' in model.logs else 0} factors, "
        f"{model._engine.reads} host reads (packing X, lil factor updates, one log row per factor)")


def main():
    measure(planted_ml1m(), "A (26 planted rectangles, 0.1 % flips, RandomState(2310))")
    free_b, _ = torch.cuda.mem_get_info("cuda:0")
    if free_b > 12 * 2 ** 30:
        measure(planted_on_device(100000, 20000, 40, 2311), "B (40 planted rectangles made on the device, seed 2311)")
    else:
        say(f"matrix B (100 000 x 20 000) left out: {free_b / 2 ** 30:.1f} GiB of device memory free")
    golden = os.path.join(ROOT, "tests", "golden")
    Xa = np.load(os.path.join(golden, "g27_mebf.npz"))["a_X"]
    meta = json.load(open(os.path.join(golden, "g27_mebf.json")))["cases"]["a"]
    for rep in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            model = MEBF(k=meta["k"], tol=meta["tol"], t=meta["t"])
            model.fit(csr_matrix(Xa.astype(np.float64)), **QUIET)
            wall = time.time() - t0
        rows = len(model.logs["updates"])
        say(f"fixture case a (96 x 72, k=6, t=0.8), run {rep}: {rows} factors in {wall:.3f} s = {wall / rows * 1e3:.1f} ms per factor (fit() wall time / "
            f"rows); the reference took 25 ms per factor on this case on a CPU host -- a different host")
    out.close()


if __name__ == "__main__":
    main()
