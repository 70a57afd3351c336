"""Timing of the GreConD+ engine on one MI355X at 6040 x 3706 (the planted matrix of scripts/grecond_times.py) and at 32256 x 20000, the
most rows the concept scan takes: device-event medians of the counts pass (bytes read, fraction of 8 TB/s), of one expansion of a concept
found after a k = 20 fit (steps, us per step, host reads) and of the rebuild, wall time of GreConDPlus(k=20).fit, and fixture case a on
the device beside the reference's CPU time.  There is no speed gate: these numbers are the record.

    python scripts/grecondplus_times.py [out.txt]        (profiles/grecondplus_times.txt is its output)
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

from pybmf_amd.models import GreConDPlus

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
PEAK = 8e12
out = open(sys.argv[1] if len(sys.argv) > 1 else "grecondplus_times.txt", "w")


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


def measure(X, label, w_fp=0.3):
    m, n = X.shape
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.time()
        model = GreConDPlus(k=20, w_fp=w_fp)
        model.fit(X, **QUIET)
        wall = time.time() - t0
    eng = model._engine
    rows = model.logs["updates"].values.tolist()
    one = eng.bits.m_pad * eng.bits.n_pad // 8
    say(f"matrix {label}: {m} x {n}, {eng.sum_x} ones (density {eng.sum_x / (m * n):.4f}); one bit matrix = {one / 2 ** 20:.1f} MiB; one MI355X")
    say(f"  GreConDPlus(k=20, w_fp={w_fp}).fit wall time: {wall:.2f} s, {len(rows)} log rows, {model.U.shape[1]} factors, expansion steps per "
        f"factor {model.n_steps}, factors swallowed {sum(model.n_covered)}, subset tests passed / rows / columns pruned "
        f"{[sum(p[i] for p in model.n_pruned) for i in range(3)]}, shapes {[r[3] for r in rows[:5]]} ...")
    # the counts pass: X and the residual in both orientations, once each
    read = 4 * one
    us, lo, hi = median_us(eng.launch_counts)
    say(f"  counts pass (rows against v and columns against u, two launches, no read): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); bytes read "
        f"{read:.3e} = {read / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    # one expansion of the next concept on the residual the fit left
    score, u, v = eng.concept()
    if score > 0:
        u_exp, v_exp, n_iter = eng.expand(u, v, w_fp, 1 - w_fp)
        for steps in (None, 16, 1):
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.time()
                eng.expand(u, v, w_fp, 1 - w_fp, steps=steps)
                ts.append(time.time() - t0)
            ts.sort()
            say(f"  one expansion of the next concept (score {score}), steps per launch {steps}: {n_iter} steps, {eng.host_reads} host reads, median wall "
                f"{ts[2] * 1e6:.0f} us = {ts[2] * 1e6 / n_iter:.1f} us per step (sets uploaded, counts pass, steps, record and sets read)")
        eng.set_expansion_state(u, v)
        n_launch = min(n_iter, 64)
        us, lo, hi = median_us(lambda: eng.launch_steps(w_fp, 1 - w_fp, 1), reps=max(n_launch - 3, 1))
        say(f"  a launch of one step alone (device events, no read): median {us:.1f} us (min {lo:.1f}, max {hi:.1f})")
    else:
        say("  no concept left after the fit: expansion not timed")
    Ub, Vb = model._Ub, model._Vb
    us, lo, hi = median_us(lambda: eng.rebuild(Ub, Vb), reps=10)
    say(f"  rebuild from {Ub.shape[0]} factors (factor bits uploaded, both orientations, per-column counts read; includes the host's wait): median "
        f"{us:.0f} us (min {lo:.0f}, max {hi:.0f}); bytes read and written {5 * one:.3e} = {5 * one / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    del model, eng


def main():
    measure(planted_ml1m(), "A (26 planted rectangles, 0.1 % flips, RandomState(2310))")
    free_b, _ = torch.cuda.mem_get_info("cuda:0")
    if free_b > 6 * 2 ** 30:
        measure(planted_on_device(32256, 20000, 40, 2311), "B (40 planted rectangles made on the device, seed 2311; 32256 rows is the limit of the concept scan)")
    else:
        say(f"matrix B (32256 x 20000) left out: {free_b / 2 ** 30:.1f} GiB of device memory free")
    golden = os.path.join(ROOT, "tests", "golden")
    Xa = np.load(os.path.join(golden, "g29_grecondplus.npz"))["a_X"]
    meta = json.load(open(os.path.join(golden, "g29_grecondplus.json")))["cases"]["a"]
    for rep in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            model = GreConDPlus(k=meta["k"], tol=meta["tol"], w_fp=meta["w_fp"], w_fn=meta["w_fn"])
            model.fit(csr_matrix(Xa.astype(np.float64)), **QUIET)
            wall = time.time() - t0
        rows = len(model.logs["updates"])
        say(f"fixture case a (96 x 72, k=5), run {rep}: {rows} log rows in {wall:.3f} s = {wall / rows * 1e3:.1f} ms per log row (fit() wall time / "
            f"rows); the reference took 0.05 to 0.13 s per log row on this case on a CPU host, and 0.25 s per log row on case b "
            f"(tests/golden/make_golden_grecondplus.py prints it) -- a different host")
    out.close()


if __name__ == "__main__":
    main()
