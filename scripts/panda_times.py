"""Timing of the Panda engine on one MI355X at 6040 x 3706 (the planted matrix of scripts/grecond_times.py) and, memory allowing, at
100 000 x 20 000: device-event medians of the couples score, of one core scan (all columns against one residual column, with its
close) and of one extension scan with its row pass, the bytes each reads and the fraction of 8 TB/s that gives, wall time of a
k = 20 fit, and fixture case c on the device beside the reference's CPU time.

    python scripts/panda_times.py [out.txt]        (profiles/panda_times.txt is its output)
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

from pybmf_amd._lib import check, lib, ptr
from pybmf_amd.engine import BitMatrix
from pybmf_amd.models import Panda
from pybmf_amd.panda import PatternEngine

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
PEAK = 8e12
out = open(sys.argv[1] if len(sys.argv) > 1 else "panda_times.txt", "w")


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


def measure(X, label):
    m, n = X.shape
    eng = PatternEngine(BitMatrix(X, "cuda:0"))
    one = eng.bits.m_pad * eng.bits.n_pad // 8
    say(f"matrix {label}: {m} x {n}, {eng.sum_x} ones (density {eng.sum_x / (m * n):.4f}); one bit matrix = {one / 2 ** 20:.1f} MiB; one MI355X")
    s = eng._stream
    # couples score: the transposed residual once, and one 4-byte row count per residual one (gathered: counted at 4 bytes each)
    read = n * eng.W * 4 + 4 * eng.sum_x
    us, lo, hi = median_us(lambda: check(lib.bmf_panda_couples(ptr(eng.rs[0]), n, eng.W, ptr(eng._count[1]), m, ptr(eng._couples), s), "couples"))
    say(f"  couples score (launch only, no read): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); bytes read {read:.3e} = {read / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    order = np.flip(np.argsort(eng.scores("couples-frequency"), kind="stable"))
    first, E = int(order[0]), order[1:]
    eng.set_candidates(E)

    def core():       # T is reset by a device copy inside the timed region: W words
        h0 = eng.start_core(first)
        return eng.core_scan(0, len(E), 1, 1.0, 1.0, 1, h0)
    read = len(E) * eng.W * 4
    us, lo, hi = median_us(core)
    i, h1, _ = core()
    say(f"  core scan (T := one column and its read, then all {len(E)} other columns against T, pick, close, one pinned read; includes the host's "
        f"two waits): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); winner at position {i}, |T| {h1}; bytes read {read:.3e} = "
        f"{read / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    us, lo, hi = median_us(lambda: check(lib.bmf_panda_core_scan(ptr(eng.rs[0]), n, eng.W, eng._p_T, ptr(eng._cand), len(E), 1, 1.0, 1.0, 1, h1,
                                                                 ptr(eng._a), eng._p_core, s), "core_scan"))
    say(f"  core scan, the two kernels alone (no close, no read): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}) = {read / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    # extension: the scan reads the residual and the cover of every candidate; the row pass behind a winner reads both row-major matrices
    h0 = eng.start_core(first)
    eng.set_items([first])
    cost = float(eng.sum_x)
    r = eng.ext_scan(0, len(E), h0, 2, 1.0, 1.0, 1.0, cost)
    read = 2 * len(E) * eng.W * 4 + (2 * m * eng.nvw * 4 if r["i"] >= 0 else 0)

    def ext():
        eng.start_core(first)
        eng.set_items([first])
        return eng.ext_scan(0, len(E), h0, 2, 1.0, 1.0, 1.0, cost)
    us, lo, hi = median_us(ext)
    say(f"  extension scan + row pass (T, I reset, all {len(E)} candidates, the winner joins I, every row outside T tested, one pinned read; includes "
        f"the host's waits): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); winner at position {r['i']}, rows added {r['added']}; bytes read "
        f"{read:.3e} = {read / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    del eng
    for init_method in ("correlation", "couples-frequency"):
        with contextlib.redirect_stdout(io.StringIO()):
            torch.cuda.synchronize()
            t0 = time.time()
            model = Panda(k=20, init_method=init_method)
            model.fit(X, **QUIET)
            wall = time.time() - t0
        rows = model.logs["updates"].values.tolist() if "updates" in model.logs else []
        say(f"  Panda(k=20, init_method={init_method!r}).fit wall time: {wall:.2f} s, {len(rows)} factors, {model._engine.reads} host reads, "
            f"last cost {rows[-1][1] if rows else None}, shapes {[r[2] for r in rows[:6]]} ...")
        del model


def main():
    measure(planted_ml1m(), "A (26 planted rectangles, 0.1 % flips, RandomState(2310))")
    free_b, _ = torch.cuda.mem_get_info("cuda:0")
    if free_b > 12 * 2 ** 30:
        measure(planted_on_device(100000, 20000, 40, 2311), "B (40 planted rectangles made on the device, seed 2311)")
    else:
        say(f"matrix B (100 000 x 20 000) left out: {free_b / 2 ** 30:.1f} GiB of device memory free")
    golden = os.path.join(ROOT, "tests", "golden")
    Xc = np.load(os.path.join(golden, "g28_panda.npz"))["c_X"]
    meta = json.load(open(os.path.join(golden, "g28_panda.json")))["cases"]["c"]
    for rep in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            model = Panda(k=meta["k"], tol=meta["tol"], init_method=meta["init_method"])
            model.fit(csr_matrix(Xc.astype(np.float64)), **QUIET)
            wall = time.time() - t0
        rows = len(model.logs["updates"])
        say(f"fixture case c (96 x 72, k=5, correlation), run {rep}: {rows} factors in {wall:.3f} s = {wall / rows * 1e3:.1f} ms per factor (fit() wall "
            f"time / rows); the reference took 0.28 s per factor on this case on a CPU host (tests/golden/make_golden_panda.py prints it, "
            f"from a run without its line tracer) -- a different host")
    out.close()


if __name__ == "__main__":
    main()
