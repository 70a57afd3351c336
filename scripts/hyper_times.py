"""Timing of the Hyper engine on one MI355X at 6040 x 3706 (the planted matrix of scripts/grecond_times.py) and, memory allowing, at
100 000 x 20 000: device-event medians of one level step of the miner (all pairs of the 200 fullest columns: 19 900 candidates) and of
one evaluate launch (the n singletons and those 19 900 pairs on the residual X), the bytes each moves and the fraction of 8 TB/s that
gives, and the wall time of a whole fit on the first 400 columns of the smaller matrix.  (Every non-empty column ends as a factor of
its own at a min_support that keeps the planted blocks' subsets from being frequent, and a factor costs the host tens of milliseconds
in the factor matrices and the log: all 3706 columns would time those, for minutes.)

    python scripts/hyper_times.py [out.txt]        (profiles/hyper_times.txt is its output)
"""
import contextlib
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pybmf_amd._lib import check, lib, ptr
from pybmf_amd.engine import BitMatrix
from pybmf_amd.hyper import HyperEngine
from pybmf_amd.models import Hyper

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
PEAK = 8e12
TOP = 200
out = open(sys.argv[1] if len(sys.argv) > 1 else "hyper_times.txt", "w")


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
    eng = HyperEngine(BitMatrix(X, "cuda:0"))
    row = eng.W * 4
    say(f"matrix {label}: {m} x {n}, {eng.sum_x} ones (density {eng.sum_x / (m * n):.4f}); one bit row = {row} bytes; one MI355X")
    s = eng._stream
    top = np.sort(np.argsort(eng._count.cpu().numpy(), kind="stable")[-TOP:])
    pairs = [(int(a), int(b)) for i, a in enumerate(top) for b in top[i + 1:]]
    count = len(pairs)
    tid, cnt = eng._level(eng.x_t, n, pairs)
    pr, cn = eng._ints(pairs), torch.empty(count, dtype=torch.int32, device="cuda:0")
    us, lo, hi = median_us(lambda: check(lib.bmf_hyper_level(ptr(eng.x_t), n, ptr(eng.x_t), n, eng.W, ptr(pr), count, ptr(tid), ptr(cn), s), "level"))
    moved, written = 3 * count * row, count * row
    say(f"  level step, {count} candidates (all pairs of the {TOP} fullest columns; launch only, no read): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); "
        f"bytes moved {moved:.3e} (two rows read, one written per candidate) = {moved / (us * 1e-6) / PEAK:.4f} of 8 TB/s; the {TOP} source rows "
        f"({TOP * row:.3e} bytes) stay in cache, the written rows alone are {written:.3e} bytes = {written / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    eng._adopt([list(p) for p in pairs], [int(c) for c in cnt], [(tid, list(range(count)))])
    del tid
    C = eng.n_cand
    ids = eng._ints(np.arange(C))
    us, lo, hi = median_us(lambda: check(lib.bmf_hyper_eval(ptr(eng._tid), ptr(eng.rs_t), n, eng.W, ptr(eng._items), eng.maxlen, ptr(ids), C, C,
                                                            ptr(eng._scratch), ptr(eng._rec), s), "eval"))
    moved = (2 * C + n + 2 * count) * row          # per candidate: its tidset read, T written, one residual row read per item
    say(f"  evaluate launch, {C} candidates ({n} singletons, {count} pairs; launch only, no read): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); "
        f"bytes moved {moved:.3e} (tidset read, T written, one residual row read per item) = {moved / (us * 1e-6) / PEAK:.4f} of 8 TB/s; without the "
        f"residual rows, which the cache serves: {2 * C * row:.3e} bytes = {2 * C * row / (us * 1e-6) / PEAK:.4f} of 8 TB/s")
    t0 = time.time()
    nT, _ = eng.evaluate_all()
    say(f"  evaluate_all() with its pinned read of {C} records: {(time.time() - t0) * 1e3:.2f} ms wall; {int((nT > 0).sum())} candidates have a non-empty T")
    del eng


def fit(X, min_support):
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.time()
        model = Hyper(min_support=min_support)
        model.fit(X, **QUIET)
        wall = time.time() - t0
    rows = model.logs["updates"].values.tolist() if "updates" in model.logs else []
    eng = model._engine
    say(f"  Hyper(min_support={min_support}).fit on {X.shape[0]} x {X.shape[1]} (the leading columns), wall time: {wall:.2f} s, {eng.n_cand} candidates ({eng.n_cand - eng.n} mined itemsets), {len(rows)} factors, "
        f"iter sum {sum(r[2] for r in rows)}, {eng.reads} host reads, residual {eng.residual_sum()}, shapes {[r[3] for r in rows[:6]]} ...")


def main():
    say("python scripts/hyper_times.py profiles/hyper_times.txt")
    XA = planted_ml1m()
    measure(XA, "A (26 planted rectangles, 0.1 % flips, RandomState(2310))")
    fit(XA[:, :400], 0.15)
    free_b, _ = torch.cuda.mem_get_info("cuda:0")
    if free_b > 12 * 2 ** 30:
        measure(planted_on_device(100000, 20000, 40, 2311), "B (40 planted rectangles made on the device, seed 2311)")
    else:
        say(f"matrix B (100 000 x 20 000) left out: {free_b / 2 ** 30:.1f} GiB of device memory free")
    out.close()


if __name__ == "__main__":
    main()
