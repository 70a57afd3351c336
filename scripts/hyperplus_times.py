"""Timing of the HyperPlus engine on one MI355X at 6040 x 3706 (the planted matrix of scripts/hyper_times.py): device-event medians of
one bmf_hyperplus_pairs launch over 500 sampled pairs and over all 19 900 pairs of k = 200 factors (one rectangle per column of the
200 fullest columns, what Hyper ends with on this matrix; the cover is theirs), the bytes the launch asks for and the fraction of
8 TB/s that gives, and the wall time of a HyperPlus(target_k=10) fit on the rectangles of the first 100 columns.  (The fit keeps the
reference's lil copies of U and V per round: 90 rounds of them at 100 factors, thousands of MB at 400.)

    python scripts/hyperplus_times.py [out.txt]        (profiles/hyperplus_times.txt is its output)
"""
import contextlib
import io
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from scipy.sparse import lil_matrix

from pybmf_amd._lib import check, lib, ptr
from pybmf_amd.engine import BitMatrix
from pybmf_amd.hyperplus import HyperPlusEngine
from pybmf_amd.models import HyperPlus

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
PEAK = 8e12
TOP = 200
FIT_COLUMNS = 100
out = open(sys.argv[1] if len(sys.argv) > 1 else "hyperplus_times.txt", "w")


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


def column_rectangles(X, cols):
    """One rectangle per listed column: (its rows) x (the column)."""
    return [[int(t) for t in np.nonzero(X[:, j])[0]] for j in cols], [[int(j)] for j in cols]


def measure(X):
    m, n = X.shape
    eng = HyperPlusEngine(BitMatrix(X, "cuda:0"))
    row = eng.W * 4
    say(f"matrix A (26 planted rectangles, 0.1 % flips, RandomState(2310)): {m} x {n}, {eng.sum_x} ones (density {eng.sum_x / (m * n):.4f}); "
        f"one bit row = {row} bytes; one MI355X")
    top = np.sort(np.argsort(X.sum(axis=0), kind="stable")[-TOP:])
    T, I = column_rectangles(X, top)
    eng.load_factors(T, I)
    say(f"  k = {TOP} factors: one rectangle per column of the {TOP} fullest columns ({sum(len(t) for t in T)} ones covered, FP {eng.counts()[1]})")
    every = np.array([(a, b) for a in range(TOP) for b in range(a + 1, TOP)], dtype=np.int32)
    sample = every[np.random.RandomState(2312).choice(len(every), 500, replace=False)]
    for label, pairs in (("500 sampled pairs", sample), (f"all {len(every)} pairs", every)):
        count = len(pairs)
        pr = torch.from_numpy(np.ascontiguousarray(pairs)).to("cuda:0")
        rec = torch.empty((count, 5), dtype=torch.int64, device="cuda:0")
        us, lo, hi = median_us(lambda: check(lib.bmf_hyperplus_pairs(ptr(eng.u_t), ptr(eng.v), TOP, ptr(eng.x_t), ptr(eng.pd_t), n, eng.W, eng.nvw, ptr(pr),
                                                                      count, ptr(rec), eng._stream), "pairs"))
        new_fp = rec.cpu().numpy()[:, 0]
        asked = count * (2 * 4 + 2) * row          # per pair: 2 columns of I, each x_t[j], pd_t[j] and the two T rows; the two T rows once more
        distinct = (2 * TOP + 2 * TOP) * row + count * (8 + 40)
        say(f"  bmf_hyperplus_pairs, {label} (launch only, no read): median {us:.0f} us (min {lo:.0f}, max {hi:.0f}); bytes asked for {asked:.3e} "
            f"(per pair and column of I: x_t[j], pd_t[j] and the two T rows; the two T rows once more for |T|) = {asked / (us * 1e-6) / PEAK:.4f} of 8 TB/s; "
            f"distinct bytes {distinct:.3e} (the {TOP} T rows, the {TOP} columns of x_t and pd_t, the v rows, pairs and records: all of it "
            f"stays in cache) = {distinct / (us * 1e-6) / PEAK:.6f} of 8 TB/s; new_fp min {new_fp.min()}, median {int(np.median(new_fp))}, max {new_fp.max()}")
    t0 = time.time()
    eng.score_pairs(every)
    say(f"  score_pairs() of all {len(every)} pairs with its pinned read of 5 int64 each: {(time.time() - t0) * 1e3:.2f} ms wall")
    del eng


def fit(X):
    T, I = column_rectangles(X, [j for j in range(X.shape[1]) if X[:, j].any()])
    k = len(T)
    U, V = lil_matrix((X.shape[0], k)), lil_matrix((X.shape[1], k))
    for f, (t, cols) in enumerate(zip(T, I)):
        U[t, f], V[cols, f] = 1, 1
    hyper = types.SimpleNamespace(U=U, V=V, T=T, I=I, k=k, logs={})
    for savings in ("reference", "new_fp"):
        hyper.logs = {}
        with contextlib.redirect_stdout(io.StringIO()):
            np.random.seed(2313)
            torch.cuda.synchronize()
            t0 = time.time()
            model = HyperPlus(model=hyper, target_k=10, samples=500, savings=savings)
            model.fit(X, **QUIET)
            wall = time.time() - t0
        rows = model.logs["refinements"].values.tolist()
        eng = model._engine
        say(f"  HyperPlus(target_k=10, samples=500, savings='{savings}').fit on {X.shape[0]} x {X.shape[1]} (the leading columns, one rectangle per "
            f"non-empty column: k = {k}), wall time: {wall:.2f} s, {len(rows)} rounds, k = {model.k} at the end, {eng.reads} host reads, "
            f"FP {eng.counts()[1]} of {eng.sum_x} ones (FPB {rows[-1][4]:.4f}), trials {sum(len(t) for t, _ in model.trials)}")


def main():
    say("python scripts/hyperplus_times.py profiles/hyperplus_times.txt")
    XA = planted_ml1m()
    measure(XA)
    fit(np.ascontiguousarray(XA[:, :FIT_COLUMNS]))
    out.close()


if __name__ == "__main__":
    main()
