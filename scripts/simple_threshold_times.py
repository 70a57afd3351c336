"""Timing of one 1600-trial threshold search (40 x 40 grid) on one MI355X at 6040 x 3706, k = 16 and k = 64, two ways, both enqueued
without a host read and bracketed by device events:

  grid   bmf_thresh_panels for both factors + ONE bmf_grid_cover_count (csrc/thresh_grid.hip);
  loop   the same panels, then 1600 back-to-back bmf_cover_count launches, one per pair (what the code could do before).

Warm chip (three untimed rounds), median of REPS timed rounds, min and max stated; the counts of the two ways are compared.  Then the
wall time of a whole SimpleThreshold.fit at the same shape, log included, beside the 29 - 30 s the reference's notebook recorded for a
300 x 500 matrix at k = 20 on a laptop (context, not a like-for-like comparison).

    python scripts/simple_threshold_times.py [out.txt]        (profiles/simple_threshold_times.txt is its output)
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
from pybmf_amd.engine import BitMatrix, _stream
from pybmf_amd.models.SimpleThreshold import SimpleThreshold, threshold_grid
from pybmf_amd.thresh_grid import ThreshGridEngine

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
REPS = 7
N_GRID = 40
out = open(sys.argv[1] if len(sys.argv) > 1 else "simple_threshold_times.txt", "w")


def say(*parts):
    line = " ".join(str(x) for x in parts)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def planted(m, n, k, seed):
    rs = np.random.RandomState(seed)
    Ub, Vb = rs.rand(m, k) < 0.08, rs.rand(n, k) < 0.05
    X = ((Ub.astype(np.float32) @ Vb.astype(np.float32).T) > 0) ^ (rs.rand(m, n) < 0.01)
    U = Ub * rs.uniform(0.3, 1.0, size=(m, k)) + 0.25 * rs.rand(m, k)   # noise up to 0.25: most grid points change some bits
    V = Vb * rs.uniform(0.3, 1.0, size=(n, k)) + 0.25 * rs.rand(n, k)
    return X.astype(np.uint8), U, V


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def measure(k):
    m, n = 6040, 3706
    X, U, V = planted(m, n, k, 2400 + k)
    B = BitMatrix(X, "cuda:0")
    eng = ThreshGridEngine({"train": B}, U, V)
    thr_u = np.repeat(threshold_grid(U, N_GRID)[:, None], k, axis=1)
    thr_v = np.repeat(threshold_grid(V, N_GRID)[:, None], k, axis=1)
    tu, tv = eng._thr(thr_u, 0), eng._thr(thr_v, 0)
    rb = torch.empty((N_GRID, B.m_pad), dtype=torch.int64, device="cuda:0")
    cb = torch.empty((N_GRID, eng.kp, B.n_pad // 32), dtype=torch.int32, device="cuda:0")
    grid_cnt = torch.zeros((N_GRID, N_GRID, 2), dtype=torch.int64, device="cuda:0")
    loop_cnt = torch.zeros((N_GRID, N_GRID, 2), dtype=torch.int64, device="cuda:0")
    st = _stream()
    words = B.n_pad // 32

    def panels():
        check(lib.bmf_thresh_panels(ptr(eng.U64[0]), B.m_pad, m, k, eng.kp, ptr(tu), N_GRID, ptr(rb), None, 0, st), "panels")
        check(lib.bmf_thresh_panels(ptr(eng.V64[0]), B.n_pad, n, k, eng.kp, ptr(tv), N_GRID, None, ptr(cb), words, st), "panels")

    def grid():
        grid_cnt.zero_()
        panels()
        check(lib.bmf_grid_cover_count(ptr(B.bits), B.m_pad, B.ldx, words, ptr(rb), None, N_GRID, ptr(cb), None, words, eng.kp, N_GRID, ptr(grid_cnt), st), "grid")

    rows = [ptr(rb[a]) for a in range(N_GRID)]
    cols = [ptr(cb[b]) for b in range(N_GRID)]
    outs = [[ptr(loop_cnt[a, b]) for b in range(N_GRID)] for a in range(N_GRID)]

    def loop():
        loop_cnt.zero_()
        panels()
        for a in range(N_GRID):
            for b in range(N_GRID):
                lib.bmf_cover_count(ptr(B.bits), B.m_pad, B.ldx, words, rows[a], cols[b], words, eng.kp, outs[a][b], None, st)

    g, l_ = timed(grid), timed(loop)
    p = timed(panels)
    same = bool((grid_cnt == loop_cnt).all().item())
    say(f"k = {k}: {m} x {n}, {B.sum_local} ones, {N_GRID} x {N_GRID} grid = {N_GRID * N_GRID} trials; device-event ms, median of {REPS} (min, max)")
    say(f"  panels alone (both factors, {N_GRID} thresholds each):        {p[0]:9.3f} ({p[1]:.3f}, {p[2]:.3f})")
    say(f"  grid: panels + one bmf_grid_cover_count:             {g[0]:9.3f} ({g[1]:.3f}, {g[2]:.3f})")
    say(f"  loop: panels + {N_GRID * N_GRID} bmf_cover_count launches:          {l_[0]:9.3f} ({l_[1]:.3f}, {l_[2]:.3f})")
    say(f"  loop / grid = {l_[0] / g[0]:.1f}; slowest grid round vs fastest loop round: {g[2]:.3f} vs {l_[1]:.3f} ms; counts equal: {same}")
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.time()
        model = SimpleThreshold(U=U, V=V, n_grid=N_GRID, seed=2024)
        model.fit(X, **QUIET)
        wall = time.time() - t0
    say(f"  SimpleThreshold(n_grid={N_GRID}).fit, upload of X, search and the {len(model.logs['updates'])}-row log: {wall:.3f} s wall "
        f"(best iter {model.best_iter}, u = {model.u:.6f}, v = {model.v:.6f})")
    return same


def main():
    say("python scripts/simple_threshold_times.py profiles/simple_threshold_times.txt")
    ok = all([measure(16), measure(64)])
    say("the reference's notebook: 'grid search with 1600 trials in total', 29 - 30 s for a 300 x 500 matrix at k = 20 (a laptop CPU; context only)")
    out.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
