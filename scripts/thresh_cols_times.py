"""Timing of the columnwise thresholding objective (bmf_thresh_cols64, csrc/thresh_cols.hip) beside the scalar one (bmf_thresh_trace64,
csrc/thresh_trace.hip) on one MI355X at 6040 x 3706 with MovieLens-1M's number of ones (a stand-in with heavy-tailed row and column
sums), k = 16 and k = 64: one chain of max_points F evaluations (what a Wolfe search announces) and one F + dF evaluation (what every
outer iteration adds), both entry points at the same shape and batch, enqueued without a host read and bracketed by device events.
Warm chip (three untimed rounds), median of REPS timed rounds, min and max stated.  The columnwise results at constant vectors are
compared with the scalar ones.

    python scripts/thresh_cols_times.py [out.txt]        (profiles/thresh_cols_times.txt is its output)
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pybmf_amd._lib import check, lib, ptr

REPS = 7
out = open(sys.argv[1] if len(sys.argv) > 1 else "thresh_cols_times.txt", "w")


def say(*parts):
    line = " ".join(str(x) for x in parts)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def stand_in():
    rs = np.random.RandomState(11)
    m, n = 6040, 3706
    pu, pv = rs.pareto(1.2, m) + 1, rs.pareto(1.2, n) + 1
    P = np.outer(pu / pu.sum(), pv / pv.sum())
    s = 1_000_209.0
    for _ in range(60):
        s *= 1_000_209.0 / np.minimum(P * s, 1.0).sum()
    return (rs.rand(m, n) < np.minimum(P * s, 1.0)).astype(np.uint8)


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
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def segments(X):
    m = X.shape[0]
    rows, cols = np.nonzero(X)
    counts = np.bincount(rows, minlength=m)
    nseg_row = (counts + 127) // 128
    seg_row = np.repeat(np.arange(m), nseg_row)
    first = np.cumsum(nseg_row) - nseg_row
    within = np.arange(seg_row.size) - first[seg_row]
    seg_beg = (np.cumsum(counts) - counts)[seg_row] + 128 * within
    seg_len = np.minimum(counts[seg_row] - 128 * within, 128)
    o = np.argsort(-seg_len, kind="stable")
    return dev(seg_row[o].astype(np.int32)), dev(seg_beg[o].astype(np.int64)), dev(seg_len[o].astype(np.int32)), int(seg_row.size), dev(cols.astype(np.int32)), float(rows.size)


def measure(X, k):
    m, n = X.shape
    rs = np.random.RandomState(k)
    ld = 32 if k <= 32 else 64
    Ud, Vd = torch.zeros((m, ld), dtype=torch.float64, device="cuda"), torch.zeros((n, ld), dtype=torch.float64, device="cuda")
    Ud[:, :k], Vd[:, :k] = dev(rs.rand(m, k)), dev(rs.rand(n, k))
    seg_row, seg_beg, seg_len, nseg, idx, sx = segments(X)
    maxp = int(lib.bmf_thresh_cols64_max_points(k))
    assert maxp == int(lib.bmf_thresh_trace64_max_pairs(k))
    w_cols, w_trace = int(lib.bmf_thresh_cols64_work(m, n, k, maxp)), int(lib.bmf_thresh_trace64_work(m, n, k, maxp))
    work_c, work_t = torch.zeros(w_cols, dtype=torch.float64, device="cuda"), torch.zeros(w_trace, dtype=torch.float64, device="cuda")
    rec = 2 + 2 * k
    out_c, out_t = torch.zeros(rec * maxp + 1, dtype=torch.float64).pin_memory(), torch.zeros(4 * maxp + 1, dtype=torch.float64).pin_memory()
    say(f"k = {k}: {m} x {n}, {int(sx)} ones in {nseg} segments, {maxp} points per call; workspace {w_cols * 8 / 2 ** 20:.0f} MiB columnwise, "
        f"{w_trace * 8 / 2 ** 20:.0f} MiB scalar; device-event us, median of {REPS} (min, max)")
    seq = [0.0]
    worst_f = worst_g = 0.0
    for points, grad, what in ((maxp, 0, f"one chain of {maxp} F evaluations"), (1, 1, "one F + dF evaluation      ")):
        uv = [(0.45 + 0.01 * i, 0.55 - 0.01 * i) for i in range(points)]
        flat = (C.c_double * (2 * points))(*[x for p_ in uv for x in p_])
        xd = dev(np.array([np.concatenate([np.full(k, u), np.full(k, v)]) for u, v in uv]))

        def cols():
            seq[0] += 1.0
            check(lib.bmf_thresh_cols64(ptr(seg_row), ptr(seg_beg), ptr(seg_len), nseg, ptr(idx), m, n, ptr(Ud), ptr(Vd), ld, k, ptr(xd), points, 10.0, sx,
                                        grad, ptr(work_c), ptr(out_c), seq[0], stream()), "bmf_thresh_cols64")

        def trace():
            seq[0] += 1.0
            check(lib.bmf_thresh_trace64(ptr(seg_row), ptr(seg_beg), ptr(seg_len), nseg, ptr(idx), m, n, ptr(Ud), ptr(Vd), ld, k, flat, points, 10.0, sx,
                                         grad, ptr(work_t), ptr(out_t), seq[0], stream()), "bmf_thresh_trace64")
        c, t = timed(cols), timed(trace)
        torch.cuda.synchronize()
        oc, ot = out_c.numpy(), out_t.numpy()
        for i in range(points):
            worst_f = max(worst_f, abs(oc[rec * i + 1] / ot[4 * i + 1] - 1))
            if grad:
                scale = max(abs(ot[4 * i + 2]), abs(ot[4 * i + 3])) + 1.0
                worst_g = max(worst_g, abs(oc[rec * i + 2: rec * i + 2 + k].sum() - ot[4 * i + 2]) / scale,
                              abs(oc[rec * i + 2 + k: rec * (i + 1)].sum() - ot[4 * i + 3]) / scale)
        say(f"  {what}: columnwise {c[0]:8.1f} ({c[1]:.1f}, {c[2]:.1f})   scalar {t[0]:8.1f} ({t[1]:.1f}, {t[2]:.1f})   columnwise / scalar = {c[0] / t[0]:.2f}")
    say(f"  constant vectors against the scalar kernel: 2 F differs by {worst_f:.1e} relative, the summed gradient halves by {worst_g:.1e} of the scale")
    return worst_f <= 1e-11 and worst_g <= 1e-9


def main():
    say("python scripts/thresh_cols_times.py profiles/thresh_cols_times.txt")
    X = stand_in()
    ok = all([measure(X, 16), measure(X, 64)])
    out.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
