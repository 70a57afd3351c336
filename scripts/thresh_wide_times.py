"""Timing of the thresholding objective at a rank above 64 (csrc/thresh_wide.hip) beside the k = 64 entry points, on one MI355X, at
6040 x 3706 with the density of the benchmark's MovieLens-1M stand-in (bench.py, secondary_c5): device-event medians (3 warm-up calls,
50 timed) of one F batch and one F + dF batch of the trace form -- k = 64 through bmf_thresh_trace64, k = 128 through
bmf_thresh_trace_wide, in the same process, at max_pairs pairs and at one pair --, of one evaluation over a list of observed cells
(10 % of the cells: two transforms + the cell pass) at both ranks, and the wall time of a whole fit of golden g33 case b (150 x 140,
k = 128).  Random fp64 factors in (0, 1), lamda = 10, thresholds around 0.5.  No gate: the wide rank is a correctness row.

    python scripts/thresh_wide_times.py [out.txt]        (profiles/thresh_wide_times.txt is its output)
"""
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pybmf_amd._lib import check, lib, ptr
from pybmf_amd.engine import SparseObs

out = open(sys.argv[1] if len(sys.argv) > 1 else "thresh_wide_times.txt", "w")


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


def median_us(fn, reps=50):
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
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[-1 - len(ts) // 10]


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


def trace_times(X, k, wide):
    m, n = X.shape
    rs = np.random.RandomState(k)
    ld = 128 if wide else 64
    Ud, Vd = torch.zeros((m, ld), dtype=torch.float64, device="cuda"), torch.zeros((n, ld), dtype=torch.float64, device="cuda")
    Ud[:, :k], Vd[:, :k] = dev(rs.rand(m, k)), dev(rs.rand(n, k))
    seg_row, seg_beg, seg_len, nseg, idx, sx = segments(X)
    entry, name = (lib.bmf_thresh_trace_wide, "bmf_thresh_trace_wide") if wide else (lib.bmf_thresh_trace64, "bmf_thresh_trace64")
    maxp = int((lib.bmf_thresh_trace_wide_max_pairs if wide else lib.bmf_thresh_trace64_max_pairs)(k))
    n_work = int((lib.bmf_thresh_trace_wide_work if wide else lib.bmf_thresh_trace64_work)(m, n, k, maxp))
    work = torch.zeros(n_work, dtype=torch.float64, device="cuda")
    out_host = torch.zeros(4 * maxp + 1, dtype=torch.float64).pin_memory()
    seq = [0.0]
    say(f"{name}: k = {k}, {nseg} segments of {int(sx)} ones, max_pairs = {maxp}, workspace {n_work * 8 / 2 ** 20:.0f} MiB")
    for pairs in (maxp, 1):
        pts = [(0.45 + 0.01 * i, 0.55 - 0.01 * i) for i in range(pairs)]
        uv = (C.c_double * (2 * pairs))(*[x for p_ in pts for x in p_])
        for grad in (0, 1):
            def call():
                seq[0] += 1.0
                check(entry(ptr(seg_row), ptr(seg_beg), ptr(seg_len), nseg, ptr(idx), m, n, ptr(Ud), ptr(Vd), ld, k, uv, pairs, 10.0, sx, grad, ptr(work),
                            ptr(out_host), seq[0], stream()), name)
            med, lo, hi = median_us(call)
            say(f"  {'F + dF' if grad else 'F     '} batch of {pairs} pair(s): median {med:8.1f} us (10th .. 90th percentile {lo:.1f} .. {hi:.1f}), {med / pairs:8.1f} us per pair")
    return out_host.numpy()[1]


def masked_times(obs, m, n, k, wide):
    rs = np.random.RandomState(k)
    kp = 128 if wide else 64
    Ud, Vd = torch.zeros((m, kp), dtype=torch.float64, device="cuda"), torch.zeros((n, kp), dtype=torch.float64, device="cuda")
    Ud[:, :k], Vd[:, :k] = dev(rs.rand(m, k)), dev(rs.rand(n, k))
    Us, dUs, Vs, dVs = (torch.zeros_like(Ud), torch.zeros_like(Ud), torch.zeros_like(Vd), torch.zeros_like(Vd))
    blocks = 1024
    partial, res = torch.zeros(4 * blocks, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    ls = obs.csr
    for grad in (0, 1):
        def call():
            s = stream()
            dU, dV = (ptr(dUs), ptr(dVs)) if grad else (None, None)
            if wide:
                check(lib.bmf_thresh_transform64_wide(ptr(Ud), m, m, k, 0.5, 10.0, ptr(Us), dU, s))
                check(lib.bmf_thresh_transform64_wide(ptr(Vd), n, n, k, 0.5, 10.0, ptr(Vs), dV, s))
                check(lib.bmf_masked_thresh64_wide(ptr(ls["ptr"]), ptr(ls["idx"]), ptr(ls["val"]), None, ptr(ls["seg_row"]), ptr(ls["seg_beg"]), ls["nseg"],
                                                   ptr(Us), dU, ptr(Vs), dV, k, ptr(partial), blocks, ptr(res), s))
            else:
                check(lib.bmf_thresh_transform64(ptr(Ud), m, m, k, kp, 0.5, 10.0, ptr(Us), dU, s))
                check(lib.bmf_thresh_transform64(ptr(Vd), n, n, k, kp, 0.5, 10.0, ptr(Vs), dV, s))
                check(lib.bmf_masked_thresh64_k(ptr(ls["ptr"]), ptr(ls["idx"]), ptr(ls["val"]), None, ptr(ls["seg_row"]), ptr(ls["seg_beg"]), ls["nseg"],
                                                ptr(Us), dU, ptr(Vs), dV, kp, k, ptr(partial), blocks, ptr(res), s))
        med, lo, hi = median_us(call)
        say(f"  k = {k:3d} {'F + dF' if grad else 'F     '} over {obs.nnz} observed cells ({ls['nseg']} segments): median {med:8.1f} us "
            f"(10th .. 90th percentile {lo:.1f} .. {hi:.1f})")


def main():
    say("device:", torch.cuda.get_device_name(0))
    X = stand_in()
    m, n = X.shape
    say(f"matrix: {m} x {n}, {int(X.sum())} ones (power-law row / column popularity, the benchmark's MovieLens-1M stand-in)")
    say("trace form (W = 'full'), device-event medians of one call:")
    trace_times(X, 64, False)
    trace_times(X, 128, True)
    say("observed cells (W = 'mask'), two transforms + the cell pass:")
    rs = np.random.RandomState(3)
    r, c = np.nonzero(rs.rand(m, n) < 0.1)
    obs = SparseObs(r, c, X[r, c].astype(np.float64), None, (m, n))
    masked_times(obs, m, n, 64, False)
    masked_times(obs, m, n, 128, True)
    # a whole fit of golden g33 case b
    from pybmf_amd.models import BinaryMFThreshold
    here = os.path.join(ROOT, "tests", "golden")
    z, meta = np.load(os.path.join(here, "g33_threshold_wide.npz")), json.load(open(os.path.join(here, "g33_threshold_wide.json")))
    Xb = np.unpackbits(z["b_X_bits"], axis=1, bitorder="little")[:, : z["b_shape"][1]]
    ts = []
    for _ in range(3):
        with contextlib.redirect_stdout(io.StringIO()):
            mdl = BinaryMFThreshold(k=128, U=z["b_U"].copy(), V=z["b_V"].copy(), W="full", u=0.5, v=0.5, lamda=100, min_diff=1e-3, max_iter=100)
            t0 = time.perf_counter()
            mdl.fit(Xb, task="reconstruction", show_logs=False, show_result=False, save_model=False)
            ts.append(time.perf_counter() - t0)
    say(f"whole fit of golden g33 case b (150 x 140, k = 128, lamda = 100, {len(mdl.logs['updates'])} log rows, reference: "
        f"{len(meta['b']['lam100']['rows']['rows'])}): wall {', '.join(f'{t * 1e3:.0f}' for t in ts)} ms (first call includes set-up)")


if __name__ == "__main__":
    main()
