"""Timing of the coordinate-descent NMF path (NMFSklearn) on one MI355X at the benchmark's planted 100 000 x 20 000, k = 64: the time
of one CD iteration (bmf_nmf_cd_iterate, two sweeps), device-event means of its kernels called one by one (the sweep also through
bmf_timer_*, which brackets the two sweep launches inside the iteration), the NNDSVD initialisation split into the products on the
device and the LAPACK calls on the host, and the wall time of a whole fit.  For scale: the headline multiplicative-update step is
2 x 209 us of bits GEMM and 2 x 40 us of epilogue (profiles/r05_kernel_stats_headline.csv).

    python scripts/nmf_times.py [out.txt] [m n k]        (profiles/nmf_times.txt is its output)
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pybmf_amd._lib import check, lib, ptr
from pybmf_amd.engine import BitMatrix, _stream
from pybmf_amd.generators import PlantedBooleanOnDevice
from pybmf_amd.models.NMFSklearn import nndsvd_init
from pybmf_amd.nmf import NMFEngine

out = open(sys.argv[1] if len(sys.argv) > 1 else "nmf_times.txt", "w")
m, n, k = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (100000, 20000, 64)
CMD = "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:])   # the command as it was run


def say(*parts):
    line = " ".join(str(x) for x in parts) + "   [" + CMD + "]"
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def mean_us(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


dens = 0.067 if k >= 32 else 0.2
t0 = time.time()
X = BitMatrix(PlantedBooleanOnDevice(m, n, k, density=(dens, dens), seed=1000, noise=(0.05, 0.01), noise_seed=2000), "cuda:0")
eng = NMFEngine(X, k)
torch.cuda.synchronize()
say(f"matrix {m} x {n}, k = {k} (kp = {eng.kp}), ones {X.sum_local}: generated, packed and tiled in {time.time() - t0:.2f} s")

# ---- NNDSVD: the products on the device against the rest (LU, QR, the small SVD, the NNDSVD loop: host, fp64) ----
spent = {"device": 0.0, "calls": 0}


def product(T, transposed=False):
    t = time.time()
    R = eng.product(T, transposed)
    spent["device"] += time.time() - t
    spent["calls"] += 1
    return R


t0 = time.time()
W0, H0 = nndsvd_init((m, n), X.sum_local / (float(m) * n), k, "nndsvd", np.random.RandomState(2024), product)
t_init = time.time() - t0
say(f"NNDSVD init: {t_init:.2f} s wall = {spent['device']:.2f} s in {spent['calls']} products with X / X^T of {k + 10} columns (upload, digit planes, "
    f"bits GEMM, slab sum, download) + {t_init - spent['device']:.2f} s of host LAPACK and NumPy")

# ---- the CD iteration ----
eng.load_factors(W0, np.ascontiguousarray(H0.T))
check(lib.bmf_timer_enable(256))
t0 = time.time()
rows = []
for it in range(30):
    eng.iterate(it)
    rows.append(sum(eng.row(it)))
wall30 = time.time() - t0
launches, total_ms = C.c_int(0), C.c_double(0.0)
check(lib.bmf_timer_read(C.byref(launches), C.byref(total_ms)))
check(lib.bmf_timer_disable())
say(f"30 CD iterations, violations read every iteration: {wall30 * 1e3 / 30:.3f} ms per iteration (wall); violation ratio after 30: {rows[-1] / rows[0]:.3g}")
both_us = total_ms.value * 1e3 / max(launches.value, 1)
say(f"bmf_nmf_cd_sweep inside the iteration (bmf_timer_*, {launches.value} launches, U and V sweeps mixed): {both_us:.1f} us mean")
# every second bracketed launch is a U sweep: bmf_timer_stride(2) times those alone, and the V sweeps follow from the mixed mean
check(lib.bmf_timer_enable(256))
check(lib.bmf_timer_stride(2))
for it in range(30, 60):
    eng.iterate(it)
    eng.row(it)
check(lib.bmf_timer_read(C.byref(launches), C.byref(total_ms)))
check(lib.bmf_timer_disable())
u_us = total_ms.value * 1e3 / max(launches.value, 1)
say(f"  of which the U sweeps ({launches.value} launches of 30 further iterations, bmf_timer_stride(2)): {u_us:.1f} us mean; the V sweeps, as "
    f"2 x mixed - U: {2 * both_us - u_us:.1f} us.  Inside the iteration a sweep finds its numerator slabs and its factor in HBM or the "
    f"last-level cache as the GEMM left them; the stand-alone figures below repeat one launch over the same buffers")
it_us = mean_us(lambda: check(lib.bmf_nmf_cd_iterate(C.byref(eng._st), 0, _stream())), reps=10)
say(f"bmf_nmf_cd_iterate back to back, no host read: {it_us:.1f} us per iteration")

kp, kk, st = eng.kp, eng.kp * eng.kp, _stream()
for side, F64, F, rows_pad, rws, held, held_pad, tiled, panel, scale, slab, splits, G64, ws, part in (
        ("U", eng.U64, eng.U, X.m_pad, X.m, eng.V, X.n_pad, eng._tiled[0], eng.Vpanel, eng.scaleV, eng.Mslab, eng.splits_xv, eng.GV64, eng.wsU, eng.partU),
        ("V", eng.V64, eng.V, X.n_pad, X.n, eng.U, X.m_pad, eng._tiled[1], eng.Upanel, eng.scaleU, eng.Nslab, eng.splits_xtu, eng.GU64, eng.wsV, eng.partV)):
    keep = F64.clone()
    g = mean_us(lambda: (check(lib.bmf_gram_partial(ptr(held), held_pad, kp, kp, ptr(eng.gram_slabs), eng.gram_blocks, st)),
                         check(lib.bmf_reduce_slabs(ptr(eng.gram_slabs), kk, eng.gram_blocks, kk, ptr(eng.GU), ptr(G64), st))))
    x = mean_us(lambda: check(lib.bmf_xf_bits_i8(ptr(tiled), rows_pad, held_pad // 32, held_pad // 32, ptr(panel), held_pad, 3, ptr(scale[kp:]), kp,
                                                 ptr(slab), rows_pad * kp, splits, 1, st)))
    s = mean_us(lambda: check(lib.bmf_nmf_cd_sweep(ptr(F64), ptr(F), rows_pad, rws, k, kp, ptr(slab), rows_pad * kp, splits, ptr(G64), ptr(ws), ptr(part), st)))
    F64.copy_(keep)
    F.copy_(F64)
    own_panel, own_scale = (eng.Upanel, eng.scaleU) if side == "U" else (eng.Vpanel, eng.scaleV)
    p = mean_us(lambda: check(lib.bmf_make_panel_i8(ptr(F64), ptr(F), rows_pad, kp, kp, 3, ptr(own_panel), rows_pad, ptr(ws), ptr(own_scale), st)))
    say(f"{side} half ({rows_pad} rows, {splits} numerator slab(s)): Gram + slab sum {g:.1f} us, bits GEMM {x:.1f} us, sweep {s:.1f} us, digit planes "
        f"(stand-alone builder, with its own maxima pass) {p:.1f} us")
    say(f"  sweep against the GEMM it follows: {s / x:.2f} x" + ("  -- the sweep costs MORE than its GEMM" if s > x else ""))

# ---- a whole fit: init + load + iterations to tol = 1e-4 (at most 200) ----
torch.cuda.synchronize()
t0 = time.time()
W0, H0 = nndsvd_init((m, n), X.sum_local / (float(m) * n), k, "nndsvd", np.random.RandomState(2024), eng.product)
eng.load_factors(W0, np.ascontiguousarray(H0.T))
n_iter, first = 0, None
for it in range(200):
    eng.iterate(it)
    v = sum(eng.row(it))
    n_iter = it + 1
    first = v if it == 0 else first
    if first == 0 or v / first <= 1e-4:
        break
U, V = eng.factors()
err = eng.rec_error()
say(f"whole fit (NNDSVD init, {n_iter} iterations to ratio {v / first:.3g}, factors to the host, rec_error): {time.time() - t0:.2f} s wall; "
    f"||X - U V^T||_F = {np.sqrt(max(err, 0)):.2f}")
out.close()
