"""Cost model of the cover kernels (C3 shape): the full count vs. the number of set factor bits per row, then the incremental count
(bmf_cover_delta) in both orientations from all words changed to none."""
import ctypes as C
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from pybmf_amd import _lib as L

d = torch.device("cuda:0")
m_pad, n_pad, kp = 100352, 20480, 64
ldx = n_pad // 32
X = torch.randint(-2**31, 2**31 - 1, (m_pad, ldx), dtype=torch.int32, device=d)
vcol = torch.randint(-2**31, 2**31 - 1, (kp, ldx), dtype=torch.int32, device=d)
counts = torch.zeros(4, dtype=torch.int64, device=d)
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rs = np.random.RandomState(0)
for p in (0, 1, 2, 4, 8, 16, 32, 64):
    u = np.zeros(m_pad, np.uint64)
    for _ in range(p):
        pass
    bits = np.zeros((m_pad, 64), np.uint8)
    if p:
        idx = np.argsort(rs.rand(m_pad, 64), axis=1)[:, :p]
        np.put_along_axis(bits, idx, 1, axis=1)
    u = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).ravel()
    ud = torch.from_numpy(u.view(np.int64)).to(d)
    for _ in range(2):
        L.check(L.lib.bmf_cover_count(L.ptr(X), m_pad, ldx, ldx, L.ptr(ud), L.ptr(vcol), ldx, kp, L.ptr(counts), None, s))
    torch.cuda.synchronize()
    if os.environ.get("COLD"):   # every launch after 512 MiB of other traffic: X comes from HBM, as in the iteration loop
        flush = torch.zeros(512 << 20, dtype=torch.uint8, device=d)
        ts = []
        for _ in range(10):
            flush_sum = flush.view(torch.int32).sum()   # a READ of 512 MiB: evicts X without leaving dirty lines behind
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(L.lib.bmf_cover_count(L.ptr(X), m_pad, ldx, ldx, L.ptr(ud), L.ptr(vcol), ldx, kp, L.ptr(counts), None, s))
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        print(f"popc={p:2d}: {sorted(ts)[len(ts) // 2]:8.1f} us (cold)")
        continue
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        L.check(L.lib.bmf_cover_count(L.ptr(X), m_pad, ldx, ldx, L.ptr(ud), L.ptr(vcol), ldx, kp, L.ptr(counts), None, s))
    e1.record()
    torch.cuda.synchronize()
    print(f"popc={p:2d}: {e0.elapsed_time(e1) / 10 * 1e3:8.1f} us")

# ---- the incremental count (bmf_cover_delta): the price of an iteration in which every word changed, and the floor of one in which
# none did, in both orientations of the headline shape, against the full count above (popc = p set bits in the new AND the old word)
def timed(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def words_with(rows, p, seed):
    bits = np.zeros((rows, 64), np.uint8)
    idx = np.argsort(np.random.RandomState(seed).rand(rows, 64), axis=1)[:, :p]
    np.put_along_axis(bits, idx, 1, axis=1)
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).ravel()


XT = torch.randint(-2**31, 2**31 - 1, (n_pad, m_pad // 32), dtype=torch.int32, device=d)
ucol = torch.randint(-2**31, 2**31 - 1, (kp, m_pad // 32), dtype=torch.int32, device=d)
for p in (4, 8):
    for name, bits_, rows, words, col in (("rows (X, U words)", X, m_pad, ldx, vcol), ("columns (X^T, V words)", XT, n_pad, m_pad // 32, ucol)):
        new_h, old_h = words_with(rows, p, 1), words_with(rows, p, 2)
        old_h[new_h == old_h] ^= np.uint64(1)
        new = torch.from_numpy(new_h.view(np.int64)).to(d)
        old = torch.from_numpy(old_h.view(np.int64)).to(d)
        other = torch.zeros(max(m_pad, n_pad), dtype=torch.int64, device=d)
        other_prev = torch.zeros_like(other)
        flip = torch.from_numpy((new_h ^ (np.uint64(1) << np.random.RandomState(4).randint(0, 64, rows).astype(np.uint64))).view(np.int64)).to(d)
        for label, prev, frac in (("all dirty", old, 1.0), ("all, 1 bit", flip, 1.0), ("none dirty", new, 0.0)):
            t = timed(lambda: L.check(L.lib.bmf_cover_delta(L.ptr(bits_), words, words, rows, L.ptr(new), L.ptr(prev), L.ptr(col), words, kp, L.ptr(counts),
                                                            L.ptr(other), L.ptr(other_prev), (n_pad if rows == m_pad else m_pad), None, s)))
            print(f"delta popc={p}: {name:24s} {label:10s} {t:8.1f} us")
        for frac in (0.003, 0.05, 0.25):
            prev_h = new_h.copy()
            sel = np.random.RandomState(3).rand(rows) < frac
            prev_h[sel] = old_h[sel]
            prev = torch.from_numpy(prev_h.view(np.int64)).to(d)
            t = timed(lambda: L.check(L.lib.bmf_cover_delta(L.ptr(bits_), words, words, rows, L.ptr(new), L.ptr(prev), L.ptr(col), words, kp, L.ptr(counts),
                                                            L.ptr(other), L.ptr(other_prev), (n_pad if rows == m_pad else m_pad), None, s)))
            print(f"delta popc={p}: {name:24s} {frac:10.3f} {t:8.1f} us")
    if p == 4:
        full = torch.from_numpy(words_with(m_pad, p, 1).view(np.int64)).to(d)
        print(f"full  popc={p}: {timed(lambda: L.check(L.lib.bmf_cover_count(L.ptr(X), m_pad, ldx, ldx, L.ptr(full), L.ptr(vcol), ldx, kp, L.ptr(counts), None, s))):8.1f} us")
