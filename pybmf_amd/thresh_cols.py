"""The engine of ``BinaryMFThresholdExColumnwise``: the device state of one fit and the batched evaluation of the columnwise
thresholding objective (csrc/thresh_cols.hip, ``bmf_thresh_cols64``).

It holds the segment list of the ones of X, the workspace, the pinned result records and a pinned staging array the points are
written to (the first launch of a call copies them to the device).  ``evaluate(points, want_grad)`` fills the memo tables ``F_memo``
/ ``dF_memo``, keyed by the bytes of the point (a 2k-vector of float64: [us, vs]).
"""
from __future__ import annotations

import time

import numpy as np
import torch

from ._lib import lib, check, ptr
from .ones_list import list_fits, ones_segments


def key_of(x) -> bytes:
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


class ThreshColsEngine:
    """B: the BitMatrix of X (all rows); Ud, Vd: fp64 device factors with leading dimension `ldf`; stream_obj / stream_ptr: the
    stream every launch of the fit goes to."""

    def __init__(self, B, Ud, Vd, ldf, m, n, k, lamda, stream_obj, stream_ptr):
        self.m, self.n, self.k, self.ldf, self.lamda = int(m), int(n), int(k), int(ldf), float(lamda)
        self.Ud, self.Vd, self.stream_obj, self.stream_ptr = Ud, Vd, stream_obj, stream_ptr
        dev = B.device
        with torch.cuda.device(dev):
            free_b, _ = torch.cuda.mem_get_info(dev)
            if not list_fits(B.sum_local, free_b):
                raise NotImplementedError(f"the list of the {int(B.sum_local)} ones of X does not fit the memory budget of the trace form "
                                          "(16 bytes per one within a quarter of the free device memory, at most 4 GiB); the columnwise "
                                          "objective has no tile-product route")
            self.seg_row, self.seg_beg, self.seg_len, self.nseg, self.idx = ones_segments(B, self.m, self.n)
            if self.idx.numel() == 0:
                raise NotImplementedError("X has no ones: the trace form walks the list of the ones")
            if self.nseg > 8 * self.m + 64:
                raise NotImplementedError(f"{self.nseg} segments of ones for {self.m} rows: the workspace of the trace form holds 8 m + 64")
            self.max_points = int(lib.bmf_thresh_cols64_max_points(self.k))
            # the workspace grows with the points per call: keep it within a quarter of the free device memory, at most 2 GiB, by
            # evaluating fewer points per call (BinaryMFThreshold._setup_trace)
            budget = min(torch.cuda.mem_get_info(dev)[0] // 4, 2 << 30)
            n_work = int(lib.bmf_thresh_cols64_work(self.m, self.n, self.k, self.max_points))
            while self.max_points > 1 and n_work * 8 > budget:
                self.max_points //= 2
                n_work = int(lib.bmf_thresh_cols64_work(self.m, self.n, self.k, self.max_points))
            if n_work <= 0 or n_work * 8 > budget:
                raise NotImplementedError(f"the workspace of one point ({n_work * 8} bytes) does not fit the memory budget of the trace form "
                                          f"({budget} bytes); the columnwise objective has no tile-product route")
            self.work = torch.zeros(n_work, dtype=torch.float64, device=dev)
            self.rec = 2 + 2 * self.k
            # (pinned with the model's device current: the kernels read / write through the host pointers)
            self.out_host = torch.zeros(self.rec * self.max_points + 1, dtype=torch.float64).pin_memory()
            self.x_host = torch.zeros(2 * self.k * self.max_points, dtype=torch.float64).pin_memory()
        self.out, self.x = self.out_host.numpy(), self.x_host.numpy()
        self.seq = 0.0
        self.sum_x = float(self.idx.numel())
        self.last_hit = 8
        self.poll = True
        self.F_memo, self.dF_memo = {}, {}

    def evaluate(self, points, want_grad):
        """F (and dF) at every point of `points` (2k-vectors); fills the memo tables."""
        k2, rec = 2 * self.k, self.rec
        pts = [np.ascontiguousarray(p_, dtype=np.float64) for p_ in points]
        for a in range(0, len(pts), self.max_points):
            part = pts[a:a + self.max_points]
            npart = len(part)
            # (the previous call has delivered all its stamps, so its first launch -- the only reader of the staging array -- is over)
            self.x[: npart * k2] = np.concatenate(part)
            self.seq += 1.0
            seq, out = self.seq, self.out
            check(lib.bmf_thresh_cols64(ptr(self.seg_row), ptr(self.seg_beg), ptr(self.seg_len), self.nseg, ptr(self.idx), self.m, self.n, ptr(self.Ud),
                                        ptr(self.Vd), self.ldf, self.k, ptr(self.x_host), npart, self.lamda, self.sum_x, int(want_grad), ptr(self.work),
                                        ptr(self.out_host), seq, self.stream_ptr), "bmf_thresh_cols64")
            # every record's word 0 and the word after the last record carry this call's sequence number, each written behind the values
            # it vouches for: wait for ALL of them (bounded), else for the stream
            if self.poll:
                stamps = out[0:rec * npart + 1:rec]
                deadline = time.perf_counter() + 0.002
                while not (stamps == seq).all():
                    if time.perf_counter() > deadline:
                        self.stream_obj.synchronize()
                        break
            else:
                self.stream_obj.synchronize()
            for i, p_ in enumerate(part):
                key = p_.tobytes()
                self.F_memo[key] = float(0.5 * out[rec * i + 1])
                if want_grad:
                    self.dF_memo[key] = out[rec * i + 2: rec * (i + 1)].copy()
