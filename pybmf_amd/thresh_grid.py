"""The engine of ``SimpleThreshold``: the Boolean cover counts of many threshold pairs (u, v) on fixed real factors U, V.

The fp64 factors sit on the device as blocks of up to 64 columns (one block for k <= 64, two for 64 < k <= 128: the convention of
``blocks.py``).  ``bmf_thresh_panels`` turns a block and T threshold vectors into T bit panels -- the k-bit word of every row of U,
the bit-columns of V -- and ``bmf_grid_cover_count`` / ``bmf_pairs_cover_count`` (csrc/thresh_grid.hip) count TP / FP of panel pairs
against the bits of every data set.  One chain of launches per search, one read-back of the counters at its end.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .engine import _stream

BK = 64            # columns of a block
MAX_K = 2 * BK


def plan(rows_pad: int, words: int, panels: int):
    """(chunk_words, rows_per_block, a_batch) of the cover kernels at this shape (host arithmetic, no GPU)."""
    cw, rpb, ab = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib.bmf_grid_cover_plan(rows_pad, words, panels, C.byref(cw), C.byref(rpb), C.byref(ab)), "bmf_grid_cover_plan")
    return cw.value, rpb.value, ab.value


class ThreshGridEngine:
    """``sets``: {'train': BitMatrix, 'val': ..., 'test': ...} of one shape; U (m x k), V (n x k) host arrays, k <= 128."""

    def __init__(self, sets, U, V):
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        self.sets = dict(sets)
        B = self.sets["train"]
        self.m, self.n, self.m_pad, self.n_pad, self.device = B.m, B.n, B.m_pad, B.n_pad, B.device
        self.k = int(U.shape[1])
        if not (1 <= self.k <= MAX_K) or U.shape != (self.m, self.k) or V.shape != (self.n, self.k):
            raise ValueError(f"factors of shape {U.shape}, {V.shape} for a {self.m} x {self.n} matrix (k <= {MAX_K})")
        for S in self.sets.values():
            assert (S.m, S.n, S.m_pad, S.n_pad) == (self.m, self.n, self.m_pad, self.n_pad)
        self.nb = 1 if self.k <= BK else 2
        self.kp = 32 if self.k <= 32 else BK
        self.kb = [min(BK, self.k - BK * b) for b in range(self.nb)]   # real columns of each block
        self.sums = {name: int(S.sum_local) for name, S in self.sets.items()}
        with torch.cuda.device(self.device):
            self.U64, self.V64 = self._upload(U, self.m_pad), self._upload(V, self.n_pad)

    def _upload(self, F, rows_pad):
        out = []
        for b in range(self.nb):
            t = torch.zeros((rows_pad, self.kp), dtype=torch.float64, device=self.device)
            t[: F.shape[0], : self.kb[b]] = torch.from_numpy(np.ascontiguousarray(F[:, BK * b: BK * b + self.kb[b]])).to(self.device)
            out.append(t)
        return out

    # ---- panels ---------------------------------------------------------------------------------------------------------------
    def _thr(self, thr, b):
        """Columns of block b of the (T, k) threshold vectors, on the device."""
        thr = np.asarray(thr, dtype=np.float64)
        assert thr.ndim == 2 and thr.shape[1] == self.k and thr.shape[0] >= 1, thr.shape
        return torch.from_numpy(np.ascontiguousarray(thr[:, BK * b: BK * b + self.kb[b]])).to(self.device)

    def row_panels(self, thr):
        """Per block: int64 [T][m_pad], the k-bit words of the rows of U under each threshold vector."""
        out = []
        for b in range(self.nb):
            t = self._thr(thr, b)
            rb = torch.empty((t.shape[0], self.m_pad), dtype=torch.int64, device=self.device)
            check(lib.bmf_thresh_panels(ptr(self.U64[b]), self.m_pad, self.m, self.kb[b], self.kp, ptr(t), t.shape[0], ptr(rb), None, 0, _stream()),
                  "bmf_thresh_panels")
            out.append(rb)
        return out

    def col_panels(self, thr):
        """Per block: int32 [T][kp][n_pad / 32], the bit-columns of V under each threshold vector."""
        out = []
        for b in range(self.nb):
            t = self._thr(thr, b)
            cb = torch.empty((t.shape[0], self.kp, self.n_pad // 32), dtype=torch.int32, device=self.device)
            check(lib.bmf_thresh_panels(ptr(self.V64[b]), self.n_pad, self.n, self.kb[b], self.kp, ptr(t), t.shape[0], None, ptr(cb), self.n_pad // 32,
                                        _stream()), "bmf_thresh_panels")
            out.append(cb)
        return out

    # ---- counts ---------------------------------------------------------------------------------------------------------------
    def _args(self, S, rb, cb):
        second = (ptr(rb[1]), ptr(cb[1])) if self.nb == 2 else (None, None)
        return (ptr(S.bits), S.m_pad, S.ldx, S.n_pad // 32, ptr(rb[0]), second[0], rb[0].shape[0], ptr(cb[0]), second[1], S.n_pad // 32, self.kp,
                cb[0].shape[0])

    def grid_counts(self, thr_u, thr_v):
        """{set: int64 [A][B][2]} -- TP, FP of every pair (thr_u[a], thr_v[b]).  The vectors of `thr_u` must ascend in every column
        (the nesting the grid kernel walks)."""
        thr_u = np.asarray(thr_u, dtype=np.float64)
        assert (np.diff(thr_u, axis=0) >= 0).all(), "the grid kernel takes ascending thresholds"
        with torch.cuda.device(self.device):
            rb, cb = self.row_panels(thr_u), self.col_panels(thr_v)
            out = {}
            for name, S in self.sets.items():
                cnt = torch.zeros((rb[0].shape[0], cb[0].shape[0], 2), dtype=torch.int64, device=self.device)
                a = self._args(S, rb, cb)
                check(lib.bmf_grid_cover_count(*a, ptr(cnt), _stream()), "bmf_grid_cover_count")
                out[name] = cnt
            return {name: c.cpu().numpy() for name, c in out.items()}

    def pair_counts(self, thr_u, thr_v, pairs):
        """{set: int64 [T][2]} -- TP, FP of the pairs (thr_u[pairs[t][0]], thr_v[pairs[t][1]]); no order is assumed."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        assert pairs.ndim == 2 and pairs.shape[1] == 2 and pairs.shape[0] >= 1
        assert pairs.min() >= 0 and pairs[:, 0].max() < len(thr_u) and pairs[:, 1].max() < len(thr_v)
        with torch.cuda.device(self.device):
            rb, cb = self.row_panels(thr_u), self.col_panels(thr_v)
            pd = torch.from_numpy(pairs).to(self.device)
            out = {}
            for name, S in self.sets.items():
                cnt = torch.zeros((pairs.shape[0], 2), dtype=torch.int64, device=self.device)
                check(lib.bmf_pairs_cover_count(*self._args(S, rb, cb), ptr(pd), pairs.shape[0], ptr(cnt), _stream()), "bmf_pairs_cover_count")
                out[name] = cnt
            return {name: c.cpu().numpy() for name, c in out.items()}
