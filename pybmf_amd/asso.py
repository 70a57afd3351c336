"""Device state of an Asso fit (``PyBMF/models/Asso.py``): the bits of X (row-major and transposed, ``BitMatrix``), of the prediction
X_pd and of the candidate basis rows, and the sweep over the candidates on them (csrc/asso.hip).

    n_cand = eng.build_basis(tau)                 candidate rows from the column associations; empty rows are no candidates
    hit = eng.best(best_score, w_fp, w_fn)        one sweep of the reference's loop over the remaining candidates:
                                                  (position in the list, candidate, score, T, F) or None
    u, v = eng.column(cand)                       the winner's column vector and basis row as packed uint32 words
    eng.apply(u, v); eng.remove(cand)             X_pd |= u x v; the candidate leaves the list
    eng.counts("train"), eng.row_counts(), eng.prediction(), eng.factor_arrays(), eng.truncate(k)

A sweep keeps the candidate with the LARGEST score above best_score, the first of equals (the reference replaces its best on every
strict improvement).  best() launches over blocks of the remaining list and carries the running best score from block to block, so
`block` is a speed knob only: every value gives the same result.  The host reads one record per launch.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine
from .engine import BitMatrix

WORK_BYTES = 64 << 20   # default ceiling of the (row tile, candidate) partial sums of one launch


class AssoEngine(BitSetEngine):
    title = "Asso"

    def __init__(self, bits: BitMatrix, extra: dict = None):
        super().__init__(bits, extra)
        dev = self.device
        self.ldx, self.W = bits.ldx, bits.ldxt
        self._tiles = -(-self.m // 64)
        # candidates per launch: all of them while the partial sums stay within WORK_BYTES, never fewer than 64
        self._max_block = max(64, min(self.n, WORK_BYTES // (16 * self._tiles)))
        n_work = int(lib.bmf_asso_score_work(self.m, self._max_block))
        with torch.cuda.device(dev):
            # X and X^T are in HBM already (BitMatrix); the prediction and the candidate rows add two row-major bit matrices
            self._require_free((bits.m_pad + self.n) * self.ldx * 4 + n_work + 16 * self.m + 40 * self.n,
                               "the bits of the prediction and of the candidates and the partial sums take", "; row sharding is not built")
            self.pd = torch.zeros_like(bits.bits)
            self.basis = torch.zeros((self.n, self.ldx), dtype=torch.int32, device=dev)
            self._count = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self._cand = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self._rows = torch.zeros(2 * self.m, dtype=torch.int32, device=dev)          # [TP_old | FP_old] per row
            self._work = torch.empty(n_work // 8 + 1, dtype=torch.int64, device=dev)
            self._T = torch.zeros(self.n, dtype=torch.int64, device=dev)
            self._F = torch.zeros(self.n, dtype=torch.int64, device=dev)
            self._score = torch.zeros(self.n, dtype=torch.float64, device=dev)
            self._rec = torch.zeros(8, dtype=torch.int64, device=dev)                    # [record: 5 | |u| | -]
            self._rec_host = torch.zeros(8, dtype=torch.int64).pin_memory()
            self._u = torch.zeros(self.W, dtype=torch.int32, device=dev)
            self._v = torch.zeros(self.ldx, dtype=torch.int32, device=dev)
            self._col_work = torch.zeros(-(-self.m // 32), dtype=torch.int32, device=dev)
        self._p_tp, self._p_fp = self._p(self._rows), self._p(self._rows, self.m)
        self.list = np.zeros(0, dtype=np.int32)    # the remaining candidates, ascending
        self._rows_fresh = False
        self._weights = None
        self._factors = []
        self.launches = 0                          # of the last best() call

    @property
    def n_factors(self) -> int:
        return len(self._factors)

    # ---- candidates ---------------------------------------------------------------------------------------------------
    def build_basis(self, tau) -> int:
        """Candidate row i = (C[i, :] / C[i, i] > tau) of the column co-occurrence counts C = X^T X; returns how many are not empty."""
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_asso_basis(ptr(self.bits.bits_t), self.n, self.W, float(tau), ptr(self.basis), self.ldx, ptr(self._count),
                                     self._stream), "bmf_asso_basis")
            count = self._count.cpu().numpy()
        self.list = np.nonzero(count > 0)[0].astype(np.int32)
        return int(self.list.size)

    def basis_rows(self) -> np.ndarray:
        """The candidate matrix (all n rows, the empty ones included) as uint8, on the host."""
        b = self.basis.cpu().numpy().view(np.uint8)
        return np.unpackbits(b, axis=1, bitorder="little")[:, : self.n]

    def remove(self, cand: int):
        self.list = self.list[self.list != cand]

    # ---- sweep ----------------------------------------------------------------------------------------------------------
    def row_counts(self):
        """(TP_old, FP_old) per row of the current prediction against X, on the host; refreshed on the device when stale."""
        with torch.cuda.device(self.device), self._on_stream():
            if not self._rows_fresh:
                check(lib.bmf_confusion_rows(ptr(self.bits.bits), self.ldx, ptr(self.pd), self.ldx, self.m, self.ldx, self._p_tp, self._p_fp,
                                             self._stream), "bmf_confusion_rows")
                self._rows_fresh = True
            host = self._rows.cpu().numpy()
        return host[: self.m].astype(np.int64), host[self.m:].astype(np.int64)

    def launch_score(self, pos: int, count: int, best_score: float, w_fp: float, w_fn: float):
        """Enqueue bmf_asso_score and bmf_asso_pick on entries [pos, pos + count) of the device list; no read, no wait."""
        p_cand = self._p(self._cand, pos)
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_asso_score(ptr(self.bits.bits), ptr(self.pd), ptr(self.basis), self.ldx, self.m, self.n, p_cand, count,
                                     self._p_tp, self._p_fp, w_fp, w_fn, ptr(self._work), self._stream), "bmf_asso_score")
            check(lib.bmf_asso_pick(ptr(self._work), self.m, p_cand, count, best_score, w_fp, w_fn, ptr(self._T), ptr(self._F),
                                    ptr(self._score), ptr(self._rec), self._stream), "bmf_asso_pick")

    def launch_results(self, count: int):
        """(T, F, score) per candidate of the last launch and its record, on the host (tests, timing)."""
        with torch.cuda.device(self.device), self._on_stream():
            out = [t[:count].cpu().numpy() for t in (self._T, self._F, self._score)]
            rec = self._rec.cpu().numpy()[:5].copy()
        return out[0], out[1], out[2], rec

    def set_list(self, cands):
        """Replace the candidate list by hand (tests, timing)."""
        self.list = np.ascontiguousarray(cands, dtype=np.int32)

    def best(self, best_score, w_fp, w_fn, block=None):
        """(position in the list, candidate, score, T, F) of the candidate with the largest score above best_score, the first of
        equals, or None.  T, F: TP and FP of the prediction with that candidate's factor added."""
        w_fp, w_fn, running = float(w_fp), float(w_fn), float(best_score)
        self._weights = (w_fp, w_fn)
        self.launches = 0
        total = int(self.list.size)
        if total == 0:
            return None
        self.row_counts()
        with torch.cuda.device(self.device), self._on_stream():
            self._cand[:total].copy_(torch.from_numpy(self.list))
        step = self._max_block if not block else min(int(block), self._max_block)
        hit = None
        for pos in range(0, total, step):
            count = min(step, total - pos)
            self.launch_score(pos, count, running, w_fp, w_fn)
            with torch.cuda.device(self.device), self._on_stream():
                self._rec_host.copy_(self._rec, non_blocking=True)
                self._stream_obj.synchronize()
            self.launches += 1
            rec = self._rec_host.numpy()
            if rec[0] >= 0:
                running = struct.unpack("d", struct.pack("q", int(rec[2])))[0]
                hit = (pos + int(rec[0]), int(rec[1]), running, int(rec[3]), int(rec[4]))
        return hit

    def column(self, cand: int, w_fp=None, w_fn=None):
        """(u, v) of candidate `cand` against the current prediction: v = its basis row (n_pad / 32 words), u = the rows that take it
        (m_pad / 32 words).  Weights: those of the last best() call unless given."""
        if w_fp is None:
            w_fp, w_fn = self._weights
        if not 0 <= cand < self.n:
            raise ValueError(f"candidate {cand} outside [0, {self.n})")
        self.row_counts()
        with torch.cuda.device(self.device), self._on_stream():
            self._v.copy_(self.basis[cand])
            check(lib.bmf_asso_column(ptr(self.bits.bits), ptr(self.pd), ptr(self._v), self.ldx, self.m, self._p_tp, self._p_fp,
                                      float(w_fp), float(w_fn), ptr(self._u), ptr(self._col_work), C.c_void_p(self._rec.data_ptr() + 40),
                                      self._stream), "bmf_asso_column")
            u, v = self._u.cpu().numpy().view(np.uint32).copy(), self._v.cpu().numpy().view(np.uint32).copy()
        return u, v

    # ---- prediction -----------------------------------------------------------------------------------------------------
    def _or_in(self, u, v):
        with torch.cuda.device(self.device), self._on_stream():
            self._u.copy_(torch.from_numpy(u.view(np.int32)))
            self._v.copy_(torch.from_numpy(v.view(np.int32)))
            check(lib.bmf_asso_apply(ptr(self.pd), self.ldx, self.m, ptr(self._u), ptr(self._v), self._stream), "bmf_asso_apply")
        self._rows_fresh = False

    def apply(self, u, v):
        """The factor (u, v), packed words as column() returns them, joins the prediction."""
        u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
        assert u.size == self.W and v.size == self.ldx
        self._or_in(u, v)
        self._factors.append((u.copy(), v.copy()))

    def load_prediction(self, X_pd):
        """Replace the prediction by a dense 0 / 1 matrix (tests, timing); the factor list is left alone."""
        rows = np.zeros((self.m, self.ldx * 32), dtype=np.uint8)
        rows[:, : self.n] = np.asarray(X_pd) != 0
        words = np.packbits(rows, axis=1, bitorder="little").view(np.int32)
        with torch.cuda.device(self.device), self._on_stream():
            self.pd[: self.m].copy_(torch.from_numpy(words))
        self._rows_fresh = False

    def truncate(self, k: int):
        """Keep the first k applied factors: the prediction is rebuilt from them."""
        self._factors = self._factors[:k]
        with torch.cuda.device(self.device), self._on_stream():
            self.pd.zero_()
        self._rows_fresh = False
        for u, v in self._factors:
            self._or_in(u, v)

    def _pd_bits(self, for_counts):
        return self.pd, False
