"""Device state of the two refiners of an Asso model (``PyBMF/models/AssoIter.py``, ``AssoOpt.py``): the bits of X (``BitMatrix``),
one bit row per factor of V, one factor mask per row of U, and the kernels of csrc/asso_refine.hip on them.

    eng.load_factors(U, V)                              dense 0 / 1 factors, (m, k) and (n, k)
    score, TP, FP, n_u = eng.refine_column(k, w_fp, w_fn)   AssoIter: column k of U re-decided against the other factors; TP, FP of the
                                                        new prediction, score = w_fn TP - w_fp FP, n_u = rows that take the factor
    score, TP, FP, ones = eng.optimal_rows(w_fp, w_fn)  AssoOpt: every row of U becomes its first best subset; eng.chosen() = j per row
    eng.counts("train"), eng.factor_arrays(), eng.prediction()

U changes on the device only; the host reads one record of four numbers per launch.  The prediction bits are built from U and V when
counts() or prediction() ask for them.

Limits (bmf_asso_refine_chunk): a workgroup keeps the V bit rows in at most 60 KiB of the CU's 160 KiB of LDS, `chunk` words of every
row at a time -- all of them when k n_pad bits fit (k = 64 at n = 7552), else the kernels walk over n chunk by chunk with their counts in
registers; `chunk=` forces a smaller one (any multiple of 4 gives the same result).  refine_column takes k <= 1024 (a chunk of at
least 8 words must fit), optimal_rows k <= 16 (2^k subsets per row); beyond that NotImplementedError.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine
from .engine import BitMatrix

K_MAX_COLUMN, K_MAX_ROWS = 1024, 16


class AssoRefineEngine(BitSetEngine):
    def __init__(self, bits: BitMatrix, extra: dict = None):
        super().__init__(bits, extra)
        dev = self.device
        self.ldx = bits.ldx
        self.k = 0
        with torch.cuda.device(dev):
            self._part = torch.zeros(3 * self.m, dtype=torch.int64, device=dev)
            self._u = torch.zeros(-(-self.m // 32), dtype=torch.int32, device=dev)
            self._j = torch.zeros(self.m, dtype=torch.int32, device=dev)
            self._rec = torch.zeros(4, dtype=torch.int64, device=dev)
            self._rec_host = torch.zeros(4, dtype=torch.int64).pin_memory()
        self.pd = None            # the prediction bits, made on demand
        self._pd_fresh = False

    # ---- factors ----------------------------------------------------------------------------------------------------------
    def load_factors(self, U, V):
        """U (m, k), V (n, k): dense arrays, nonzero = 1."""
        U, V = np.asarray(U) != 0, np.asarray(V) != 0
        if U.ndim != 2 or V.ndim != 2 or U.shape[0] != self.m or V.shape[0] != self.n or U.shape[1] != V.shape[1] or U.shape[1] < 1:
            raise ValueError(f"factors of shape {U.shape}, {V.shape} do not fit a {self.m} x {self.n} matrix")
        self.k = k = U.shape[1]
        self.kw = -(-k // 32)
        masks = np.zeros((self.m, self.kw * 32), dtype=np.uint8)
        masks[:, :k] = U
        rows = np.zeros((k, self.ldx * 32), dtype=np.uint8)
        rows[:, : self.n] = V.T
        with torch.cuda.device(self.device), self._on_stream():
            self.U = torch.from_numpy(np.packbits(masks, axis=1, bitorder="little").view(np.int32).copy()).to(self.device)
            self.V = torch.from_numpy(np.packbits(rows, axis=1, bitorder="little").view(np.int32).copy()).to(self.device)
        self._pd_fresh = False

    def _chunk(self, chunk, rows_kernel):
        limit = K_MAX_ROWS if rows_kernel else K_MAX_COLUMN
        what = "optimal_rows searches 2^k subsets per row" if rows_kernel else "refine_column keeps 8 words of every factor's bit row in 60 KiB of LDS"
        if self.k < 1:
            raise ValueError("no factors are loaded")
        if self.k > limit or lib.bmf_asso_refine_chunk(self.k, self.ldx, int(rows_kernel)) < 0:
            raise NotImplementedError(f"k = {self.k}: {what}, k <= {limit}")
        return 0 if chunk is None else int(chunk)

    def _record(self):
        with torch.cuda.device(self.device), self._on_stream():
            self._rec_host.copy_(self._rec, non_blocking=True)
            self._stream_obj.synchronize()
        rec = self._rec_host.numpy()
        self._pd_fresh = False
        return struct.unpack("d", struct.pack("q", int(rec[0])))[0], int(rec[1]), int(rec[2]), int(rec[3])

    # ---- the two refinements ----------------------------------------------------------------------------------------------
    def refine_column(self, k: int, w_fp, w_fn, chunk=None):
        """Column k of U := the rows whose score rises, strictly, when factor k joins the other factors they hold.  Returns
        (score, TP, FP, |u|): TP, FP of the prediction with the new column, score = w_fn TP - w_fp FP."""
        chunk = self._chunk(chunk, False)
        if not 0 <= k < self.k:
            raise ValueError(f"column {k} outside [0, {self.k})")
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_asso_refine_column(ptr(self.bits.bits), self.ldx, self.m, ptr(self.V), self.k, ptr(self.U), self.kw, int(k), chunk,
                                             float(w_fp), float(w_fn), ptr(self._u), ptr(self._part), ptr(self._rec), self._stream),
                  "bmf_asso_refine_column")
        return self._record()

    def column(self):
        """The decisions of the last refine_column as a bool vector of m rows."""
        b = self._u.cpu().numpy().view(np.uint8)
        return np.unpackbits(b, bitorder="little")[: self.m].astype(bool)

    def optimal_rows(self, w_fp, w_fn, chunk=None):
        """Every row of U := the subset j of the factors with the largest score against the row of X, the first of equals in the order
        of j (factor 0 is the most significant bit).  Returns (score, TP, FP, ones of U) of the new prediction."""
        chunk = self._chunk(chunk, True)
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_asso_refine_rows(ptr(self.bits.bits), self.ldx, self.m, ptr(self.V), self.k, chunk, float(w_fp), float(w_fn),
                                           ptr(self._j), ptr(self.U), ptr(self._part), ptr(self._rec), self._stream), "bmf_asso_refine_rows")
        return self._record()

    def chosen(self):
        """j per row of the last optimal_rows."""
        return self._j.cpu().numpy().astype(np.int64)

    # ---- prediction -----------------------------------------------------------------------------------------------------
    def _pd_bits(self, for_counts):
        """U o V^T, built when U has changed since the last product."""
        if not self._pd_fresh:
            with torch.cuda.device(self.device), self._on_stream():
                if self.pd is None:
                    self.pd = torch.zeros_like(self.bits.bits)
                check(lib.bmf_asso_refine_product(ptr(self.U), self.kw, ptr(self.V), self.k, self.ldx, self.m, ptr(self.pd), self._stream),
                      "bmf_asso_refine_product")
            self._pd_fresh = True
        return self.pd, False

    def factor_arrays(self):
        """(U, V) as uint8 arrays of shape (m, k) and (n, k), from the device bits."""
        U = np.unpackbits(self.U.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, : self.k]
        V = np.unpackbits(self.V.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, : self.n].T
        return np.ascontiguousarray(U), np.ascontiguousarray(V)
