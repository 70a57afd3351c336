"""Device state of a GreConD fit (``PyBMF/models/GreConD.py``): the bits of X, of the residual X_rs and of the prediction X_pd, all
transposed (one bit row of m_pad / 32 words per column of X, ``BitMatrix.bits_t``), and the concept search on them (csrc/grecond.hip).

    score, u, v = eng.concept(block=None)     one call of the reference's get_concept: u, v as packed uint32 words
    eng.apply(u, v)                           X_rs &= ~(u x v),  X_pd |= u x v, per-column residual counts refreshed
    eng.counts("train")                       (TP, FP, FN, TN) of X_pd against a data set
    eng.residual_sum(), eng.factor_arrays(), eng.prediction()

A sweep of get_concept replaces the best concept INSIDE the sweep, so the candidates behind an accepted one meet a new best_u.  Here a
launch evaluates a block of the sweep's remaining candidates against the current best_u, the device picks the FIRST one in column
order whose score exceeds best_score, that one is closed on the device, and the sweep goes on behind it (the scores of the block's
later candidates are dropped); a block without a winner just advances.  `block` is a speed knob only.  The host reads one record per
launch: the winner's (position, column, score, |u|, |v|) with the bits of best_v and best_u behind it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine, pack_bits, unpack_bits
from .engine import BitMatrix

MAX_ROWS_PAD = 32256   # the row sets of a candidate group (16 x m_pad / 8 bytes) and 1 KiB of scratch are kept within 64 KiB of LDS


class ConceptEngine(BitSetEngine):
    title = "GreConD"

    def __init__(self, bits: BitMatrix, extra: dict = None):
        super().__init__(bits, extra)
        dev = self.device
        self.W, self.nvw = bits.ldxt, bits.n_pad // 32
        if bits.m_pad > MAX_ROWS_PAD:
            raise NotImplementedError(f"GreConD on {self.m} rows: the concept scan keeps the row sets of 16 candidates within 64 KiB of LDS, "
                                      f"at most {MAX_ROWS_PAD} (padded) rows; row sharding is not built")
        n_work = int(lib.bmf_concept_scan_work(self.n))
        with torch.cuda.device(dev):
            # X and X^T are in HBM already (BitMatrix); the residual and the prediction add two transposed copies
            self._require_free(2 * bits.n_pad * self.W * 4 + n_work + 64 * self.n, "the bits of the residual and of the prediction take")
            self.rs_t = bits.bits_t.clone()
            self.pd_t = torch.zeros_like(bits.bits_t)
            self._work = torch.empty(n_work // 8 + 1, dtype=torch.int64, device=dev)
            self._cand = torch.zeros(max(self.n, 1), dtype=torch.int32, device=dev)
            self._score = torch.zeros(max(self.n, 1), dtype=torch.int64, device=dev)
            self._nu = torch.zeros(max(self.n, 1), dtype=torch.int32, device=dev)
            self._nv = torch.zeros(max(self.n, 1), dtype=torch.int32, device=dev)
            self._colcount = torch.zeros(bits.n_pad + 2, dtype=torch.int32, device=dev)   # [residual sum (int64) | count per column]
            # state: [rec: 8 int64 | best_v: nvw words | best_u: W words] -- what the host reads after a launch, in one copy
            self._state = torch.zeros(16 + self.nvw + self.W, dtype=torch.int32, device=dev)
            self._state_host = torch.zeros(16 + self.nvw + self.W, dtype=torch.int32).pin_memory()
            self._uv_dev = torch.zeros(self.nvw + self.W, dtype=torch.int32, device=dev)
            self._all_rows = torch.from_numpy(pack_bits(np.ones(self.m, dtype=bool), self.W).view(np.int32)).to(dev)
        self._p_rec, self._p_v, self._p_u = self._p(self._state), self._p(self._state, 16), self._p(self._state, 16 + self.nvw)
        self._state_np = self._state_host.numpy()
        self._factors = []
        self.launches = self.accepted = 0   # of the last concept() call
        self._refresh_counts(None, None)

    # ---- residual / prediction ----------------------------------------------------------------------------------------
    def _refresh_counts(self, u_ptr, v_ptr):
        cc = self._colcount
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_concept_apply(ptr(self.rs_t), ptr(self.pd_t), self.n, self.W, u_ptr, v_ptr, C.c_void_p(cc.data_ptr() + 8),
                                        C.c_void_p(cc.data_ptr()), self._stream), "bmf_concept_apply")
            host = cc[: self.n + 2].cpu().numpy()
        self._rsum = int(host[:2].view(np.int64)[0])
        self._col_host = host[2:].copy()

    def apply(self, u, v):
        """The factor (u, v), packed words as concept() returns them, leaves the residual and joins the prediction."""
        u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
        assert u.size == self.W and v.size == self.nvw
        with torch.cuda.device(self.device), self._on_stream():
            self._uv_dev.copy_(torch.from_numpy(np.concatenate([v, u]).view(np.int32)))
        base = self._uv_dev.data_ptr()
        self._refresh_counts(C.c_void_p(base + 4 * self.nvw), C.c_void_p(base))
        self._factors.append((u.copy(), v.copy()))

    def rebuild(self, U_bits, V_bits):
        """X_pd and X_rs made anew from the factors U_bits (f x W packed words) and V_bits (f x nvw): the only way a prediction shrinks
        (apply() never restores a residual bit).  The factors replace those applied so far; the per-column counts are refreshed."""
        U_bits = np.ascontiguousarray(U_bits, dtype=np.uint32).reshape(-1, self.W)
        V_bits = np.ascontiguousarray(V_bits, dtype=np.uint32).reshape(-1, self.nvw)
        f = U_bits.shape[0]
        assert V_bits.shape[0] == f
        cc = self._colcount
        with torch.cuda.device(self.device), self._on_stream():
            self._fac_u = torch.from_numpy(U_bits.view(np.int32)).to(self.device) if f else None
            self._fac_v = torch.from_numpy(V_bits.view(np.int32)).to(self.device) if f else None
            check(lib.bmf_bits_rebuild(ptr(self.bits.bits_t), self.n, self.W, ptr(self._fac_u) if f else None,
                                       ptr(self._fac_v) if f else None, self.nvw, f, ptr(self.pd_t), ptr(self.rs_t),
                                       C.c_void_p(cc.data_ptr() + 8), C.c_void_p(cc.data_ptr()), self._stream), "bmf_bits_rebuild")
            host = cc[: self.n + 2].cpu().numpy()
        self._rsum = int(host[:2].view(np.int64)[0])
        self._col_host = host[2:].copy()
        self._factors = [(U_bits[i].copy(), V_bits[i].copy()) for i in range(f)]

    def residual_sum(self) -> int:
        return self._rsum

    def _pd_bits(self, for_counts):
        return self.pd_t, True

    # ---- concept search -----------------------------------------------------------------------------------------------
    def residual_columns(self) -> np.ndarray:
        """The columns that still hold a residual one, ascending: the candidates of a concept search (j_rs of the reference)."""
        return np.nonzero(self._col_host > 0)[0].astype(np.int32)

    def set_search_state(self, best_u=None, cands=None):
        """Start a search by hand (tests, timing): best_u (packed words; None = all rows), best_v empty, `cands` as the sweep's list."""
        with torch.cuda.device(self.device), self._on_stream():
            self._state.zero_()
            self._state[16 + self.nvw:] = self._all_rows if best_u is None else \
                torch.from_numpy(np.ascontiguousarray(best_u, dtype=np.uint32).view(np.int32)).to(self.device)
            if cands is not None and len(cands):
                self._cand[: len(cands)].copy_(torch.from_numpy(np.ascontiguousarray(cands, dtype=np.int32)))

    def launch_scan(self, pos: int, count: int, best_score: int):
        """Enqueue bmf_concept_scan on candidates [pos, pos + count) of the list against the device's best_u; no read, no wait."""
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_concept_scan(ptr(self.bits.bits_t), ptr(self.rs_t), self.n, self.W, self._p_u,
                                       C.c_void_p(self._cand.data_ptr() + 4 * pos), count, int(best_score), ptr(self._work), ptr(self._score),
                                       ptr(self._nu), ptr(self._nv), self._p_rec, self._stream), "bmf_concept_scan")

    def scan_results(self, count: int):
        """(score, |u_j|, |v_j|) of the last launch_scan over `count` candidates and its record, on the host."""
        with torch.cuda.device(self.device), self._on_stream():
            out = [t[:count].cpu().numpy() for t in (self._score, self._nu, self._nv)]
            rec = self._state[:16].cpu().numpy().view(np.int64)[:5]
        return out[0], out[1], out[2], rec

    def _launch(self, pos: int, count: int, best_score: int):
        """Scan candidates [pos, pos + count) of the sweep's list, close the winner on the device, read the record."""
        self.launch_scan(pos, count, best_score)
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_concept_close(ptr(self.bits.bits_t), self.n, self.W, -1, self._p_rec, self._p_u, self._p_v, self._stream),
                  "bmf_concept_close")
            self._state_host.copy_(self._state, non_blocking=True)
            self._stream_obj.synchronize()
        self.launches += 1
        return self._state_np[:16].view(np.int64)

    def concept(self, block=None):
        """(score, u, v) of get_concept on the current residual; score 0 = no pattern (u = all rows, v = empty)."""
        self.launches = self.accepted = 0
        self.set_search_state()
        best_score = 0
        v_host = np.zeros(self.nvw, dtype=np.uint32)
        u_host = self._all_rows.cpu().numpy().view(np.uint32).copy()
        j_rs = self.residual_columns()
        while True:
            last = best_score
            j_list = j_rs[~unpack_bits(v_host, self.nvw * 32)[j_rs]] if j_rs.size else j_rs
            if j_list.size:
                with torch.cuda.device(self.device), self._on_stream():
                    self._cand[: j_list.size].copy_(torch.from_numpy(np.ascontiguousarray(j_list)))
            pos = 0
            while pos < j_list.size:
                count = j_list.size - pos if not block else min(int(block), j_list.size - pos)
                rec = self._launch(pos, count, best_score)
                if rec[0] >= 0:
                    best_score = int(rec[2])
                    pos += int(rec[0]) + 1
                    self.accepted += 1
                    v_host = self._state_np[16:16 + self.nvw].view(np.uint32).copy()
                    u_host = self._state_np[16 + self.nvw:].view(np.uint32).copy()
                else:
                    pos += count
            if best_score == last:
                break
        return best_score, u_host, v_host
