"""Device state of a GreConD+ fit (``PyBMF/models/GreConDPlus.py``) on top of ``ConceptEngine``: the concept search is the one of
GreConD, and on the same bits (csrc/grecondplus.hip)

    u_exp, v_exp, n = eng.expand(u, v, w_fp, w_fn, steps=None)    the reference's expansion() of a concept against the fixed residual
    U, V, U_exp, V_exp = eng.prune_overlapped(U, V, U_exp, V_exp) remove_overlapped() on packed factor bits (f x W and f x nvw words)
    eng.rebuild(U, V)                                             X_pd and X_rs anew from the surviving factors, both orientations
    eng.counts("train")                                           (TP, FP, FN, TN) of X_pd

The expansion scores row i by d_i = ((-w_fp) c_i + w_fn b_i) - w_fn a_i with a_i = |rs_i|, b_i = |x_i & (rs_i | v)|, c_i = |v & ~x_i|,
columns likewise against u.  One pass over the bits counts (a, b, c) for every row and every column; after that a joined column changes
the row counters only through its own bit row, so a step is O(m + n) and a whole expansion runs on one workgroup without a host read
per step.  A joined row needs the residual ROW-MAJOR, which ConceptEngine does not keep: rebuild() writes that second copy
(rs = x & ~OR of the v of the factors that hold the row), at the cost of one more bit matrix in HBM.

`steps` is the step budget of a launch (default: the whole expansion in one); every value gives the same result.  The record of the last
expansion stays in `eng.trace`: (axis, index, r_score, c_score) per evaluated step, the stop included (axis -1).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import bit_positions, popcount
from .grecond import ConceptEngine

class ExpansionEngine(ConceptEngine):
    title = "GreConD+"

    def __init__(self, bits, extra: dict = None):
        super().__init__(bits, extra)
        dev, m, n = self.device, self.m, self.n
        self.ldx = bits.ldx
        with torch.cuda.device(dev):
            self._require_free(bits.m_pad * self.ldx * 4 + 12 * (m + n) + 8 * int(lib.bmf_expand_rec_words(m, n)),
                               "the row-major residual and the expansion counters take")
            self.rs = bits.bits.clone()                                            # the residual row-major; rebuild() keeps it current
            self._row_abc = torch.zeros(3 * m, dtype=torch.int32, device=dev)
            self._col_abc = torch.zeros(3 * n, dtype=torch.int32, device=dev)
            # sets: [u | u_exp | v | v_exp], each padded to a multiple of 4 words (16-byte loads of the counts pass)
            self._sets = torch.zeros(2 * self.W + 2 * self.nvw, dtype=torch.int32, device=dev)
            self._n_rec = int(lib.bmf_expand_rec_words(m, n))
            self._rec = torch.zeros(self._n_rec, dtype=torch.int64, device=dev)
            self._rec_host = torch.zeros(self._n_rec, dtype=torch.int64).pin_memory()
        self._p_su, self._p_sue = self._p(self._sets), self._p(self._sets, self.W)
        self._p_sv, self._p_sve = self._p(self._sets, 2 * self.W), self._p(self._sets, 2 * self.W + self.nvw)
        self.trace = []
        self.host_reads = 0

    # ---- residual / prediction ----------------------------------------------------------------------------------------
    def rebuild(self, U_bits, V_bits):
        """ConceptEngine.rebuild, and the row-major residual from the same factors."""
        super().rebuild(U_bits, V_bits)
        f = len(self._factors)
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_bits_rebuild(ptr(self.bits.bits), self.m, self.ldx, ptr(self._fac_v) if f else None,
                                       ptr(self._fac_u) if f else None, self.W, f, None, ptr(self.rs), None, None, self._stream),
                  "bmf_bits_rebuild")

    def apply(self, u, v):
        raise NotImplementedError("GreConD+ sets its residual with rebuild(): apply() would leave the row-major copy behind")

    # ---- expansion ----------------------------------------------------------------------------------------------------
    def launch_counts(self):
        """Enqueue the two counts passes against the u and v of the device's sets; no read, no wait."""
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_expand_counts(ptr(self.bits.bits), ptr(self.rs), self.m, self.ldx, self._p_sv, ptr(self._row_abc), self._stream),
                  "bmf_expand_counts")
            check(lib.bmf_expand_counts(ptr(self.bits.bits_t), ptr(self.rs_t), self.n, self.W, self._p_su, ptr(self._col_abc), self._stream),
                  "bmf_expand_counts")

    def set_expansion_state(self, u, v):
        """u, v (packed words) become the sets of an expansion that has not begun; the counters are counted."""
        u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
        assert u.size == self.W and v.size == self.nvw
        host = np.concatenate([u, np.zeros(self.W, np.uint32), v, np.zeros(self.nvw, np.uint32)]).view(np.int32)
        with torch.cuda.device(self.device), self._on_stream():
            self._sets.copy_(torch.from_numpy(host))
            self._rec.zero_()
        self.launch_counts()

    def launch_steps(self, w_fp: float, w_fn: float, steps: int):
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_expand_steps(ptr(self.bits.bits), ptr(self.rs), ptr(self.bits.bits_t), ptr(self.rs_t), self.m, self.n, self.ldx,
                                       self.W, float(w_fp), float(w_fn), int(steps), ptr(self._row_abc), ptr(self._col_abc), self._p_su,
                                       self._p_sv, self._p_sue, self._p_sve, ptr(self._rec), self._stream), "bmf_expand_steps")

    def counters(self):
        """((a, b, c) of the rows, (a, b, c) of the columns) as the device holds them now."""
        with torch.cuda.device(self.device), self._on_stream():
            r, c = self._row_abc.cpu().numpy(), self._col_abc.cpu().numpy()
        return r.reshape(3, self.m), c.reshape(3, self.n)

    def read_record(self):
        """(joins, stopped, [(axis, index, r_score, c_score) per evaluated step]) of the expansion so far."""
        with torch.cuda.device(self.device), self._on_stream():
            self._rec_host.copy_(self._rec, non_blocking=True)
            self._stream_obj.synchronize()
        self.host_reads += 1
        rec = self._rec_host.numpy()
        seen = int(rec[2])
        e = rec[4:4 + 4 * seen].reshape(seen, 4)
        scores = e[:, 2:].copy().view(np.float64)
        return int(rec[0]), bool(rec[1]), [(int(e[i, 0]), int(e[i, 1]), float(scores[i, 0]), float(scores[i, 1])) for i in range(seen)]

    def sets(self):
        """(u, u_exp, v, v_exp) of the device, packed words."""
        with torch.cuda.device(self.device), self._on_stream():
            s = self._sets.cpu().numpy().view(np.uint32)
        W, nvw = self.W, self.nvw
        return s[:W].copy(), s[W:2 * W].copy(), s[2 * W:2 * W + nvw].copy(), s[2 * W + nvw:].copy()

    def expand(self, u, v, w_fp, w_fn, steps=None):
        """(u_exp, v_exp, n) of expansion(X, X_rs, u, v, w_fp, w_fn): packed words, n = the reference's n_iter (the stop counts)."""
        if not (np.isfinite(w_fp) and np.isfinite(w_fn)):
            raise ValueError("the weights of the expansion must be finite")
        budget = self.m + self.n + 1 if not steps else int(steps)
        if budget < 1:
            raise ValueError("steps must be a positive number of steps per launch")
        self.set_expansion_state(u, v)
        self.host_reads = 0
        while True:
            self.launch_steps(w_fp, w_fn, budget)
            joins, stopped, trace = self.read_record()
            if stopped:
                break
        self.trace = trace
        _, u_exp, _, v_exp = self.sets()
        return u_exp, v_exp, len(trace)

    # ---- overlap pruning ----------------------------------------------------------------------------------------------
    def _prefilter(self, sets, exts, X, lines, ld):
        """The (factor, line) pairs, line in the factor's extension, whose factor set lies inside the line of X."""
        pair_set, pair_line = [], []
        for k in range(exts.shape[0]):
            pos = bit_positions(exts[k])
            pair_line.append(pos)
            pair_set.append(np.full(pos.size, k, dtype=np.int32))
        pair_line, pair_set = np.concatenate(pair_line), np.concatenate(pair_set)
        if pair_line.size == 0:
            return 0
        with torch.cuda.device(self.device), self._on_stream():
            S = torch.from_numpy(np.ascontiguousarray(sets).view(np.int32)).to(self.device)
            pl, ps = torch.from_numpy(pair_line).to(self.device), torch.from_numpy(pair_set).to(self.device)
            flag = torch.zeros(pair_line.size, dtype=torch.int32, device=self.device)
            check(lib.bmf_bits_subset(ptr(X), lines, ld, ptr(S), sets.shape[0], ptr(pl), ptr(ps), pair_line.size, ptr(flag), self._stream),
                  "bmf_bits_subset")
            return int(flag.sum().item())

    def prune_overlapped(self, U, V, U_exp, V_exp):
        """remove_overlapped() on packed factors (f x W, f x nvw words).  A row of an extension can only leave when its row of X holds
        the factor's v, a column when its column holds u: those subset tests run first, and the count matrix U @ V.T (m x n int32) is
        only built when one of them passes.  self.pruned = (pairs that passed, rows removed, columns removed)."""
        U, V = np.array(U, dtype=np.uint32).reshape(-1, self.W), np.array(V, dtype=np.uint32).reshape(-1, self.nvw)
        U_exp, V_exp = np.array(U_exp, dtype=np.uint32).reshape(-1, self.W), np.array(V_exp, dtype=np.uint32).reshape(-1, self.nvw)
        f = U.shape[0]
        assert V.shape[0] == f and U_exp.shape[0] == f and V_exp.shape[0] == f
        self.pruned = (0, 0, 0)
        if f == 0 or not (U_exp.any() or V_exp.any()):
            return U, V, U_exp, V_exp
        passed = self._prefilter(V, U_exp, self.bits.bits, self.m, self.ldx) + self._prefilter(U, V_exp, self.bits.bits_t, self.n, self.W)
        if passed == 0:
            return U, V, U_exp, V_exp
        m, n, dev = self.m, self.n, self.device
        with torch.cuda.device(dev), self._on_stream():
            self._require_free(4 * m * n, "the count matrix U @ V.T of the overlap pruning takes", "; tiling it is not built")
            dU, dV = torch.from_numpy(U.view(np.int32)).to(dev), torch.from_numpy(V.view(np.int32)).to(dev)
            dUe, dVe = torch.from_numpy(U_exp.view(np.int32)).to(dev), torch.from_numpy(V_exp.view(np.int32)).to(dev)
            cov = torch.empty((m, n), dtype=torch.int32, device=dev)
            u_old = torch.zeros(self.W, dtype=torch.int32, device=dev)
            check(lib.bmf_overlap_counts(ptr(dU), self.W, ptr(dV), self.nvw, f, m, n, ptr(cov), n, self._stream), "bmf_overlap_counts")
            for k in range(f):
                if not (U_exp[k].any() or V_exp[k].any()):
                    continue
                check(lib.bmf_overlap_prune(ptr(self.bits.bits), self.ldx, m, n, ptr(cov), n, C.c_void_p(dU.data_ptr() + 4 * self.W * k),
                                            C.c_void_p(dUe.data_ptr() + 4 * self.W * k), C.c_void_p(dV.data_ptr() + 4 * self.nvw * k),
                                            C.c_void_p(dVe.data_ptr() + 4 * self.nvw * k), ptr(u_old), self.W, self._stream),
                      "bmf_overlap_prune")
            out = [t.cpu().numpy().view(np.uint32) for t in (dU, dV, dUe, dVe)]
        self.pruned = (passed, popcount(U_exp) - popcount(out[2]), popcount(V_exp) - popcount(out[3]))
        return tuple(out)
