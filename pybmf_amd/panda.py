"""Device state of a Panda fit (``PyBMF/models/Panda.py``): the bits of X, of the residual X_rs and of the cover X_pd, each in both
orientations (``BitMatrix.bits`` / ``bits_t`` and four copies of their size), the transaction set T and the item set I of the
pattern that is being grown, and the scans over them (csrc/panda.hip).

    s = eng.scores("frequency" | "couples-frequency")      one int64 score per column of the residual
    h0 = eng.start_core(col)                               T := residual column `col`; its size
    eng.set_candidates(E)                                  the extension list, in the order the scans walk it
    i, h1, scores = eng.core_scan(pos, count, mode, w_model, w_fn, w0, h0, want_scores=False)
    eng.set_items(I)                                       I := the columns of the core
    r = eng.ext_scan(pos, count, n_t, n_i, w_model, w_fp, w_fn, cost_old)
    u, v = eng.apply_core()                                (T, I) leaves the residual and joins the cover, in both orientations
    eng.counts("train"), eng.error_counts(), eng.factor_cells(), eng.residual_sum(), eng.factor_arrays(), eng.prediction()

A scan takes candidates [pos, pos + count) of the list against the T the device holds.  core_scan: mode 0 picks the FIRST candidate in
list order whose d_cost <= 0, mode 1 (correlation) the highest |T & rs_e|, among equals the last position, if its d_cost <= 0; the
winner is closed on the device (T &= its column) in the same launch chain.  ext_scan picks the first candidate with cost_new <=
cost_old; on the device it joins I and the row pass follows (the rows outside T that the cost allows join T).  The sweep goes on
behind the winner; a block without a winner just advances.  The host reads one pinned record per launch chain -- the winner's
position and counts, the row pass's three integers -- never one per candidate, and the scores of a correlation round in the same
wait.  E's order is kept on the host: a sort is n log n on a list the host already holds, and the one list the device needs is
copied once per sweep (correlation: once per round, with the scores the host sorts by coming back in that round's read).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine, pack_bits, unpack_bits
from .engine import BitMatrix

REC_CORE, REC_EXT, OUT_ROWS, T_AT = 0, 16, 32, 40      # offsets into the state, in 32-bit words


class PatternEngine(BitSetEngine):
    title = "Panda"

    def __init__(self, bits: BitMatrix, extra: dict = None):
        super().__init__(bits, extra)
        dev = self.device
        self.W, self.nvw = bits.ldxt, bits.ldx
        self.x = [bits.bits_t, bits.bits]
        self.N, self.ld = [self.n, self.m], [self.W, self.nvw]
        W, nvw, n = self.W, self.nvw, self.n
        with torch.cuda.device(dev):
            self._require_free(4 * (bits.m_pad * bits.n_pad // 8), "the bits of the residual and of the cover in both orientations take",
                               "; row sharding is not built")
            self.rs = [bits.bits_t.clone(), bits.bits.clone()]
            self.pd = [torch.zeros_like(bits.bits_t), torch.zeros_like(bits.bits)]
            self._count = [torch.zeros(self.N[o], dtype=torch.int32, device=dev) for o in (0, 1)]      # |rs_j| per bit row
            self._pdcount = [torch.zeros(self.N[o], dtype=torch.int32, device=dev) for o in (0, 1)]
            self._couples = torch.zeros(n, dtype=torch.int64, device=dev)
            self._cand = torch.zeros(n, dtype=torch.int32, device=dev)
            self._a = torch.zeros(n, dtype=torch.int32, device=dev)
            self._b = torch.zeros(n, dtype=torch.int32, device=dev)
            self._work = torch.empty(int(lib.bmf_panda_rows_work(self.m)) // 4, dtype=torch.int32, device=dev)
            # state: [rec of the core scan: 8 int64 | rec of the extension scan: 8 int64 | out of the row pass: 4 int64 | T | I]
            self._state = torch.zeros(T_AT + W + nvw, dtype=torch.int32, device=dev)
            self._state_host = torch.zeros(T_AT + W + nvw, dtype=torch.int32).pin_memory()
            self._a_host = torch.zeros(n, dtype=torch.int32).pin_memory()
            self._out = torch.zeros(4, dtype=torch.int64, device=dev)
        self._p_core, self._p_ext, self._p_out = self._p(self._state, REC_CORE), self._p(self._state, REC_EXT), self._p(self._state, OUT_ROWS)
        self._p_T, self._p_I = self._p(self._state, T_AT), self._p(self._state, T_AT + W)
        self._host = self._state_host.numpy()
        self._rsum, self._pdsum, self._cells, self._factors = self.sum_x, 0, 0, []
        self.reads = 0                        # host reads (stream synchronisations) so far
        with torch.cuda.device(dev), self._on_stream():
            for o in (0, 1):
                check(lib.bmf_mebf_scores(ptr(self.rs[o]), self.N[o], self.ld[o], ptr(self._count[o]), ptr(self._out), self._stream), "bmf_mebf_scores")

    def _read(self, words, *more):
        """The first `words` words of the state (and further device -> pinned copies) in one wait."""
        self._state_host[:words].copy_(self._state[:words], non_blocking=True)
        for dst, src in more:
            dst.copy_(src, non_blocking=True)
        self._stream_obj.synchronize()
        self.reads += 1

    # ---- orderings ----------------------------------------------------------------------------------------------------
    def scores(self, method):
        """One int64 score per column: the residual column counts, or sum of the residual row counts over the column's ones minus
        its own count (every pair of ones in a row that the column takes part in)."""
        with torch.cuda.device(self.device), self._on_stream():
            if method == "frequency":
                out = self._count[0].cpu().numpy().astype(np.int64)
            elif method == "couples-frequency":
                check(lib.bmf_panda_couples(ptr(self.rs[0]), self.n, self.W, ptr(self._count[1]), self.m, ptr(self._couples), self._stream),
                      "bmf_panda_couples")
                out = self._couples.cpu().numpy()
            else:
                raise ValueError(f"no score called {method!r}")
        self.reads += 1
        return out

    # ---- the pattern being grown --------------------------------------------------------------------------------------
    def start_core(self, col):
        """T := residual column `col`; returns |T|."""
        with torch.cuda.device(self.device), self._on_stream():
            self._state[T_AT:T_AT + self.W].copy_(self.rs[0][col])
            check(lib.bmf_panda_close(ptr(self.rs[0]), self.n, self.W, int(col), self._p_core, self._p_T, self._stream), "bmf_panda_close")
            self._read(16)
        return int(self._host[:16].view(np.int64)[4])

    def set_candidates(self, E):
        E = np.ascontiguousarray(E, dtype=np.int32)
        assert E.size <= self.n
        if E.size:
            with torch.cuda.device(self.device), self._on_stream():
                self._cand[: E.size].copy_(torch.from_numpy(E))

    def set_items(self, I):
        """I := the columns listed."""
        flags = np.zeros(self.n, dtype=bool)
        flags[np.asarray(I, dtype=np.int64)] = True
        with torch.cuda.device(self.device), self._on_stream():
            self._state[T_AT + self.W:].copy_(torch.from_numpy(pack_bits(flags, self.nvw).view(np.int32)))

    def core_scan(self, pos, count, mode, w_model, w_fn, w0, h0, want_scores=False):
        """(winner's position in [0, count) or -1, its h1 = the new |T|, the h1 of all `count` candidates if wanted)."""
        assert 0 <= pos and count >= 1 and pos + count <= self.n
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_panda_core_scan(ptr(self.rs[0]), self.n, self.W, self._p_T, self._p(self._cand, pos), count, int(mode), float(w_model),
                                          float(w_fn), int(w0), int(h0), ptr(self._a), self._p_core, self._stream), "bmf_panda_core_scan")
            check(lib.bmf_panda_close(ptr(self.rs[0]), self.n, self.W, -1, self._p_core, self._p_T, self._stream), "bmf_panda_close")
            self._read(16, *([(self._a_host[:count], self._a[:count])] if want_scores else []))
        rec = self._host[:16].view(np.int64)
        win = int(rec[0])
        assert win < 0 or rec[4] == rec[2], "the closed T does not have the size the scan counted"
        return win, int(rec[2]), (self._a_host[:count].numpy().astype(np.int64) if want_scores else None)

    def ext_scan(self, pos, count, n_t, n_i, w_model, w_fp, w_fn, cost_old):
        """dict(i = the winner's position or -1, a, b = its counts, added, sum_d_fn, sum_d_fp = the row pass behind it).  n_t = |T|
        now, n_i = |I| once the winner has joined."""
        assert 0 <= pos and count >= 1 and pos + count <= self.n
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_panda_ext_scan(ptr(self.rs[0]), ptr(self.pd[0]), self.n, self.W, self._p_T, self._p(self._cand, pos), count, int(n_t),
                                         float(w_model), float(w_fp), float(w_fn), float(cost_old), ptr(self._a), ptr(self._b), self._p_ext,
                                         self._stream), "bmf_panda_ext_scan")
            check(lib.bmf_panda_rows(ptr(self.rs[1]), ptr(self.pd[1]), self.m, self.nvw, self.n, -1, self._p_ext, self._p_I, int(n_i), self._p_T,
                                     self.W, float(w_model), float(w_fp), float(w_fn), ptr(self._work), self._p_out, self._stream), "bmf_panda_rows")
            self._read(T_AT)
        rec, out = self._host[REC_EXT:REC_EXT + 16].view(np.int64), self._host[OUT_ROWS:OUT_ROWS + 8].view(np.int64)
        return dict(i=int(rec[0]), a=int(rec[2]), b=int(rec[3]), added=int(out[0]), sum_d_fn=int(out[1]), sum_d_fp=int(out[2]))

    def core_rows(self):
        """T as packed words, from the device."""
        with torch.cuda.device(self.device), self._on_stream():
            self._read(T_AT + self.W)
        return self._host[T_AT:T_AT + self.W].view(np.uint32).copy()

    def apply_core(self):
        """(T, I) as the device holds them leave the residual and join the cover; returns them as packed words."""
        with torch.cuda.device(self.device), self._on_stream():
            for o, hit, mask in ((0, self._p_I, self._p_T), (1, self._p_T, self._p_I)):
                check(lib.bmf_mebf_apply(ptr(self.rs[o]), ptr(self.pd[o]), self.N[o], self.ld[o], hit, mask, ptr(self._count[o]),
                                         ptr(self._pdcount[o]), self._p(self._out, 4 * o), self._stream), "bmf_mebf_apply")
            out = self._out.cpu().numpy()
            self._read(T_AT + self.W + self.nvw)
        assert out[0] == out[2] and out[1] == out[3], "the two orientations disagree"
        self._rsum, self._pdsum = int(out[0]), int(out[1])
        u = self._host[T_AT:T_AT + self.W].view(np.uint32).copy()
        v = self._host[T_AT + self.W:].view(np.uint32).copy()
        self._factors.append((u, v))
        self._cells += int(unpack_bits(u, self.m).sum()) + int(unpack_bits(v, self.n).sum())
        return u, v

    # ---- counts -------------------------------------------------------------------------------------------------------
    def factor_cells(self) -> int:
        """|U| + |V| of the factors applied so far."""
        return self._cells

    def residual_sum(self) -> int:
        return self._rsum

    def error_counts(self):
        """(FP, FN) of the cover as it stands."""
        tp = self.sum_x - self._rsum
        return self._pdsum - tp, self._rsum

    def counts(self, name="train"):
        """(TP, FP, FN, TN) of the cover against data set `name`; the training set's without a device read."""
        if name != "train":
            self.reads += 1
            return super().counts(name)
        fp, fn = self.error_counts()
        tp = self.sum_x - fn
        return tp, fp, fn, self.m * self.n - tp - fp - fn

    def _pd_bits(self, for_counts):
        return (self.pd[0], True) if for_counts else (self.pd[1], False)

    def bit_matrices(self):
        """(rs_t, pd_t, rs, pd) as host uint32 arrays (tests)."""
        return tuple(t.cpu().numpy().view(np.uint32) for t in (self.rs[0], self.pd[0], self.rs[1], self.pd[1]))
