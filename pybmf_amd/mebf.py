"""Device state of an MEBF fit (``PyBMF/models/MEBF.py``): the bits of X, of the residual X_rs and of the cover X_pd, each in both
orientations (``BitMatrix.bits`` / ``bits_t`` and four copies of their size), and the median expansion on them (csrc/mebf.hip).

    c0, c1 = eng.growth(t)        the two candidates of bidirectional_growth (axis 0, axis 1)
    c = eng.weak(t)               the candidate of get_weak_signal(axis=0); IndexError on a matrix of one column, as the reference
    eng.apply(c["u"], c["v"], c)  X_rs &= ~(u x v), X_pd |= u x v in both orientations, row and column scores refreshed
    eng.truncate(kept)            a tolerance stop dropped factors: see below
    eng.rebuild(factors)          residual and cover reset to X and nothing, `factors` re-applied
    eng.counts("train"), eng.error_counts(), eng.base_counts(), eng.residual_sum(), eng.factor_arrays(), eng.prediction()

A candidate is a dict: axis, mid (weak: first) and P (weak: second), na = |a|, nb = |b|, dTP, dFP (the cells of a x b outside the
cover that are ones / zeros of X) and u (rows, m_pad / 32 words), v (columns, n_pad / 32 words).  Only integers and bits come back.
Everything of one growth is enqueued on one stream and read in one pinned copy; a factor applied with its candidate needs no read at
all (its vectors are on the device already and the new counts follow from dTP, dFP).

After ``truncate(kept)`` the reference goes on with the residual and the prediction it has -- they still hold the dropped factor --
while it scores the next candidates on the product of the kept U, V, and it rebuilds both from the kept factors and the new one once
that is set.  Here `kept` is rebuilt into a second set of buffers (made on first use): the growth reads the residual of the live set
and counts against the cover of the second, and the next apply() makes the second set the live one.  That path is cold.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine
from .engine import BitMatrix


class _State:
    """Residual and cover in both orientations with the popcount of every bit row; index 0 = transposed (axis 0), 1 = row-major."""

    def __init__(self, eng):
        dev = eng.device
        self.rs = [torch.empty_like(eng.x[0]), torch.empty_like(eng.x[1])]
        self.pd = [torch.empty_like(eng.x[0]), torch.empty_like(eng.x[1])]
        self.score = [torch.zeros(eng.N[o], dtype=torch.int32, device=dev) for o in (0, 1)]
        self.pdcount = [torch.zeros(eng.N[o], dtype=torch.int32, device=dev) for o in (0, 1)]
        self.rsum = self.pdsum = 0
        self.factors = []


class MedianEngine(BitSetEngine):
    title = "MEBF"

    def __init__(self, bits: BitMatrix, extra: dict = None):
        super().__init__(bits, extra)
        dev = self.device
        self.W, self.nvw = bits.ldxt, bits.ldx
        self.x = [bits.bits_t, bits.bits]
        self.N, self.ld = [self.n, self.m], [self.W, self.nvw]
        self.matrix_bytes = bits.m_pad * bits.n_pad // 8
        W, nvw = self.W, self.nvw
        with torch.cuda.device(dev):
            self._require(4, "the bits of X, of the residual and of the cover in both orientations: six bit matrices")
            self._live = _State(self)
            self._kept = None                 # the second set: made by the first truncate()
            self._stale = False
            n_work = max(int(lib.bmf_mebf_grow_work(self.N[o])) for o in (0, 1))
            self._work = torch.empty(n_work // 4, dtype=torch.int32, device=dev)
            # what the host reads after a growth, in one copy: [rec axis 0: 8 int64 | rec axis 1 | a0: W | b0: nvw | a1: nvw | b1: W]
            self._off = [(0, 32, 32 + W), (16, 32 + W + nvw, 32 + W + 2 * nvw)]          # (rec, a, b) per axis, in words
            self._state = torch.zeros(32 + 2 * W + 2 * nvw, dtype=torch.int32, device=dev)
            self._state_host = torch.zeros_like(self._state, device="cpu").pin_memory()
            self._wstate = torch.zeros(16 + W + nvw, dtype=torch.int32, device=dev)      # weak signal: [rec | a: W | b: nvw]
            self._wstate_host = torch.zeros_like(self._wstate, device="cpu").pin_memory()
            self._uv_dev = torch.zeros(W + nvw, dtype=torch.int32, device=dev)
            self._out = torch.zeros(4, dtype=torch.int64, device=dev)
        self.reads = 0                        # host reads (stream synchronisations) so far
        self._reset(self._live)

    def _require(self, matrices, what):
        self._require_free(matrices * self.matrix_bytes, what + " take", "; row sharding is not built")

    # ---- residual / cover ---------------------------------------------------------------------------------------------
    def _reset(self, st):
        """st := residual X, empty cover."""
        with torch.cuda.device(self.device), self._on_stream():
            for o in (0, 1):
                st.rs[o].copy_(self.x[o])
                st.pd[o].zero_()
                st.pdcount[o].zero_()
                check(lib.bmf_mebf_scores(ptr(st.rs[o]), self.N[o], self.ld[o], ptr(st.score[o]), ptr(self._out), self._stream), "bmf_mebf_scores")
        st.rsum, st.pdsum, st.factors = self.sum_x, 0, []

    def _apply(self, st, u_ptr, v_ptr, read=True):
        with torch.cuda.device(self.device), self._on_stream():
            for o, hit, mask in ((0, v_ptr, u_ptr), (1, u_ptr, v_ptr)):
                check(lib.bmf_mebf_apply(ptr(st.rs[o]), ptr(st.pd[o]), self.N[o], self.ld[o], hit, mask, ptr(st.score[o]), ptr(st.pdcount[o]),
                                         self._p(self._out, 4 * o), self._stream), "bmf_mebf_apply")
            if read:
                out = self._out.cpu().numpy()
                self.reads += 1
                assert out[0] == out[2] and out[1] == out[3], "the two orientations disagree"
                st.rsum, st.pdsum = int(out[0]), int(out[1])

    def _apply_host(self, st, u, v):
        u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
        assert u.size == self.W and v.size == self.nvw
        with torch.cuda.device(self.device), self._on_stream():
            self._uv_dev.copy_(torch.from_numpy(np.concatenate([u, v]).view(np.int32)))
        self._apply(st, self._p(self._uv_dev), self._p(self._uv_dev, self.W))
        st.factors.append((u.copy(), v.copy()))

    def apply(self, u, v, cand=None):
        """The factor (u, v) leaves the residual and joins the cover.  cand: the candidate of the LAST growth() / weak() call that
        (u, v) came from: its vectors are on the device and its dTP, dFP give the new counts, so nothing is copied or read."""
        if self._stale:
            self._live, self._kept, self._stale = self._kept, self._live, False
        st = self._live
        if cand is None or cand.get("_serial") != self._serial:
            return self._apply_host(st, u, v)
        self._apply(st, cand["_u_ptr"], cand["_v_ptr"], read=False)
        st.rsum, st.pdsum = st.rsum - cand["dTP"], st.pdsum + cand["dTP"] + cand["dFP"]
        st.factors.append((np.array(u, dtype=np.uint32), np.array(v, dtype=np.uint32)))

    def rebuild(self, factors):
        """Residual and cover reset to X and nothing, then every (u, v) of `factors` applied."""
        self._stale = False
        self._reset(self._live)
        for u, v in factors:
            self._apply_host(self._live, u, v)

    def truncate(self, kept):
        """A tolerance stop left the factors `kept` ([(u, v)] packed words) in U, V.  Residual and prediction stay as they are until the
        next apply(); the candidates until then are counted against the product of `kept`."""
        if self._kept is None:
            with torch.cuda.device(self.device):
                self._require(4, "a second set of residual and cover bits for the factors kept by a tolerance stop")
                self._kept = _State(self)
        self._reset(self._kept)
        for u, v in kept:
            self._apply_host(self._kept, u, v)
        self._stale = True

    def residual_sum(self) -> int:
        return self._live.rsum

    def _fp_fn(self, st):
        tp = self.sum_x - st.rsum
        return st.pdsum - tp, st.rsum

    def error_counts(self):
        """(FP, FN) of the prediction as it stands (after a truncation: still with the dropped factor)."""
        return self._fp_fn(self._live)

    def base_counts(self):
        """(FP, FN) of the cover that the candidates' dTP, dFP are counted against."""
        return self._fp_fn(self._kept if self._stale else self._live)

    def counts(self, name="train"):
        """(TP, FP, FN, TN) of the prediction bits against data set `name`; the training set's without a device read."""
        if name != "train":
            self.reads += 1
            return super().counts(name)
        fp, fn = self._fp_fn(self._live)
        tp = self.sum_x - fn
        return tp, fp, fn, self.m * self.n - tp - fp - fn

    def _pd_bits(self, for_counts):
        return (self._live.pd[0], True) if for_counts else (self._live.pd[1], False)

    @property
    def _factors(self):
        """The factors that make up the prediction."""
        return self._live.factors

    def bit_matrices(self, kept=False):
        """(rs_t, pd_t, rs, pd) of the live (or the kept) set as host uint32 arrays (tests)."""
        st = self._kept if kept else self._live
        return tuple(t.cpu().numpy().view(np.uint32) for t in (st.rs[0], st.pd[0], st.rs[1], st.pd[1]))

    # ---- growth -------------------------------------------------------------------------------------------------------
    _serial = 0

    def _enqueue_grow(self, axis, state, rec_w, a_w, b_w, a_from_rec, t):
        live, base = self._live, (self._kept if self._stale else self._live)
        nbw = self.nvw if axis == 0 else self.W
        check(lib.bmf_mebf_grow(ptr(live.rs[axis]), ptr(self.x[axis]), ptr(base.pd[axis]), self.N[axis], self.ld[axis], self._p(state, a_w),
                                a_from_rec, float(t), ptr(self._work), self._p(state, b_w), nbw, self._p(state, rec_w), self._stream),
              "bmf_mebf_grow")

    def _candidate(self, axis, state, host, rec_w, a_w, b_w):
        rec = host[rec_w:rec_w + 16].view(np.int64)
        la, lb = (self.W, self.nvw) if axis == 0 else (self.nvw, self.W)
        a, b = host[a_w:a_w + la].view(np.uint32).copy(), host[b_w:b_w + lb].view(np.uint32).copy()
        pa, pb = self._p(state, a_w), self._p(state, b_w)
        u, v, pu, pv = (a, b, pa, pb) if axis == 0 else (b, a, pb, pa)
        return dict(axis=axis, mid=int(rec[0]), P=int(rec[1]), na=int(rec[2]), nb=int(rec[3]), dTP=int(rec[4]), dFP=int(rec[5]), u=u, v=v,
                    _u_ptr=pu, _v_ptr=pv, _serial=self._serial)

    def growth(self, t):
        """The candidates of get_factor(axis=0) and get_factor(axis=1) on the current residual: one stream, one read."""
        self._serial += 1
        with torch.cuda.device(self.device), self._on_stream():
            for axis, (rec_w, a_w, b_w) in enumerate(self._off):
                check(lib.bmf_mebf_select(ptr(self._live.score[axis]), self.N[axis], 0, self._p(self._state, rec_w), self._stream), "bmf_mebf_select")
                self._enqueue_grow(axis, self._state, rec_w, a_w, b_w, 1, t)
            self._state_host.copy_(self._state, non_blocking=True)
            self._stream_obj.synchronize()
        self.reads += 1
        host = self._state_host.numpy()
        return [self._candidate(axis, self._state, host, *self._off[axis]) for axis in (0, 1)]

    def weak(self, t):
        """The candidate of get_weak_signal(axis=0): a = the AND of the two residual columns with the highest scores."""
        if self.n < 2:
            raise IndexError("index 1 is out of bounds for axis 0 with size 1")
        self._serial += 1
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_mebf_select(ptr(self._live.score[0]), self.n, 1, self._p(self._wstate), self._stream), "bmf_mebf_select")
            check(lib.bmf_mebf_weak_a(ptr(self._live.rs[0]), self.W, self._p(self._wstate), self._p(self._wstate, 16), self._stream), "bmf_mebf_weak_a")
            self._enqueue_grow(0, self._wstate, 0, 16, 16 + self.W, 0, t)
            self._wstate_host.copy_(self._wstate, non_blocking=True)
            self._stream_obj.synchronize()
        self.reads += 1
        return self._candidate(0, self._wstate, self._wstate_host.numpy(), 0, 16, 16 + self.W)
