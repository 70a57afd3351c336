"""Device state of a HyperPlus fit (``PyBMF/models/HyperPlus.py``): the factors' row and column sets as bit rows, the cover they make
and the records of merge trials (csrc/hyperplus.hip).  The matrices are kept in the transposed orientation, as ``HyperEngine`` keeps
them: every bit row of x_t / rs_t / pd_t runs over the m rows of X (W = m_pad / 32 words); a factor's T is a row of u_t (W words), its I
a row of v (n_pad / 32 words).

    eng.load_factors(T_lists, I_lists)      packs and uploads u_t and v, builds the cover, the residual and their sums with one
                                            apply launch per factor; one read (the sums)
    new_fp, nT, nI, nTc, nIc = eng.score_pairs(pairs)
                                            per pair of SLOTS (a, b): the false positives the merged rectangle would add, |T_a | T_b|,
                                            |I_a | I_b|, |T_a & T_b|, |I_a & I_b|, as int64 arrays; one launch, one pinned read
    T, I = eng.merge(slot_a, slot_b)        slot_a takes the union, slot_b is freed, the cover takes T x I; returns the union as
                                            packed words; one read (T, I and the new sums together)
    eng.order                               list position -> slot.  A merge leaves the others in order and the merged one last, the
                                            order of the reference's lists, without moving a device row
    eng.counts(name), eng.prediction(), eng.factor_arrays(), eng.bit_matrices(), eng.factor_bits(), eng.reads

A trial needs no product of the other k - 2 factors: T x I contains both rectangles it replaces, so the cover with the pair merged
is the current cover OR T x I, and FP(trial) = FP + new_fp.
Memory: the residual and the cover (two bit matrices of m_pad x n_pad bits) and k rows of u_t and v; both are refused when they do
not fit.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine, pack_bits
from .engine import BitMatrix


class HyperPlusEngine(BitSetEngine):
    title = "HyperPlus"

    def __init__(self, bits: BitMatrix, extra: dict = None):
        super().__init__(bits, extra)
        dev = self.device
        self.W, self.nvw = bits.ldxt, bits.ldx
        self.x_t = bits.bits_t
        with torch.cuda.device(dev):
            self._require_free(2 * (bits.m_pad * bits.n_pad // 8), "the bits of the residual and of the cover take", "; row sharding is not built")
            self.rs_t, self.pd_t = bits.bits_t.clone(), torch.zeros_like(bits.bits_t)
            self._count = torch.zeros(self.n, dtype=torch.int32, device=dev)        # |rs_t[j]| per column
            self._pdcount = torch.zeros(self.n, dtype=torch.int32, device=dev)
            # what merge() reads, in one copy: [residual sum, cover sum: 2 int64 | T: W words | I: nvw words]
            self._state = torch.zeros(4 + self.W + self.nvw, dtype=torch.int32, device=dev)
            self._state_host = torch.zeros(4 + self.W + self.nvw, dtype=torch.int32).pin_memory()
            self._rec_host = None
        self._rsum, self._pdsum = self.sum_x, 0
        self.k_slots, self.order, self._host = 0, [], {}
        self.reads = 0                        # host reads (stream synchronisations) so far
        with torch.cuda.device(dev), self._on_stream():
            check(lib.bmf_mebf_scores(ptr(self.rs_t), self.n, self.W, ptr(self._count), self._p(self._state), self._stream), "bmf_mebf_scores")

    def _apply(self, slot):
        """rs_t[j] &= ~T, pd_t[j] |= T for the columns j of the slot's I, with the column counts and the two sums; no read."""
        check(lib.bmf_mebf_apply(ptr(self.rs_t), ptr(self.pd_t), self.n, self.W, ptr(self.v[slot]), ptr(self.u_t[slot]), ptr(self._count),
                                 ptr(self._pdcount), self._p(self._state), self._stream), "bmf_mebf_apply")

    def _read_state(self, words):
        self._state_host.copy_(self._state, non_blocking=True)
        self._stream_obj.synchronize()
        self.reads += 1
        host = self._state_host.numpy()
        self._rsum, self._pdsum = (int(x) for x in host[:4].view(np.int64))
        return host[4:4 + words].view(np.uint32).copy()

    def load_factors(self, T_lists, I_lists):
        """The factors T_lists[i] x I_lists[i] (lists of rows, of columns) take the slots 0 .. k - 1 in list order."""
        assert not self.order, "load_factors() comes once, before the first merge()"
        k = len(T_lists)
        if len(I_lists) != k:
            raise ValueError(f"{k} row sets and {len(I_lists)} column sets")
        u = np.zeros((max(k, 1), self.W), dtype=np.uint32)
        v = np.zeros((max(k, 1), self.nvw), dtype=np.uint32)
        for i, (T, I) in enumerate(zip(T_lists, I_lists)):
            T, I = np.asarray(T, dtype=np.int64).reshape(-1), np.asarray(I, dtype=np.int64).reshape(-1)
            if T.size and (T.min() < 0 or T.max() >= self.m) or I.size and (I.min() < 0 or I.max() >= self.n):
                raise ValueError(f"factor {i} names a row or a column outside the {self.m} x {self.n} matrix")
            u[i], v[i] = pack_bits(np.isin(np.arange(self.m), T), self.W), pack_bits(np.isin(np.arange(self.n), I), self.nvw)
        with torch.cuda.device(self.device), self._on_stream():
            self._require_free(u.nbytes + v.nbytes, f"the row and column sets of {k} factors take")
            self.u_t, self.v = torch.from_numpy(u.view(np.int32)).to(self.device), torch.from_numpy(v.view(np.int32)).to(self.device)
            for i in range(k):
                self._apply(i)
            if k:
                self._read_state(0)
        self.k_slots, self.order = k, list(range(k))
        self._host = {i: (u[i].copy(), v[i].copy()) for i in range(k)}

    def score_pairs(self, pairs):
        """pairs: (count, 2) slots.  (new_fp, |T|, |I|, |T_a & T_b|, |I_a & I_b|) as int64 arrays; -1 for a pair that names no two
        different slots of the array."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        count = len(pairs)
        if count == 0:
            return tuple(np.zeros(0, dtype=np.int64) for _ in range(5))
        with torch.cuda.device(self.device), self._on_stream():
            pr = torch.from_numpy(pairs).to(self.device)
            rec = torch.empty((count, 5), dtype=torch.int64, device=self.device)
            if self._rec_host is None or self._rec_host.shape[0] < count:
                self._rec_host = torch.zeros((count, 5), dtype=torch.int64).pin_memory()
            check(lib.bmf_hyperplus_pairs(ptr(self.u_t), ptr(self.v), max(self.k_slots, 1), ptr(self.x_t), ptr(self.pd_t), self.n, self.W, self.nvw,
                                          ptr(pr), count, ptr(rec), self._stream), "bmf_hyperplus_pairs")
            self._rec_host[:count].copy_(rec, non_blocking=True)
            self._stream_obj.synchronize()
        self.reads += 1
        out = self._rec_host[:count].numpy().copy()
        return tuple(out[:, i].copy() for i in range(5))

    def merge(self, slot_a, slot_b):
        """The factor of slot_a becomes the union of the two, slot_b leaves the list, the cover takes T x I.  (T, I) as packed words."""
        pa, pb = self.order.index(slot_a), self.order.index(slot_b)
        if pa == pb:
            raise ValueError("merge() takes two different slots")
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_hyperplus_union(ptr(self.u_t), ptr(self.v), self.k_slots, self.W, self.nvw, slot_a, slot_b, slot_a, self._stream),
                  "bmf_hyperplus_union")
            self._apply(slot_a)
            self._state[4:4 + self.W].copy_(self.u_t[slot_a])
            self._state[4 + self.W:].copy_(self.v[slot_a])
            words = self._read_state(self.W + self.nvw)
        T, I = words[:self.W].copy(), words[self.W:].copy()
        self.order = [s for s in self.order if s not in (slot_a, slot_b)] + [slot_a]
        del self._host[slot_b]
        self._host[slot_a] = (T, I)
        return T, I

    @property
    def _factors(self):
        """The factors in list order as packed (u, v), what BitSetEngine.factor_arrays() reads."""
        return [self._host[s] for s in self.order]

    def counts(self, name="train"):
        """(TP, FP, FN, TN) of the prediction bits against data set `name`; the training set's without a device read."""
        if name != "train":
            self.reads += 1
            return super().counts(name)
        tp, fn = self.sum_x - self._rsum, self._rsum
        fp = self._pdsum - tp
        return tp, fp, fn, self.m * self.n - tp - fp - fn

    def _pd_bits(self, for_counts):
        return self.pd_t, True

    # ---- for tests ----------------------------------------------------------------------------------------------------
    def bit_matrices(self):
        """(rs_t, pd_t) as host uint32 arrays."""
        return self.rs_t.cpu().numpy().view(np.uint32), self.pd_t.cpu().numpy().view(np.uint32)

    def factor_bits(self):
        """(u_t, v) of the live slots in list order, from the device, as host uint32 arrays."""
        u, v = self.u_t.cpu().numpy().view(np.uint32), self.v.cpu().numpy().view(np.uint32)
        return u[self.order], v[self.order]
