"""Device state of a Hyper fit (``PyBMF/models/Hyper.py``): the vertical miner, the candidates' tidsets and the hyperrectangle records
on the residual (csrc/hyper.hip).  Only the transposed orientation is kept: every bit row runs over the m rows of X (W = m_pad / 32
words), as ``BitMatrix.bits_t`` does.

    sets = eng.mine(min_support)   the frequent itemsets of length >= 2 in the defined order; candidate id j < n is the singleton [j],
                                   id n + i is sets[i]; their tidsets stay on the device
    nT, s = eng.evaluate_all(ids)  find_hyper of the listed candidates (default: all) on the residual as it stands: |T| and
                                   X_rs[T, I].sum() per candidate id, T's bits in the scratch row of the candidate; one launch, one read
    eng.commit(ids)                scratch T rows -> committed T rows; no read
    T = eng.apply(id)              the factor (committed T of id) x (itemset of id) leaves the residual and joins the cover; returns
                                   T as packed words; one read (T and the new sums together)
    eng.residual_sum(), eng.counts(name), eng.tidsets(), eng.committed_T(id), eng.reads

The miner: level L + 1 joins every frequent itemset of level L with every larger column that occurs in level L; one launch
(bmf_hyper_level) ANDs and counts a whole level, the host tests count / m >= min_support in fp64 and keeps the frequent slots by
index.  There is no subset prune: it would only spare candidates, the frequent sets are the same.  A level is read once.
Memory: tidsets, scratch T rows and committed T rows are 3 * candidates * W * 4 bytes; a level in flight holds one more row per
joined pair.  Both are refused when they do not fit.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib, ptr
from .bitset import BitSetEngine, pack_bits
from .engine import BitMatrix


class HyperEngine(BitSetEngine):
    title = "Hyper"

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
            self._hit = torch.zeros(self.nvw, dtype=torch.int32, device=dev)
            # what apply() reads, in one copy: [residual sum, cover sum: 2 int64 | T: W words]
            self._state = torch.zeros(4 + self.W, dtype=torch.int32, device=dev)
            self._state_host = torch.zeros(4 + self.W, dtype=torch.int32).pin_memory()
        self._rsum, self._pdsum, self._factors = self.sum_x, 0, []
        self.itemsets, self.n_cand = None, 0
        self.reads = 0                        # host reads (stream synchronisations) so far
        with torch.cuda.device(dev), self._on_stream():
            check(lib.bmf_mebf_scores(ptr(self.rs_t), self.n, self.W, ptr(self._count), self._p(self._state), self._stream), "bmf_mebf_scores")

    def _rows(self, count, what):
        """`count` rows of W words, refused when they do not fit."""
        self._require_free(count * self.W * 4, f"{what} take")
        return torch.empty((count, self.W), dtype=torch.int32, device=self.device)

    def _ints(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    # ---- miner --------------------------------------------------------------------------------------------------------
    def _level(self, prev, n_prev, pairs):
        """(tidsets, counts) of the joined pairs (parent slot in `prev`, column): one launch, one read."""
        count = len(pairs)
        out = self._rows(count, f"the tidsets of a level of {count} candidates")
        cnt = torch.empty(count, dtype=torch.int32, device=self.device)
        pr = self._ints(pairs)
        check(lib.bmf_hyper_level(ptr(prev), n_prev, ptr(self.x_t), self.n, self.W, ptr(pr), count, ptr(out), ptr(cnt), self._stream), "bmf_hyper_level")
        self.reads += 1
        return out, cnt.cpu().numpy().astype(np.int64)

    def mine(self, min_support):
        """The frequent itemsets of length >= 2 (lists of ascending columns; levels ascend, lexicographic inside a level).  Leaves
        `itemsets` (singletons first), `support_counts` (of the mined sets) and the tidsets of every candidate on the device."""
        n, m = self.n, self.m
        sets, counts, kept = [], [], []           # kept: (level tensor, the frequent slots in it)
        with torch.cuda.device(self.device), self._on_stream():
            assert not self._factors, "mine() comes before the first apply(): the column counts of the residual are those of X"
            cnt1 = self._count.cpu().numpy().astype(np.int64)                       # level 1 is x_t itself: |x_t[j]| from the scores
            self.reads += 1
            level = [((j,), j) for j in range(n) if np.float64(cnt1[j]) / m >= min_support]          # (itemset, slot)
            prev, n_prev = self.x_t, n
            while level:
                items = sorted({j for cols, _ in level for j in cols})
                pairs, cols_of = [], []
                for cols, slot in level:
                    for j in items:
                        if j > cols[-1]:
                            pairs.append((slot, j))
                            cols_of.append(cols + (j,))
                if not pairs:
                    break
                tid, cnt = self._level(prev, n_prev, pairs)
                level = [(cols_of[i], i) for i in range(len(pairs)) if np.float64(cnt[i]) / m >= min_support]
                if level:
                    kept.append((tid, [slot for _, slot in level]))
                    sets += [list(cols) for cols, _ in level]
                    counts += [int(cnt[slot]) for _, slot in level]
                prev, n_prev = tid, len(pairs)
            del prev
            self._adopt(sets, counts, kept)
        return sets

    def _adopt(self, sets, counts, kept):
        """The candidates are the singletons and `sets`; kept: [(level tensor, the slots of its frequent rows)], in the order of
        `sets`.  Gathers the tidsets into one array and makes the scratch and the committed T rows, the item lists and the records."""
        n = self.n
        C = n + len(sets)
        self._require_free(3 * C * self.W * 4, f"the tidsets, the scratch and the committed T rows of {C} candidates take")
        self._tid = torch.empty((C, self.W), dtype=torch.int32, device=self.device)
        self._tid[:n].copy_(self.x_t[:n])
        at = n
        while kept:
            tid, slots = kept.pop(0)
            src, dst = self._ints(slots), self._ints(np.arange(at, at + len(slots)))
            check(lib.bmf_hyper_copy(ptr(tid), tid.shape[0], ptr(src), ptr(self._tid), C, ptr(dst), self.W, len(slots), self._stream), "bmf_hyper_copy")
            at += len(slots)
            del tid
        self._scratch = torch.zeros((C, self.W), dtype=torch.int32, device=self.device)
        self._committed = torch.zeros((C, self.W), dtype=torch.int32, device=self.device)
        self.itemsets = [[j] for j in range(n)] + [list(I) for I in sets]
        self.maxlen = max(len(I) for I in self.itemsets)
        padded = np.full((C, self.maxlen), -1, dtype=np.int32)
        for i, I in enumerate(self.itemsets):
            padded[i, :len(I)] = I
        self._items = self._ints(padded)
        self._rec = torch.zeros((C, 2), dtype=torch.int32, device=self.device)
        self._rec_host = torch.zeros((C, 2), dtype=torch.int32).pin_memory()
        self.n_cand, self.support_counts = C, counts

    # ---- records ------------------------------------------------------------------------------------------------------
    def evaluate_all(self, ids=None):
        """(nT, s) as int64 arrays over the candidate ids: fresh for `ids` (default: every candidate), as they were for the others."""
        ids = np.arange(self.n_cand) if ids is None else np.asarray(ids)
        with torch.cuda.device(self.device), self._on_stream():
            if len(ids):
                d = self._ints(ids)
                check(lib.bmf_hyper_eval(ptr(self._tid), ptr(self.rs_t), self.n, self.W, ptr(self._items), self.maxlen, ptr(d), len(ids), self.n_cand,
                                         ptr(self._scratch), ptr(self._rec), self._stream), "bmf_hyper_eval")
            self._rec_host.copy_(self._rec, non_blocking=True)
            self._stream_obj.synchronize()
        self.reads += 1
        rec = self._rec_host.numpy().astype(np.int64)
        return rec[:, 0].copy(), rec[:, 1].copy()

    def commit(self, ids):
        """The scratch T rows of `ids` become their committed T rows."""
        ids = sorted(int(i) for i in ids)
        if not ids:
            return
        with torch.cuda.device(self.device), self._on_stream():
            d = self._ints(ids)
            check(lib.bmf_hyper_copy(ptr(self._scratch), self.n_cand, ptr(d), ptr(self._committed), self.n_cand, ptr(d), self.W, len(ids), self._stream),
                  "bmf_hyper_copy")

    def apply(self, cid):
        """rs_t[j] &= ~T, pd_t[j] |= T for the columns j of candidate cid and its committed T; returns T (W packed words)."""
        v = pack_bits(np.isin(np.arange(self.n), self.itemsets[cid]), self.nvw)
        with torch.cuda.device(self.device), self._on_stream():
            self._hit.copy_(torch.from_numpy(v.view(np.int32)))
            T = self._committed[cid]
            check(lib.bmf_mebf_apply(ptr(self.rs_t), ptr(self.pd_t), self.n, self.W, ptr(self._hit), ptr(T), ptr(self._count), ptr(self._pdcount),
                                     self._p(self._state), self._stream), "bmf_mebf_apply")
            self._state[4:].copy_(T)
            self._state_host.copy_(self._state, non_blocking=True)
            self._stream_obj.synchronize()
        self.reads += 1
        host = self._state_host.numpy()
        self._rsum, self._pdsum = (int(x) for x in host[:4].view(np.int64))
        u = host[4:].view(np.uint32).copy()
        self._factors.append((u, v))
        return u

    def residual_sum(self) -> int:
        return self._rsum

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
    def tidsets(self):
        return self._tid.cpu().numpy().view(np.uint32)

    def committed_T(self, cid):
        return self._committed[cid].cpu().numpy().view(np.uint32)

    def bit_matrices(self):
        """(rs_t, pd_t) as host uint32 arrays."""
        return self.rs_t.cpu().numpy().view(np.uint32), self.pd_t.cpu().numpy().view(np.uint32)
