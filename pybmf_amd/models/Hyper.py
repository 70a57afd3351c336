"""Hyper -- exact cover by overlapped hyperrectangles.  Drop-in for ``PyBMF/models/Hyper.py`` (Xiang et al., Summarizing
Transactional Databases with Overlapped Hyperrectangles).

The candidates are the singleton itemsets [j] of every column and the frequent itemsets of length >= 2 at `min_support`.  For an
itemset I, find_hyper takes the rows T that hold all of I in X and still have a residual one on I; its cost is (|T| + |I|) / (the
residual ones of T x I).  The fit is a lazy greedy: the list is kept in the order of the costs it knows, the head is re-evaluated on
the current residual and the list re-sorted until the head stays the cheapest, then T x I becomes a factor.  Mining is an AND-popcount
pass per level over column bit sets, find_hyper of EVERY live candidate on the current residual is one launch and one read per factor
(csrc/hyper.hip through ``pybmf_amd/hyper.py``); the device returns integers and bits only.  The residual does not change inside a
round, so the host replays the reference's pops, sorts, `c[0] > c[1]` tests and `iter` count on those integers -- the costs by the
reference's own fp64 expression -- remembers for each candidate the record it was last evaluated with, and commits, in one launch,
the T rows of exactly the candidates the reference would have recomputed.

Kept from the reference, on purpose:
  * find_hyper's greedy test is `cost_new <= cost_new`: always true, so T is all the candidate rows and the cost follows from two
    integers.  No candidate row: T = [], cost inf.
  * a round re-evaluates the head, then pops heads while their T is empty WITHOUT re-evaluating the new head: it can be accepted
    with the T and the cost of an earlier residual.  Such a stale T is still an exact rectangle of X (FP stays 0); it shows in
    `shape`, in U and in `model.T`.
  * `c[0] > c[1]` on a list of one candidate raises IndexError (a matrix of one column does at once), as does a list emptied by pops.
  * the number of rounds is bounded by the length of the candidate list BEFORE the loop; k = U.shape[1] at the end, so a fit that
    runs no round (X = 0) leaves k = 1 and an empty column.
Different from the reference:
  * the miner.  The reference calls mlxtend's `apriori`; here the miner is defined: levels ascend, inside a level the itemsets are in
    lexicographic order of their ascending column tuples, and an itemset is frequent iff count / m >= min_support in fp64 with the
    integer count of rows that hold all its columns.  This is believed to be the set and the order mlxtend produces (its generator
    extends each sorted combination by the larger items in order, its support is np.sum(...) / rows); NOBODY HAS CHECKED THAT
    AGAINST MLXTEND.  There is no subset prune and no max_len.
  * sort_by_cost is np.argsort(c) with NumPy's default sort, which is not stable; here the order is defined as kind='stable'.
  * `model.T[i]` is in ascending row order (the reference: find_hyper's queue order) and `model.I[i]` in ascending column order
    (the reference: the iteration order of a frozenset); both are sets.

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any min_support, any shape
whose candidates fit: two bit matrices of m_pad x n_pad bits and 3 * candidates * m_pad / 8 bytes of tidsets and T rows (refused with
the candidate count otherwise), one GPU.  After a fit: T, I (lists of int lists), U, V (lil), k and logs['updates'] with k, iter,
shape and the metric columns -- what HyperPlus imports.  task='prediction' raises NotImplementedError.
"""
from __future__ import annotations

import numpy as np

from .BooleanModel import BooleanModel


class Hyper(BooleanModel):
    title = "Hyper"

    def __init__(self, min_support):
        self.check_params(min_support=min_support)

    def _engine_class(self):
        from ..hyper import HyperEngine
        return HyperEngine

    def _fit(self):
        from ..bitset import bit_positions
        eng = self._engine
        mined = eng.mine(self.min_support)
        if len(mined) == 0:
            print("[W] No itemset discovered outside singletons. Try to decrease min_support.")
        else:
            print(f"[I] Found {len(mined)} itemsets, max size: {max(len(I) for I in mined)}")
        items = [[j] for j in range(self.n)] + [sorted(int(j) for j in I) for I in mined]      # candidate id -> itemset
        n_i = np.array([len(I) for I in items], dtype=np.int64)

        def cost(nT, s, ids):
            """The reference's (len(T) + len(I)) / X_rs[T, I].sum() in fp64; inf for an empty T."""
            with np.errstate(divide="ignore", invalid="ignore"):
                c = (nT[ids] + n_i[ids]).astype(np.float64) / s[ids].astype(np.float64)
            return np.where(nT[ids] == 0, np.inf, c)

        # init_transactions on X, sort_by_cost
        nT, s = eng.evaluate_all()
        live = np.nonzero(nT > 0)[0]              # the list, as candidate ids in list order
        known_nT, known_s = nT.copy(), s.copy()   # the record every candidate was last evaluated with
        c = cost(known_nT, known_s, live)
        pending = set(int(i) for i in live)       # evaluated on this residual, T not committed yet

        def sort():
            nonlocal live, c
            order = np.argsort(c, kind="stable")
            live, c = live[order], c[order]

        def evaluate_head():
            if len(live) == 0:
                raise IndexError("list index out of range")
            h = live[0]
            known_nT[h], known_s[h] = nT[h], s[h]
            c[0] = cost(known_nT, known_s, live[:1])[0]
            pending.add(int(h))

        sort()
        self.T, self.I = [], []
        k = 0
        for _ in range(len(live)):
            evaluate_head()
            while known_nT[live[0]] == 0:
                live, c = live[1:], c[1:]
                if len(live) == 0:
                    raise IndexError("list index out of range")
            n_iter = 0
            while True:
                if len(live) < 2:
                    raise IndexError("list index out of range")
                if not c[0] > c[1]:
                    break
                sort()
                evaluate_head()
                n_iter += 1
            eng.commit(pending)
            pending.clear()
            h = int(live[0])
            T = [int(t) for t in bit_positions(eng.apply(h)) if t < self.m]
            self.T.append(T)
            self.I.append(list(items[h]))
            u, v = np.zeros((self.m, 1)), np.zeros((self.n, 1))
            u[T], v[items[h]] = 1, 1
            self.set_factors(k, u=u, v=v)
            self._invalidate()
            self.evaluate(df_name='updates', head_info={'k': k, 'iter': n_iter, 'shape': [len(T), len(items[h])]})
            if eng.residual_sum() == 0:
                break
            nT, s = eng.evaluate_all(live)
            evaluate_head()
            sort()
            k += 1
        self.k = self.U.shape[1]
