"""Panda -- PaNDa / PaNDa+, top-k noisy patterns by description length.  Drop-in for ``PyBMF/models/Panda.py`` (Mining Top-K Patterns
from Binary Datasets in presence of Noise; A unifying framework for mining approximate top-k binary patterns).

The only model of the combinatorial family that minimises  w_model (|U| + |V|) + w_fp FP + w_fn FN.  Each factor is a dense core
(T, I) of the residual X_rs -- the items of the extension list E are walked in order and one joins I when that does not raise the
cost -- which is then extended: an item of E joins I when the cost allows it, and after each such item every transaction outside T
that does not raise the cost joins T.  All of that is AND-popcounts over bit rows in HBM with a scalar fp64 decision (csrc/panda.hip
through ``pybmf_amd/panda.py``): the device returns positions, integers and bits; the orderings of E, the running cost (the reference's
own fp64 expressions on those integers, products and sums in its order), the log and the stops are host control flow.

The order of E is defined here: np.flip(np.argsort(scores, kind='stable')) applied to E in its current order -- score descending,
and among equal scores the element LATER in the current E first.  E's order carries over from sort to sort, so a re-sort with the
same scores reverses every tie group.  init_method='correlation' re-sorts E by |T & rs_e| before every test of E[0]; once E[0] is
rejected nothing changes any more and the reference only goes on re-sorting, once per element left: here the ordering is applied
once more iff len(E) - 1 is odd, which leaves E as the reference's loop leaves it.

Kept from the reference, on purpose:
  * early_stop(error, n_factor=self.n_factors, k=k) is called before n_factors is incremented: k requested factors yield k + 1.
  * error <= tol truncates U, V to k columns -- the factor just logged is dropped -- and ends the loop.
  * the "error starts increasing" test is cost_now - w_model (|T| + |I|) > cost_old; a cost that merely increased only prints.
  * exact_decomp forces w_model = 0 and 'frequency' and skips the extension.
  * cost_old starts at w_fn * sum(X), not at the description length of the empty model.
Different from the reference:
  * the order inside tie groups.  The reference calls np.argsort with NumPy's default sort, which is not stable: the result inside
    a tie group depends on the host's sort kernel.  Every order it can produce agrees with the defined one once the scores are
    mapped through it.
  * the two stops that carry a message ("Error starts increasing.", "No pattern found.") raise a TypeError inside the reference's
    own early_stop (it calls _early_stop without `verbose`); here they work and leave the factors found so far.

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any number of factors, any
shape whose six bit matrices device memory holds, one GPU.  task='prediction' raises NotImplementedError, as for MEBF.
fit(..., block=N) sets the number of candidates per scan launch of the two sweeps (default: all that remain); every value gives
the same result.  The correlation rounds always score all of E: the pick is a maximum over the whole list.
"""
from __future__ import annotations

import numpy as np

from .BooleanModel import BooleanModel


def order_of(scores):
    """The defined order of a score vector: score descending, among equal scores the LATER position first."""
    return np.flip(np.argsort(np.asarray(scores), kind="stable"))


class Panda(BooleanModel):
    title = "Panda"

    def __init__(self, k=None, tol=0, w_model=1, w_fp=1, w_fn=1, init_method='correlation', exact_decomp=False):
        self.check_params(k=k, tol=tol, w_model=w_model, w_fp=w_fp, w_fn=w_fn, init_method=init_method, exact_decomp=exact_decomp)

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        assert self.init_method in ['frequency', 'couples-frequency', 'correlation']
        if self.exact_decomp:
            print("[I] Exact decomposition mode.")
            self.w_model = 0
            self.init_method = 'frequency'

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._block = kwargs.pop("block", None)
        super().fit(X_train, X_val, X_test, **kwargs)

    def _engine_class(self):
        from ..panda import PatternEngine
        return PatternEngine

    # ---- the reference's fp64 expressions on the device's integers --------------------------------------------------------
    def _core_d_cost(self, w0, h0, h1):
        """find_core: the cost difference of item number w0 + 1 shrinking T from h0 to h1 transactions."""
        w0, h0, h1 = np.float64(w0), np.float64(h0), np.float64(h1)
        w1 = w0 + 1
        return self.w_model * ((w1 + h1) - (w0 + h0)) - self.w_fn * ((w1 * h1) - (w0 * h0))

    def _item_cost(self, cost_old, n_t, a, b):
        """extend_core: the cost with one more item, a = |T & rs_e|, b = |T & pd_e|."""
        partial_fn = -np.float64(a)
        partial_fp = np.float64(n_t) - np.float64(b) + partial_fn
        return cost_old + self.w_model * 1 + self.w_fp * partial_fp + self.w_fn * partial_fn

    def _rows_d_cost(self, added, sum_d_fn, sum_d_fp):
        """extend_core: the sum of w_model + (w_fn d_fn + w_fp d_fp) over the transactions that joined, from the integer sums."""
        return self.w_model * np.float64(added) + (self.w_fn * np.float64(sum_d_fn) + self.w_fp * np.float64(sum_d_fp))

    def _block_of(self, left):
        return left if not self._block else min(int(self._block), left)

    # ---- one factor ---------------------------------------------------------------------------------------------------
    def find_core(self):
        """A dense core (T on the device, self.I, self.n_T) and the extension list self.E in the order extend_core walks."""
        eng = self._engine
        method = 'frequency' if self.init_method == 'frequency' else 'couples-frequency'
        E = np.arange(self.n)
        E = E[order_of(eng.scores(method))]
        first, E = int(E[0]), E[1:]
        self.I, h0 = [first], eng.start_core(first)
        fp, fn = eng.error_counts()
        cost = self.w_model * np.float64(eng.factor_cells() + h0 + 1) + self.w_fp * np.float64(fp) + self.w_fn * np.float64(fn - h0)
        if self.init_method == 'correlation':
            while len(E):
                eng.set_candidates(E)
                i, h1, scores = eng.core_scan(0, len(E), 1, self.w_model, self.w_fn, len(self.I), h0, want_scores=True)
                idx = order_of(scores)
                E, scores = E[idx], scores[idx]
                if i < 0:
                    if (len(E) - 1) % 2 == 1:          # the reference re-sorts once per element left: tie groups end reversed
                        E = E[order_of(scores)]
                    break
                assert idx[0] == i and scores[0] == h1
                cost = cost + self._core_d_cost(len(self.I), h0, h1)
                self.I.append(int(E[0]))
                E, h0 = E[1:], h1
        else:
            eng.set_candidates(E)
            pos, taken = 0, []
            while pos < len(E):
                count = self._block_of(len(E) - pos)
                i, h1, _ = eng.core_scan(pos, count, 0, self.w_model, self.w_fn, len(self.I), h0)
                if i < 0:
                    pos += count
                    continue
                cost = cost + self._core_d_cost(len(self.I), h0, h1)
                self.I.append(int(E[pos + i]))
                taken.append(pos + i)
                pos, h0 = pos + i + 1, h1
            E = np.delete(E, taken)
        self.E, self.n_T, self.cost_now = [int(e) for e in E], h0, cost
        eng.set_items(self.I)

    def extend_core(self):
        """Items of E join I in E's order while the cost allows; after each, the transactions outside T that the cost allows join T."""
        eng = self._engine
        E, cost, pos = self.E, self.cost_now, 0
        eng.set_candidates(E)
        while pos < len(E):
            count = self._block_of(len(E) - pos)
            r = eng.ext_scan(pos, count, self.n_T, len(self.I) + 1, self.w_model, self.w_fp, self.w_fn, float(cost))
            if r["i"] < 0:
                pos += count
                continue
            cost = self._item_cost(cost, self.n_T, r["a"], r["b"])
            self.I.append(int(E[pos + r["i"]]))
            if r["added"] > 0:
                cost = cost + self._rows_d_cost(r["added"], r["sum_d_fn"], r["sum_d_fp"])
                self.n_T += r["added"]
            pos += r["i"] + 1
        self.cost_now = cost

    def _fit(self):
        from ..bitset import unpack_bits
        eng = self._engine
        cost_old = self.w_fn * np.float64(eng.sum_x)
        k = 0
        self.n_factors = 0
        is_improving = True
        while is_improving:
            desc = f"[I] k: {k} - [{cost_old}]"
            self.find_core()
            desc += f" -> [{self.cost_now}]"
            if not self.exact_decomp:
                self.extend_core()
                desc += f" -> [{self.cost_now}]"
            self.print_msg(desc[4:])
            n_t, n_i = self.n_T, len(self.I)
            if self.cost_now > cost_old:
                print("[W] Cost increased.")
            if self.cost_now - self.w_model * np.float64(n_t + n_i) > cost_old:
                is_improving = self.early_stop(msg="Error starts increasing.", k=k)
                continue
            cost_old = self.cost_now
            if n_t == 0 or n_i == 0:
                is_improving = self.early_stop(msg="No pattern found.", k=k)
                continue
            u_bits, v_bits = eng.apply_core()
            u, v = unpack_bits(u_bits, self.m), unpack_bits(v_bits, self.n)
            self.set_factors(k, u=u.astype(np.float64)[:, None], v=v.astype(np.float64)[:, None])
            self._invalidate()
            self.evaluate(df_name='updates', head_info={'cost': self.cost_now, 'shape': [int(n_t), int(n_i)]})
            error = self._train_error()
            is_improving = self.early_stop(error=error, n_factor=self.n_factors, k=k)
            k += 1
            self.n_factors += 1
