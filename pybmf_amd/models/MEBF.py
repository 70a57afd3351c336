"""MEBF -- median expansion for Boolean factorization.  Drop-in for ``PyBMF/models/MEBF.py`` (Fast and Efficient Boolean Matrix
Factorization by Geometric Segmentation).

Each factor starts from the median column (axis 0) or row (axis 1) of the residual X_rs: of the columns that still hold a residual
one, the one at the middle of the order by residual count.  That column is `a`; `b` is every column whose residual shares more than
t * |a| ones with it.  Both axes are grown and the rectangle with the lower weighted error w_fp FP + w_fn FN wins; when even that
raises the cost, the AND of the two fullest residual columns is tried (weak signal).  Scores, the median, the growth and the
candidates' confusion counts are popcount passes over bit rows in HBM (csrc/mebf.hip through ``pybmf_amd/mebf.py``); the device
returns integers and bits only.  The loop over factors, the weighted errors (the reference's own fp64 expressions on those integers,
so d_cost, cost and the choice between the axes are the reference's for any weights), the log and the stops are host control flow.

Kept from the reference, on purpose:
  * weak_signal_detection asks for get_weak_signal(axis=0) twice (the second was meant to be axis 1): one candidate, along axis 0.
    On a matrix of one column it raises IndexError.
  * early_stop(error=..., k=k) followed by early_stop(n_factor=k + 1), whose result replaces the first: error <= tol truncates U, V
    to k columns -- the factor just added is dropped -- but the loop goes on.  The next round still grows on the residual and
    measures `error` on the prediction WITH the dropped factor, scores its candidates on the truncated U, V, and only the factor
    it then sets refreshes both from U, V (which now has an empty column where the dropped factor was).  The loop ends on
    n_factor >= k or an empty residual.
  * t=None fails: the reference at `self.t * a.sum()`, here with the same TypeError before anything is computed.
Different from the reference:
  * the order of the scores.  The reference takes np.flip(np.argsort(scores)) with NumPy's default sort, which is not stable: among
    equal scores -- the norm at the median position -- the pick depends on NumPy's sort kernel and so on the host's instruction set.
    Here the order is defined: score descending, and among equal scores the higher index first, which is
    np.flip(np.argsort(scores, kind='stable')).  The pick always lies in the tie group the reference picks from.
  * the stops with a message ("No pattern found", "Cost stops decreasing") raise a TypeError inside the reference's own early_stop
    (it calls _early_stop without `verbose`); here they work and leave the k factors found so far.

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any number of factors, any
number of rows that device memory holds (six bit matrices of m_pad x n_pad bits; four more after a tolerance stop truncated a
factor), one GPU.  task='prediction' raises NotImplementedError: the entry scorer (engine.ObservedScorer) reads factor bit panels of
at most 128 columns, not prediction bits.
"""
from __future__ import annotations

import numpy as np

from .BooleanModel import BooleanModel


class MEBF(BooleanModel):
    title = "MEBF"

    def __init__(self, k=None, tol=0, t=None, w_fp=1, w_fn=1):
        self.check_params(k=k, tol=tol, t=t, w_fp=w_fp, w_fn=w_fn)

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        if self.t is None:
            raise TypeError("unsupported operand type(s) for *: 'NoneType' and 'float' (MEBF needs the threshold t)")
        super().fit(X_train, X_val, X_test, **kwargs)

    def _engine_class(self):
        from ..mebf import MedianEngine
        return MedianEngine

    # ---- the reference's fp64 expressions on the device's integers --------------------------------------------------------
    def _weighted(self, fp, fn):
        return self.w_fp * np.float64(fp) + self.w_fn * np.float64(fn)

    def _choose(self, cands):
        """(candidate, d_cost) of bidirectional_growth / weak_signal_detection: the first candidate unless the second is strictly
        better; an empty candidate costs what the prediction costs now."""
        eng = self._engine
        error = self._weighted(*eng.error_counts())
        fp, fn = eng.base_counts()
        e = [error if (c["na"] == 0 or c["nb"] == 0) else self._weighted(fp + c["dFP"], fn - c["dTP"]) for c in cands]
        i = 0 if e[0] <= e[1] else 1
        return cands[i], e[i] - error

    def truncate_factors(self, k):
        super().truncate_factors(k)
        self._cut = True

    def _kept_factors(self):
        from ..bitset import pack_bits
        eng, out = self._engine, []
        U, V = np.asarray(self.U.todense()) != 0, np.asarray(self.V.todense()) != 0
        for f in range(U.shape[1]):
            if U[:, f].any() and V[:, f].any():
                out.append((pack_bits(U[:, f], eng.W), pack_bits(V[:, f], eng.nvw)))
        return out

    def _fit(self):
        from ..bitset import unpack_bits
        eng = self._engine
        self.cost = np.float64(eng.sum_x)
        k = 0
        is_improving = True
        while is_improving:
            c, self.d_cost = self._choose(eng.growth(self.t))
            if c["na"] == 0 or c["nb"] == 0:
                is_improving = self.early_stop(msg="No pattern found", k=k)
                break
            if self.d_cost > 0:   # cost increases: fall back to a small pattern
                self.print_msg("k: {}, cost increases by {}".format(k, self.d_cost))
                w = eng.weak(self.t)
                c, self.d_cost = self._choose([w, w])
                if self.d_cost > 0:
                    is_improving = self.early_stop(msg="Cost stops decreasing", k=k)
                    break
            if c["na"] == 0 or c["nb"] == 0:
                is_improving = self.early_stop(msg="No pattern found", k=k)
                break
            u, v = unpack_bits(c["u"], self.m), unpack_bits(c["v"], self.n)
            self.set_factors(k, u=u.astype(np.float64)[:, None], v=v.astype(np.float64)[:, None])
            self.cost = self.cost + self.d_cost
            eng.apply(c["u"], c["v"], c)
            self._invalidate()
            n_u, n_v = int(u.sum()), int(v.sum())
            error = self._train_error()
            self.print_msg("k: {}, pattern: {}, d_cost: {}, cost: {}, rs: {}, err: {}".format(k, [n_u, n_v], self.d_cost, self.cost,
                                                                                           eng.residual_sum(), error))
            self.evaluate(df_name='updates', head_info={'cost': self.cost, 'shape': [n_u, n_v], 'rs': eng.residual_sum()})
            self._cut = False
            self.early_stop(error=error, k=k)            # truncates on error <= tol; its verdict is replaced by the next line's
            if self._cut:
                eng.truncate(self._kept_factors())
            is_improving = self.early_stop(n_factor=k + 1)
            if eng.residual_sum() == 0:
                break
            k += 1
