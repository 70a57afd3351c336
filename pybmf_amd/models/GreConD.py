"""GreConD -- exact Boolean decomposition by greedy concept search.  Drop-in for ``PyBMF/models/GreConD.py`` (Discovery of optimal
factors in binary data via a novel method of matrix decomposition).

Each factor is a formal concept (u, v) of X: a maximal rectangle of ones, grown column by column to cover as many still-uncovered
ones (the residual X_rs) as possible.  The search is intersections, subset tests and popcounts over the columns of X as bit rows in
HBM (csrc/grecond.hip through ``pybmf_amd/grecond.py``); the loop over factors, the log and the stopping rules are host control flow
as in the reference.  There is no floating point in the search: factors, scores and shapes are the reference's, integer for integer.

Kept from the reference, on purpose:
  * get_concept replaces its best concept INSIDE a sweep over the columns (strict >, ascending column order), so this is not the
    textbook "best of the sweep" GreConD.
  * early_stop(error=..., k=k) is given the factor INDEX: when error <= tol fires, truncate_factors(k) drops the factor that was
    just added from U and V, while X_pd and the last log row still include it.  "Reach requested factor" does not truncate.
Different from the reference: when no pattern is left (score 0; an all-zero X at the first call) the reference's own early_stop
fails with a TypeError (it calls _early_stop without `verbose`); here that stop works and leaves the k factors found so far.

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any number of factors (the
prediction is kept as bits and updated per factor: no 64 / 128-column limit), up to 32256 rows, one GPU.  task='prediction' raises
NotImplementedError: the entry scorer (engine.ObservedScorer) reads factor bit panels of at most 128 columns, not prediction bits.
fit(..., block=N) sets the number of candidates per speculative launch (default: all that remain in the sweep); every value gives
the same result.
"""
from __future__ import annotations

import numpy as np

from .BooleanModel import BooleanModel


class GreConD(BooleanModel):
    title = "GreConD"

    def __init__(self, k=None, tol=0):
        self.check_params(k=k, tol=tol)

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._block = kwargs.pop("block", None)
        super().fit(X_train, X_val, X_test, **kwargs)

    def _engine_class(self):
        from ..grecond import ConceptEngine
        return ConceptEngine

    def _fit(self):
        from ..bitset import unpack_bits
        eng = self._engine
        k = 0
        is_factorizing = True
        while is_factorizing:
            score, u_bits, v_bits = eng.concept(block=self._block)
            if score == 0:
                is_factorizing = self.early_stop(msg="No pattern found", k=k)
                break
            u, v = unpack_bits(u_bits, self.m), unpack_bits(v_bits, self.n)
            self.set_factors(k, u=u.astype(np.float64)[:, None], v=v.astype(np.float64)[:, None])
            eng.apply(u_bits, v_bits)
            self._invalidate()
            n_u, n_v = int(u.sum()), int(v.sum())
            self.evaluate(df_name='updates', head_info={'k': k, 'score': score, 'shape': [n_u, n_v]})
            error = self._train_error()
            print("[I] k: {}, score: {}, error: {:.3f}, shape: [{}, {}]".format(k, score, error, n_u, n_v))
            is_factorizing = self.early_stop(error=error, n_factor=k + 1, k=k)
            k += 1
