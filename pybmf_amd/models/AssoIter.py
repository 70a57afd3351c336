"""AssoIter -- an Asso model's U refined one column at a time.  Drop-in for ``PyBMF/models/AssoIter.py``.

``AssoIter(model, w_fp=0.5, w_fn=None)`` imports k, U, V and the logs of a fitted model (a ``pybmf_amd`` Asso, the reference's, or any
object with those four attributes).  fit() then visits the columns of U in rounds, 0 .. k-1: column k is re-decided against the other
k - 1 factors -- a row takes basis V[:, k] iff its coverage score -w_fp FP + w_fn TP rises, strictly, in fp64 -- and the error of the
new prediction is compared with the best so far.  One visit is one launch of csrc/asso_refine.hip through ``pybmf_amd/asso_refine.py``:
the bit rows of V sit in LDS, the counts are exact integers, the host reads one record (score, TP, FP, |u|).

Kept from the reference, on purpose:
  * the new column is written into U whether the error falls or not; only a fall is logged (one row of logs['refinements'] with head k
    and train score, error and the default metrics) and resets the count of fruitless visits;
  * the fit ends after k fruitless visits in a row ("Error stops decreasing."), in the middle of a round if need be; a round that ends
    without that starts again at column 0;
  * score is that of the visit (the sum of the rows' chosen scores = w_fn TP - w_fp FP of the new prediction).  With weights whose
    products with the counts are exact in fp64 (0.5 / 0.5, 1 / 1 ...) it is the reference's to the bit, else it differs in the order
    of its sum only (last bits).
Different from the reference: the imported model's own U is left as it was (the reference writes into the object it shares with it);
the refined U is a new lil matrix.

Supported: Boolean X, task='reconstruction' with or without X_val / X_test, k <= 1024 factors, one GPU.  task='prediction' and
non-Boolean data raise NotImplementedError; a model whose k is None raises TypeError (the reference fails on range(None)).  An Asso
that stopped before it found its k factors has fewer columns in U and V than its k says: fit() refuses it with a ValueError that
names the shapes (fit the Asso with the k it reached, or hand over a stand-in with that k).
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import issparse, lil_matrix

from .BooleanModel import BooleanModel


def _dense(F):
    return np.asarray(F.todense()) if issparse(F) else np.asarray(F)


class AssoRefiner(BooleanModel):
    """What AssoIter and AssoOpt share: the imported model and its way into and out of the device engine; they write `_refine`."""

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        if 'model' in kwargs:
            model = kwargs.get('model')
            self.import_model(k=model.k, U=model.U, V=model.V, logs=model.logs)
            # the model itself is not kept: finish() pickles every public attribute, and a fitted pybmf_amd model holds device
            # handles (its engine) that do not pickle and device memory that should not outlive it here
            del self.model

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        if self.k is None:
            raise TypeError(f"{self.title} needs the number of factors of the imported model: its k is None")
        super().fit(X_train, X_val, X_test, **kwargs)

    def init_model(self):
        super().init_model()
        U, V = _dense(self.U), _dense(self.V)
        if U.shape != (self.m, self.k) or V.shape != (self.n, self.k):
            raise ValueError(f"the imported factors have shapes {U.shape}, {V.shape}; X is {self.m} x {self.n} and k = {self.k}")

    def _engine_class(self):
        from ..asso_refine import AssoRefineEngine
        return AssoRefineEngine

    def _fit(self):
        self._engine.load_factors(_dense(self.U), _dense(self.V))
        self._refine()
        self.U = lil_matrix(self._engine.factor_arrays()[0].astype(np.float64))

    def _weights(self):
        return self.w_fp, (1 - self.w_fp if self.w_fn is None else self.w_fn)

    def _error(self, tp, fp):
        """ERR of a prediction with these TP, FP against X_train: 1 - (TP + TN) / (m n)."""
        tn = self.m * self.n - self._engine.sum_x - fp
        return 1 - np.float64(tp + tn) / (self.m * self.n)


class AssoIter(AssoRefiner):
    title = "AssoIter"

    def __init__(self, model, w_fp=0.5, w_fn=None):
        self.check_params(model=model, w_fp=w_fp, w_fn=w_fn)

    def _refine(self):
        eng = self._engine
        w_fp, w_fn = self._weights()
        tp, fp, _, _ = self._counts_of("train")
        best_score = -w_fp * np.float64(fp) + w_fn * np.float64(tp)
        best_error = self._error(tp, fp)
        self.visits = []          # (k, error, refined or skipped) of every column visit
        n_stop = 0
        is_improving = True
        while is_improving:
            for k in range(self.k):
                score, tp, fp, _ = eng.refine_column(k, w_fp, w_fn)      # the column is written whatever the error does
                self._invalidate()
                error = self._error(tp, fp)
                self.visits.append((k, float(error), bool(error < best_error)))
                if error < best_error:
                    print("[I] Refined column i: {}, error: {:.4f} -> {:.4f}, score: {:.2f} -> {:.2f}.".format(k, best_error, error, best_score, score))
                    best_error = error
                    best_score = score
                    self.evaluate(df_name='refinements', head_info={'k': k}, train_info={'score': best_score, 'error': best_error})
                    n_stop = 0
                else:
                    n_stop += 1
                    print("[I] Skipped column i: {}.".format(k))
                    if n_stop == self.k:
                        print("[I] Error stops decreasing.")
                        is_improving = False
                        break
