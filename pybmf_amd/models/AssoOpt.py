"""AssoOpt -- an Asso model's U refined by exhaustive search over each row.  Drop-in for ``PyBMF/models/AssoOpt.py``.

``AssoOpt(model, w_fp=1, w_fn=1)`` imports k, U, V and the logs of a fitted model.  fit() gives every row i of U the subset j of the k
factors whose Boolean sum scores best against X[i, :]: score_j = -w_fp FP + w_fn TP, j = 0 .. 2^k - 1 with factor 0 the most
significant bit of j, the first of equals (np.argmax).  On the device a workgroup per row walks all 2^k subsets over the bit rows of V
in LDS (csrc/asso_refine.hip through ``pybmf_amd/asso_refine.py``); TP and FP are exact integers and the score is the expression above
on them, so the chosen j are the reference's.  ``chosen`` holds j per row after the fit.

Different from the reference: there the fit dies after U is final and before anything is logged (AttributeError: 'AssoOpt' object has
no attribute 'w').  Here it finishes: score = the coverage score of the new prediction with the model's weights, one row of
logs['refinements'] with train score and the default metrics.  The imported model's own U is left as it was; the refined U is a new
lil matrix.

Supported: Boolean X, task='reconstruction' with or without X_val / X_test, k <= 16 (2^k subsets per row; beyond that
NotImplementedError), one GPU.  task='prediction' and non-Boolean data raise NotImplementedError; a model whose k is None raises
TypeError.
"""
from __future__ import annotations

import time

import numpy as np

from .AssoIter import AssoRefiner


class AssoOpt(AssoRefiner):
    title = "AssoOpt"

    def __init__(self, model, w_fp=1, w_fn=1):
        self.check_params(model=model, w_fp=w_fp, w_fn=w_fn)

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        from ..asso_refine import K_MAX_ROWS
        if self.k is not None and self.k > K_MAX_ROWS:
            raise NotImplementedError(f"k = {self.k}: AssoOpt searches 2^k subsets per row, k <= {K_MAX_ROWS}")
        super().fit(X_train, X_val, X_test, **kwargs)

    def _refine(self):
        w_fp, w_fn = self._weights()
        tic = time.perf_counter()
        _, tp, fp, _ = self._engine.optimal_rows(w_fp, w_fn)
        toc = time.perf_counter()
        print("[I] Exhaustive search finished in {}s.".format(toc - tic))
        self.chosen = self._engine.chosen()
        self._invalidate()
        score = -w_fp * np.float64(fp) + w_fn * np.float64(tp)
        self.evaluate(df_name='refinements', train_info={'score': score})
