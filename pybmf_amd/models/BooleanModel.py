"""What the combinatorial Boolean models share (GreConD, GreConD+, Asso, AssoIter, AssoOpt, MEBF, Panda): a fit on Boolean matrices
whose state is bit sets on the device behind a host engine (``pybmf_amd/bitset.py``), scored from that engine's integer counts.

A model names its engine (``_engine_class``), takes its own keywords out of ``fit()`` before it hands over to this one, and writes
``_fit``.  ``_make_engine`` is the one place an engine is made: a test that runs a model without a GPU overrides exactly that.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import lil_matrix

from .BaseModel import BaseModel
from .ContinuousModel import ContinuousModel


class BooleanModel(BaseModel):
    device = "cuda:0"
    title = None        # the model's name in messages

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        if kwargs.get("task", getattr(self, "task", None)) == "prediction":
            raise NotImplementedError(f"{self.title} scores whole matrices (task='reconstruction'): the scorer of stored entries takes "
                                      "factor panels of at most 128 columns, not the prediction bits this model keeps")
        super().fit(X_train, X_val, X_test, **kwargs)
        self._engine = self._make_engine()
        self._invalidate()
        self._fit()
        self.finish(show_logs=self.show_logs, save_model=self.save_model, show_result=self.show_result)

    def _init_factors(self):
        """lil factors, k columns or one (BaseModelTools.py:275-286 of the reference)."""
        if hasattr(self, "U") or hasattr(self, "V"):
            print("[I] U, V existed. Skipping initialization.")
            return
        k = self.k if getattr(self, "k", None) is not None else 1
        self.U, self.V = lil_matrix((self.m, k)), lil_matrix((self.n, k))

    def _engine_class(self):
        raise NotImplementedError

    def _make_engine(self):
        from ..engine import BitMatrix
        for X in (self._X_input, self.X_val, self.X_test):
            if X is not None and not ContinuousModel._values_are_boolean(X):
                raise NotImplementedError(f"{self.title} takes Boolean (0/1) matrices")
        bits = BitMatrix(self._X_input, self.device)
        if bits.max_u8 > 1:
            raise NotImplementedError(f"{self.title} takes Boolean (0/1) matrices")
        extra = {name: BitMatrix(X, self.device) for name, X in (("val", self.X_val), ("test", self.X_test)) if X is not None}
        return self._engine_class()(bits, extra)

    # ---- scores --------------------------------------------------------------------------------------------------
    def _invalidate(self):
        """The prediction changed: the counts are asked for again, X_pd is rebuilt from the device bits on first access."""
        self._counts, self.X_pd = {}, None

    def _counts_of(self, name):
        if name not in self._counts:
            self._counts[name] = self._engine.counts(name)
        return self._counts[name]

    def _train_error(self):
        """ERR of the prediction on the training matrix: 1 - (TP + TN) / (m n)."""
        tp, _, _, tn = self._counts_of("train")
        return 1 - np.float64(tp + tn) / (self.m * self.n)

    def _score(self, name, metrics):
        """Data set `name` against X_pd, from the integer counts of the prediction bits on the device."""
        if name != "train" and getattr(self, "X_" + name) is None:
            raise ValueError(f"no {name} data was given to fit()")
        if any(mt in ("RMSE", "MAE") for mt in metrics):
            raise NotImplementedError(f"{self.title} scores the Boolean metrics only")
        return ContinuousModel._metric_values(metrics, None, self._counts_of(name))

    def _make_X_pd(self):
        """The prediction as the device holds it, as csr."""
        return self._engine.prediction()
