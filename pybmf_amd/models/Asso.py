"""Asso -- the baseline of Boolean matrix factorization.  Drop-in for ``PyBMF/models/Asso.py`` (The discrete basis problem).

Candidate basis rows come from the column associations: row i of the candidate matrix is (X^T X)[i, :] / (X^T X)[i, i] > tau.  Every
factor is the candidate whose best column vector raises the coverage score w_fn TP - w_fp FP of the prediction the most; a row of X
takes the candidate when its own score rises.  Building the candidates and scoring all of them against the current prediction are
AND-popcount contractions over bit matrices in HBM (csrc/asso.hip through ``pybmf_amd/asso.py``); the loop over factors, the log and
the stopping rules are host control flow as in the reference.  Counts are exact integers; the per-row decision is the reference's own
fp64 expression on them, so factors and shapes are the reference's, and so is the score whenever the weights' products with the
counts are exact in fp64 (0.5 / 0.5, 1 / 1 ...); with other weights the score differs from the reference's in the order of its sum
only (last bits).

Kept from the reference, on purpose:
  * a sweep keeps the candidate with the largest score above best_score, the first of equals; best_score starts at 0 and is
    inherited from factor to factor: it is the coverage score of the whole prediction, not a gain.
  * early_stop(error=..., k=k) is given the factor INDEX: when error <= tol fires, truncate_factors(k) drops the factor that was
    just added, and its candidate does not return to the list.  The reference then overwrites that stop's answer with the one of
    early_stop(n_factor=k + 1): without a requested k the fit goes on from the truncated factors -- the next factor lands in column
    k + 1 behind an empty column k -- with best_score still inherited, until no candidate is left or none improves it.
Different from the reference: its two message stops ("Candidate list is empty", "No pattern found.") fail with a TypeError inside its
own early_stop (it calls _early_stop without `verbose`); here they work and leave the factors found so far.

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any number of factors, one GPU;
no row limit beyond device memory.  task='prediction' and basis_dim=0 (the reference's TransposedModel) raise NotImplementedError.
fit(..., block=N) sets the number of candidates per launch (default: all that remain); every value gives the same result.
"""
from __future__ import annotations

import numpy as np

from .BooleanModel import BooleanModel

METRICS = ['TP', 'TPR', 'FP', 'FPR', 'FN', 'FNR', 'ERR', 'ACC', 'Recall', 'Precision', 'F1']


class Asso(BooleanModel):
    title = "Asso"

    def __init__(self, tau, k=None, tol=0, w_fp=0.5, w_fn=None):
        self.check_params(tau=tau, k=k, tol=tol, w_fp=w_fp, w_fn=w_fn)

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._block = kwargs.pop("block", None)
        if kwargs.pop("basis_dim", 1) != 1:
            raise NotImplementedError("Asso builds its candidates from the columns of X (basis_dim=1): the transposed model is not built")
        super().fit(X_train, X_val, X_test, **kwargs)

    def _engine_class(self):
        from ..asso import AssoEngine
        return AssoEngine

    def _fit(self):
        from ..bitset import unpack_bits
        eng = self._engine
        w_fp = self.w_fp
        w_fn = 1 - w_fp if self.w_fn is None else self.w_fn
        n_basis = eng.build_basis(self.tau)
        print("[I] tau: {}, candidates: {}".format(self.tau, n_basis))
        k = 0
        best_score = 0
        is_improving = True
        while is_improving:
            if eng.list.size == 0:
                is_improving = self.early_stop(msg="Candidate list is empty", k=k)
                break
            hit = eng.best(best_score, w_fp, w_fn, block=self._block)
            if hit is None:
                is_improving = self.early_stop(msg="No pattern found.", k=k)
                break
            _, cand, best_score, _, _ = hit
            u_bits, v_bits = eng.column(cand, w_fp, w_fn)
            u, v = unpack_bits(u_bits, self.m), unpack_bits(v_bits, self.n)
            self.set_factors(k, u=u.astype(np.float64)[:, None], v=v.astype(np.float64)[:, None])
            while eng.n_factors < k:        # columns a tolerance stop emptied: the engine's factors stay aligned with U, V
                eng.apply(np.zeros_like(u_bits), np.zeros_like(v_bits))
            eng.apply(u_bits, v_bits)
            eng.remove(cand)
            self._invalidate()
            tp, fp, fn, _ = self._counts_of("train")
            score_half = -0.5 * np.float64(fp) + 0.5 * np.float64(tp)
            desc_len = 1 * (self.U.sum() + self.V.sum()) + 1 * np.float64(fp) + 1 * np.float64(fn)
            n_u, n_v = int(u.sum()), int(v.sum())
            self.evaluate(df_name='updates', head_info={'k': k},
                          train_info={'score': best_score, 'score_0.5': score_half, 'desc_len': desc_len, 'shape': [n_u, n_v]},
                          metrics=METRICS, verbose=self.verbose)
            error = self._train_error()
            print("[I] k: {}, score: {}, error: {:.3f}, shape: [{}, {}]".format(k, best_score, error, n_u, n_v))
            if not self.early_stop(error=error, k=k):
                eng.truncate(k)                 # U, V lost factor k: so does the prediction
                self._invalidate()
            is_improving = self.early_stop(n_factor=k + 1)   # (the reference keeps only this answer)
            k += 1
