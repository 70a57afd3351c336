"""FastStep -- Boolean factorisation by projected gradient descent on a logistic loss, one factor (column pair) at a time, each step a
Wolfe line search.  Drop-in for ``PyBMF/models/FastStep.py`` (FastStep: Scalable Boolean matrix decomposition).

    M = 2 X - 1,   F = sum log(1 + exp(W o (-M o (U V^T - tau)))),   X_pd = (U V^T > tau)

F, its gradient on column k and the TP / FP counts of the thresholded product are ONE streaming pass on the GPU per call
(csrc/faststep.hip through ``pybmf_amd/faststep.py``); the line search (``solvers/line_search.py``) and the loops are host control flow,
as in the reference -- quirks included: the factors start in [1e-5, 0.01], every accepted step is projected onto x >= 1e-5 and
re-evaluated there, both loops stop one count AFTER their limit (max_iter + 1 steps, max_round + 1 rounds), and the prediction is a
threshold of the real product, not the Boolean product of thresholded factors.

Supported: Boolean X, k <= 64, W = 'full' or 'mask' (the stored pattern of a csr X_train, explicit zeros included), one GPU,
task='reconstruction'.  X_val / X_test are refused (they are not scored here).
"""
from __future__ import annotations

import numpy as np

from ..solvers import line_search
from ..utils import ismat, to_dense
from .ContinuousModel import ContinuousModel


def to_interval(X, lo, hi):
    """Affine map of the values of X onto [lo, hi] (utils/common.py:163-176)."""
    lo_val, hi_val = X.min(), X.max()
    return (X - lo_val) / (hi_val - lo_val) * (hi - lo) + lo


class FastStep(ContinuousModel):
    def __init__(self, k, U=None, V=None, W='full', tau=20, solver='line-search', tol=0, min_diff=1e-2, max_round=30, max_iter=50,
                 init_method='uniform', normalize_method=None, seed=None):
        self.check_params(k=k, U=U, V=V, W=W, tau=tau, solver=solver, tol=tol, min_diff=min_diff, max_round=max_round, max_iter=max_iter,
                          init_method=init_method, normalize_method=normalize_method, seed=seed)

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        assert self.solver in ['line-search']
        assert self.init_method in ['uniform']
        assert self.normalize_method in ['balance', 'matrixwise-normalize', 'columnwise-normalize', 'matrixwise-mapping',
                                         'columnwise-mapping', None]
        if ismat(self.W):
            # (the reference's own init_W compares the array with a list of strings and raises)
            raise NotImplementedError("FastStep takes W='full' or W='mask'; a mask / weight matrix is not supported "
                                      "(the reference raises on one as well)")
        assert self.W in ['mask', 'full']

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        if X_val is not None or X_test is not None:
            raise NotImplementedError("FastStep scores the training matrix only: X_val / X_test are not supported")
        if kwargs.get("task", getattr(self, "task", None)) == "prediction":
            raise NotImplementedError("FastStep scores the whole training matrix (task='reconstruction')")
        super().fit(X_train, X_val, X_test, **kwargs)
        if self.k > 64 or getattr(self, "_sharded", False):
            raise NotImplementedError("FastStep runs on one GPU with k <= 64")
        self._start_factors()
        self._engine = self._make_engine()
        self._counts = None
        self._log_buffer = {}
        try:
            self._fit()
        finally:
            self._flush_logs()
            self._log_buffer = None
        self.X_pd = None   # (U V^T > tau) as csr, built on first access
        self.finish(show_logs=self.show_logs, save_model=self.save_model, show_result=self.show_result)

    # ---- start-up ------------------------------------------------------------------------------------------------
    def init_W(self):
        """'full': no mask.  'mask': the stored pattern of the csr training matrix, explicit zeros included, as a 0 / 1 csr matrix;
        it goes to the device as a second bit matrix (_make_engine)."""
        self._obs, self._mask_is_pattern, self._mask_pattern = None, False, None
        if self.W == 'full':
            return
        from scipy.sparse import issparse
        if not issparse(self.X_train):
            raise NotImplementedError("W='mask' needs a host matrix (ndarray / scipy sparse) to take the stored pattern from")
        if self.X_train.nnz == self.m * self.n:
            return   # every cell is stored: the all-ones mask
        pattern = self.X_train.copy()
        pattern.data = np.ones(pattern.data.shape, dtype=np.uint8)
        self._mask_pattern = pattern

    def _start_factors(self):
        """The factors of init_model mapped to [1e-5, 0.01], as in the paper (:33-35)."""
        self.U = to_interval(self.U, 1e-5, 0.01)
        self.V = to_interval(self.V, 1e-5, 0.01)

    def _make_engine(self):
        from ..engine import BitMatrix
        from ..faststep import FastStepEngine
        if not self._boolean:
            raise NotImplementedError("this model's GPU path takes a Boolean (0/1) matrix")
        mask = None if self._mask_pattern is None else BitMatrix(self._mask_pattern, self._bits.device)
        return FastStepEngine(self._bits, self.k, self.tau, self.U, self.V, mask=mask)

    # ---- objective -----------------------------------------------------------------------------------------------
    def _select(self, k):
        if getattr(self, "_k_on_device", None) != k:
            self._engine.set_factor(k)
            self._k_on_device, self._memo = k, {}

    def _eval(self, params, k, want_grad, want_counts=False):
        """(F, dF, counts) at `params` for factor k.  A point is evaluated once: the search asks for the accepted point again as
        new_fval / new_slope and as f0 / g0 of the next search (line_search.py:22-23,54-55)."""
        self._select(k)
        params = np.ascontiguousarray(params, dtype=np.float64)
        key = params.tobytes()
        hit = self._memo.get(key)
        if hit is not None and (hit[1] is not None or not want_grad) and (hit[2] is not None or not want_counts):
            return hit
        F, du, dv, tp, fp = self._engine.evaluate(params[:self.m], params[self.m:], want_grad, want_counts)
        if len(self._memo) >= 8:   # (a search revisits its last few points only)
            self._memo.pop(next(iter(self._memo)))
        hit = (F, np.concatenate([du, dv]) if want_grad else None, (tp, fp) if want_counts else None)
        self._memo[key] = hit
        return hit

    def F(self, params, k):
        """The objective with column k of the factors replaced by `params` = [u (m) | v (n)]   (:147-172)."""
        return self._eval(params, k, False)[0]

    def dF(self, params, k):
        """Its gradient on column k, [du (m) | dv (n)]   (:175-211)."""
        return self._eval(params, k, True)[1].copy()

    # ---- loops ---------------------------------------------------------------------------------------------------
    def _fit(self):
        n_round = 0
        is_factorizing = True
        while is_factorizing:
            n_round += 1
            for k in range(self.k):
                n_iter = 0
                is_improving = True
                u, v = to_dense(self.U[:, k], squeeze=True), to_dense(self.V[:, k], squeeze=True)
                x_last = np.concatenate([u, v])
                self._k_on_device = None          # other columns moved since this factor's B_k was built
                p_last = -self.dF(x_last, k=k)
                new_fval = self.F(x_last, k=k)
                while is_improving:
                    n_iter += 1
                    xk, pk = x_last, p_last
                    alpha, fc, gc, new_fval, old_fval, new_slope = line_search(f=self.F, myfprime=self.dF, xk=xk, pk=pk, args=(),
                                                                                kwargs={'k': k}, maxiter=50)
                    if alpha is None:
                        print("[W] Search direction is not a descent direction.")
                        break
                    x_last = xk + alpha * pk
                    p_last = -new_slope
                    # projection, then the gradient, the objective and the counts of X_pd at the projected point (one pass)
                    eps = 1e-5
                    x_last[x_last < eps] = eps
                    new_fval, grad, self._counts = self._eval(x_last, k, True, True)
                    p_last = -grad
                    self.U[:, k], self.V[:, k] = x_last[:self.m], x_last[self.m:]
                    self._engine.commit(k, x_last[:self.m], x_last[self.m:])
                    error_last = old_fval
                    error = new_fval   # due to projection, error might oscillate
                    diff = np.abs(error - error_last)
                    self.print_msg("    Wolfe line search iter       : {}".format(n_iter))
                    self.print_msg("    num of function evals        : {}".format(fc))
                    self.print_msg("    num of gradient evals        : {}".format(gc))
                    self.print_msg("    function value update        : {:.3f} -> {:.3f}".format(old_fval, new_fval))
                    self.evaluate(df_name='updates', head_info={'round': n_round, 'k': k, 'iter': n_iter, 'original_F': new_fval,
                                                                'projected_F': error})
                    is_improving = self.early_stop(n_iter=n_iter, diff=diff, error=error, verbose=False)
            is_factorizing = self.early_stop(n_round=n_round, error=error)

    def early_stop(self, error=None, diff=None, n_round=None, n_iter=None, n_factor=None, msg=None, k=None, verbose=True):
        is_improving = super().early_stop(error=error, diff=diff, n_iter=n_iter, n_factor=n_factor, msg=msg, k=k, verbose=verbose)
        if n_round is not None and hasattr(self, 'max_round') and n_round > self.max_round:
            self._early_stop(msg="Reach maximum round", k=k, verbose=verbose)
            is_improving = False
        return is_improving

    # ---- scores --------------------------------------------------------------------------------------------------
    def _score(self, name, metrics):
        """The training matrix against X_pd = (U V^T > tau), from the TP / FP counts of the last evaluation pass, the number of ones
        of X and the number of cells."""
        if name != "train":
            raise ValueError(f"no {name} data was given to fit()")
        if any(mt in ("RMSE", "MAE") for mt in metrics):
            raise NotImplementedError("FastStep scores the Boolean metrics only")
        counts = getattr(self, "_counts", None)
        if counts is None:   # before the first step: the counts at the factors as they stand
            x = np.concatenate([self.U[:, 0], self.V[:, 0]])
            self._k_on_device = None
            counts = self._counts = self._eval(x, 0, False, True)[2]
        tp, fp = counts
        fn = self._engine.sum_x - tp
        return self._metric_values(metrics, None, (tp, fp, fn, self.m * self.n - tp - fp - fn))

    def _make_X_pd(self):
        """(U V^T > tau) at the engine's fp64 masters (the factors of the fit), as csr."""
        self._k_on_device = None   # (the engine reuses the buffer of B_k)
        return self._engine.prediction()
