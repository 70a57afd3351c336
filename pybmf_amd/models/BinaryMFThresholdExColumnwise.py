"""BinaryMFThresholdExColumnwise -- learn one binarisation threshold PER FACTOR COLUMN (``us``, ``vs``) for given real factors U, V, by
the Wolfe line search of ``BinaryMFThreshold`` on the sigmoid-smoothed reconstruction error.  The last step of the reference's
``examples/ex05_3_FastStep.ipynb``: FastStep -> SimpleThreshold(columnwise=True, randomize=True) -> this model on its ``us``, ``vs``.

The reference's module ``PyBMF/models/BinaryMFThresholdExColumnwise.py`` is not in its tree; the scalar model, the notebook's stored
output of a run and ``get_prediction_with_threshold(us=, vs=)`` define it.  THIS BUILD'S DEFINITIONS:
  parameters  ``k, U, V, W, us, vs, lamda, min_diff, max_iter, init_method, solver, normalize_method, seed``, printed in this order
              (``min_diff : 0.001`` by default, as recorded); ``us`` / ``vs``: a scalar (broadcast) or any sequence of length k, kept as
              float64 arrays of shape (k,) -- the print shows ``us : (20,)`` as recorded.
  objective   the scalar model's F with a row vector of thresholds: F(x) = 1/2 || X - Us Vs^T ||^2, Us[i][c] = sigmoid(lamda (U[i][c] -
              us[c])), likewise Vs; x = [us, vs], 2k numbers.
  gradient    the scalar model's dF with its last sum taken per column: dF[c] = sum_i ((R Vs) * dUs)[i][c], dF[k + c] = sum_j ((R^T Us) *
              dVs)[j][c], R = X - Us Vs^T (the reference's sign).  With constant vectors the two halves sum to the scalar model's dF.
  bounds      per column: [min_i U[i][c] + 1e-6, max_i U[i][c] - 1e-6], likewise V (beyond its column's range a threshold changes nothing).
  search      ``BinaryMFThreshold._search`` unchanged: ``line_search(maxiter=50)``, ``limit_step_size``, ``early_stop(n_iter, diff)``.
  log         ``logs['updates']``: time, iter, F and the four scores per data set (no threshold columns, as recorded); row 0 is the start.
  verbose     the scalar model's four lines, then the old and new x as {:.2f} lists and alpha * pk as {:.4f}, in the recorded layout.
After ``fit``: ``us``, ``vs`` (float64 arrays), ``U``, ``V`` as given (after ``normalize_method``), ``X_pd`` at (us, vs) on first access,
``n_iter``.

F and dF are the trace form over the ones of X, a whole Armijo chain per call (``pybmf_amd/thresh_cols.py``, csrc/thresh_cols.hip).
Refused (NotImplementedError): data that is not 0 / 1, a mask or weights that leave cells unobserved, k > 64, a sharded run, a list of
ones that does not fit the memory budget of the trace form (this model has no tile-product route).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .BinaryMFThreshold import BinaryMFThreshold
from .ContinuousModel import ContinuousModel

MAX_K = 64


def as_thresholds(name, value, k):
    """A scalar or a sequence of length k as a float64 array of shape (k,)."""
    a = np.array(value, dtype=np.float64)
    if a.ndim == 0:
        return np.full(int(k), float(a))
    if a.shape != (int(k),):
        raise ValueError(f"{name} must be a scalar or a sequence of k = {k} thresholds, got shape {a.shape}")
    return a


class BinaryMFThresholdExColumnwise(BinaryMFThreshold):
    def __init__(self, k, U, V, W='mask', us=0.5, vs=0.5, lamda=100, min_diff=1e-3, max_iter=100, init_method='custom', solver="line-search",
                 normalize_method=None, seed=None):
        us, vs = as_thresholds("us", us, k), as_thresholds("vs", vs, k)
        self.check_params(k=k, U=U, V=V, W=W, us=us, vs=vs, lamda=lamda, min_diff=min_diff, max_iter=max_iter, init_method=init_method,
                          solver=solver, normalize_method=normalize_method, seed=seed)

    # ---- what is refused, before anything is uploaded ------------------------------------------------------------------------------
    def _refuse(self, X_train, X_val, X_test):
        from scipy.sparse import coo_matrix, issparse
        from ..utils import ismat
        if self.k > MAX_K:
            raise NotImplementedError(f"k={self.k}: the columnwise objective is built for k <= {MAX_K}")
        for X in (X_train, X_val, X_test):
            if X is not None and not self._values_are_boolean(X):
                raise NotImplementedError("BinaryMFThresholdExColumnwise takes Boolean (0/1) matrices: its objective is the trace form over "
                                          "the ones of X")
        try:
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        except ImportError:
            world = 1
        if world > 1:
            raise NotImplementedError("BinaryMFThresholdExColumnwise runs on one GPU: the thresholds are 2k numbers, there is nothing to shard")
        cells = int(X_train.shape[0]) * int(X_train.shape[1])
        unobserved = False
        if isinstance(self.W, str):
            if self.W == "mask":   # the pattern of stored entries; a dense array is held as the csr of its non-zeros (init_W)
                stored = X_train.nnz if issparse(X_train) else (np.count_nonzero(X_train) if isinstance(X_train, np.ndarray) else cells)
                unobserved = stored != cells
        elif ismat(self.W):
            Wc = coo_matrix(self.W)
            unobserved = not (Wc.nnz == cells and (Wc.data == 1).all())
        if unobserved:
            raise NotImplementedError("BinaryMFThresholdExColumnwise takes the all-ones mask only (W='full', or a mask / weights that observe "
                                      "every cell with weight 1): the columnwise objective has no pass over observed cells")

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._refuse(X_train, X_val, X_test)
        super().fit(X_train, X_val, X_test, **kwargs)

    # ---- thresholds <-> x --------------------------------------------------------------------------------------------------------
    def threshold_to_x(self):
        return np.concatenate([self.us, self.vs])

    def x_to_threshold(self, x_last):
        self.us, self.vs = np.array(x_last[: self.k], dtype=np.float64), np.array(x_last[self.k:], dtype=np.float64)

    def x_bounds(self):
        eps = 1e-6
        return (np.concatenate([self.U.min(axis=0) + eps, self.V.min(axis=0) + eps]),
                np.concatenate([self.U.max(axis=0) - eps, self.V.max(axis=0) - eps]))

    def _thresholds(self):
        return self.us, self.vs   # (k,) arrays: `F > thr` broadcasts them over the columns

    def evaluate_with_threshold(self, n_iter, new_fval):
        self.X_pd = None
        self.evaluate(df_name='updates', head_info={'iter': n_iter, 'F': new_fval})

    def _make_X_pd(self):
        from ..device_ops import boolean_product_csr
        return boolean_product_csr(self.U, self.V, us=self.us, vs=self.vs, device=self.device)

    def _print_step(self, xk, x_last, alpha, pk):
        self.print_msg("    threshold update             :")
        self.print_msg("      [" + ", ".join("{:.2f}".format(x) for x in xk) + "]")
        self.print_msg("    ->[" + ", ".join("{:.2f}".format(x) for x in x_last) + "]")
        self.print_msg("    threshold update direction   :")
        self.print_msg("      [" + ", ".join("{:.4f}".format(x) for x in alpha * pk) + "]")

    # ---- device side ---------------------------------------------------------------------------------------------------------------
    def _upload_factors(self):
        import torch
        from ..thresh_cols import ThreshColsEngine
        if getattr(self, "_obs", None) is not None or not self._boolean:
            raise NotImplementedError("BinaryMFThresholdExColumnwise takes a Boolean matrix under the all-ones mask only")
        if getattr(self, "_sharded", False) or getattr(self, "_rows", (0, self.m)) != (0, self.m):
            raise NotImplementedError("BinaryMFThresholdExColumnwise runs on one GPU")
        B = self._bits
        dev = B.device
        self._kp = 32 if self.k <= 32 else 64
        with torch.cuda.device(dev):
            self._Ud = torch.zeros((B.m_pad, self._kp), dtype=torch.float64, device=dev)
            self._Vd = torch.zeros((B.n_pad, self._kp), dtype=torch.float64, device=dev)
            self._Ud[: self.m, : self.k] = torch.from_numpy(np.ascontiguousarray(self.U, dtype=np.float64)).to(dev)
            self._Vd[: self.n, : self.k] = torch.from_numpy(np.ascontiguousarray(self.V, dtype=np.float64)).to(dev)
            self._stream_obj = torch.cuda.current_stream()
            self._panel_bufs = (torch.empty((1, B.m_pad), dtype=torch.int64, device=dev),
                                torch.empty((1, self._kp, B.n_pad // 32), dtype=torch.int32, device=dev),
                                torch.zeros(2, dtype=torch.int64, device=dev))
        self._stream_ptr = C.c_void_p(self._stream_obj.cuda_stream)
        self._engine = ThreshColsEngine(B, self._Ud, self._Vd, self._kp, self.m, self.n, self.k, self.lamda, self._stream_obj, self._stream_ptr)
        self._F_memo, self._dF_memo = self._engine.F_memo, self._engine.dF_memo
        # what `_search` reads of the scalar model's trace state: the points per call and the length of the last Armijo chain
        self._trace = {"max_pairs": self._engine.max_points, "last_hit": 8}

    def _prefetch(self, points):
        """line_search's announcement of its next trial steps: evaluate F at the ones not known yet, in one batch."""
        from ..thresh_cols import key_of
        todo = [p_ for p_ in points if key_of(p_) not in self._F_memo]
        if todo:
            self._engine.evaluate(todo, False)

    def F(self, params):
        """1/2 || X - Us Vs^T ||_F^2 at x = [us, vs]; a point is evaluated once per fit."""
        from ..thresh_cols import key_of
        key = key_of(params)
        if key not in self._F_memo:
            self._engine.evaluate([params], False)
        return self._F_memo[key]

    def dF(self, params):
        """The 2k-vector of the gradient, in the scalar model's sign convention; memoised like F."""
        from ..thresh_cols import key_of
        key = key_of(params)
        if key not in self._dF_memo:
            self._engine.evaluate([params], True)
        return self._dF_memo[key].copy()

    def _cover_counts(self):
        """TP / FP / FN / TN at the current (us, vs): the k-bit words of U > us and the bit-columns of V > vs are built on the device from
        the fp64 factors of the search (two bmf_thresh_panels calls), then one cover-count launch and a 16-byte read-back."""
        import torch
        from .._lib import lib, check, ptr
        if getattr(self, "_engine", None) is None or getattr(self, "_log_buffer", None) is None:
            return ContinuousModel._cover_counts(self)   # (outside fit() the host-side U, V are the truth)
        B, kp = self._bits, self._kp
        rb, cb, cnt = self._panel_bufs
        with torch.cuda.device(B.device):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            thr = torch.from_numpy(np.stack([self.us, self.vs])).to(B.device)
            check(lib.bmf_thresh_panels(ptr(self._Ud), B.m_pad, self.m, self.k, kp, ptr(thr[0]), 1, ptr(rb), None, 0, s), "bmf_thresh_panels")
            check(lib.bmf_thresh_panels(ptr(self._Vd), B.n_pad, self.n, self.k, kp, ptr(thr[1]), 1, None, ptr(cb), B.n_pad // 32, s), "bmf_thresh_panels")
            cnt.zero_()
            check(lib.bmf_cover_count(ptr(B.bits), B.m_pad, B.ldx, B.n_pad // 32, ptr(rb), ptr(cb), B.n_pad // 32, kp, ptr(cnt), None, s), "bmf_cover_count")
            tp, fp = (int(x) for x in cnt.cpu().numpy())
        fn = int(B.sum_local) - tp
        return tp, fp, fn, self.m * self.n - tp - fp - fn
