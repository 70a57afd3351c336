"""NMFSklearn -- scikit-learn's NMF with the coordinate-descent solver and the Frobenius loss, on the GPU.

Counterpart of ``PyBMF/models/NMFSklearn.py``: same constructor; the reference hands X to ``sklearn.decomposition.NMF`` (``solver='cd'``,
``shuffle=False``, no regularisation).  What that call does is restated here without scikit-learn:

* the solver (``_fit_coordinate_descent``): per iteration a sweep over the rows of U with V held, then one over the rows of V with the
  new U -- ``bmf_nmf_cd_iterate`` (csrc/nmf_cd.hip through ``pybmf_amd/nmf.py``); the stopping rule on the sum of the projected
  gradients ("violation") relative to the first iteration's runs on the host;
* the initialisers (``_initialize_nmf``): 'random' on the host; 'nndsvd', 'nndsvda', 'nndsvdar' from a randomised truncated SVD
  (``_randomized_svd``) whose products with X and X^T run on the device and whose LU / QR / small SVD run on the host with SciPy.

Supported: Boolean X, k <= 64, one GPU.  ``solver='mu'``, the other beta losses and ``init_method=None`` are refused.
"""
from __future__ import annotations

import types
import warnings

import numpy as np

from ..utils import to_dense, to_sparse
from .ContinuousModel import ContinuousModel


# ---- the initialisers: host arithmetic around `product(T, transposed)` = X @ T, or X^T @ T when transposed ----------------------------

def random_init(shape, x_mean, k, rng):
    """(W, H) of init='random': H is drawn before W."""
    m, n = shape
    avg = np.sqrt(x_mean / k)
    H = avg * rng.standard_normal(size=(k, n))
    W = avg * rng.standard_normal(size=(m, k))
    return np.abs(W), np.abs(H)


def randomized_svd(shape, k, rng, product):
    """(U, S, Vt) of the k leading singular triplets of X (m x n), Halko et al.'s range finder as scikit-learn runs it: 10 extra
    columns, 7 power iterations (4 when k >= 0.1 min(m, n)) each normalised by an LU factorisation, a QR at the end, the SVD of the
    projected thin matrix, signs fixed so that the largest entry of every left singular vector of the matrix worked on is positive.
    The matrix worked on is X^T when m < n."""
    from scipy import linalg
    m, n = shape
    n_random = k + 10
    n_iter = 7 if k < 0.1 * min(m, n) else 4
    transpose = m < n
    # A = X^T if transpose else X:  A @ Q = product(Q, transpose),  A^T @ Q = product(Q, not transpose)
    Q = rng.normal(size=(m if transpose else n, n_random))
    for _ in range(n_iter):
        Q, _ = linalg.lu(product(Q, transpose), permute_l=True, check_finite=False)
        Q, _ = linalg.lu(product(Q, not transpose), permute_l=True, check_finite=False)
    Q, _ = linalg.qr(product(Q, transpose), mode="economic", check_finite=False)
    B = product(Q, not transpose).T   # Q^T A
    Uhat, s, Vt = linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    U = Q @ Uhat
    if not transpose:
        signs = np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])
    else:
        signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    U, Vt = U * signs[np.newaxis, :], Vt * signs[:, np.newaxis]
    if transpose:
        return Vt[:k, :].T, s[:k], U[:, :k].T
    return U[:, :k], s[:k], Vt[:k, :]


def nndsvd_init(shape, x_mean, k, variant, rng, product, eps=1e-6):
    """(W, H) of init='nndsvd' / 'nndsvda' / 'nndsvdar' (Boutsidis & Gallopoulos 2008): of every singular pair past the first the
    larger of the positive and the negative part is kept; entries below eps become 0 and are then left (nndsvd), set to the mean of
    X (a) or to small random values (ar, W before H)."""
    m, n = shape
    if k > min(m, n):
        raise ValueError(f"init_method={variant!r} needs k <= min(m, n) = {min(m, n)}, got k = {k}")
    U, S, Vt = randomized_svd(shape, k, rng, product)
    left, right = U, Vt.T                                  # singular vectors as columns: m x k and n x k
    # every pair split into its non-negative and its non-positive part at once; the norms of the four parts of a pair as vectors
    parts = {sign: (np.maximum(sign * left, 0.0), np.maximum(sign * right, 0.0)) for sign in (1.0, -1.0)}
    norms = {sign: (np.sqrt((a * a).sum(axis=0)), np.sqrt((b * b).sum(axis=0))) for sign, (a, b) in parts.items()}
    weight = {sign: na * nb for sign, (na, nb) in norms.items()}
    keep_pos = weight[1.0] > weight[-1.0]                  # strict: a tie keeps the negative parts
    keep_pos[0] = True                                      # the leading pair is one-signed: both vectors by absolute value
    W, H = np.empty_like(left), np.empty_like(right)
    for j in range(k):
        if j == 0:
            W[:, 0], H[:, 0] = np.sqrt(S[0]) * np.abs(left[:, 0]), np.sqrt(S[0]) * np.abs(right[:, 0])
            continue
        sign = 1.0 if keep_pos[j] else -1.0
        (a, b), (na, nb) = parts[sign], norms[sign]
        scale = np.sqrt(S[j] * weight[sign][j])
        W[:, j], H[:, j] = scale * (a[:, j] / na[j]), scale * (b[:, j] / nb[j])
    H = np.ascontiguousarray(H.T)
    for F in (W, H):                                        # W first: 'ar' draws for W before H
        F[F < eps] = 0.0
        holes = F == 0
        if variant == "nndsvda":
            F[holes] = x_mean
        elif variant == "nndsvdar":
            F[holes] = np.abs(x_mean * rng.standard_normal(int(holes.sum())) / 100)
    return W, H


class NMFSklearn(ContinuousModel):
    def __init__(self, k, U=None, V=None, beta_loss='frobenius', init_method='nndsvd', solver='cd', tol=1e-4, max_iter=1000, seed=None):
        self.check_params(k=k, U=U, V=V, beta_loss=beta_loss, init_method=init_method, solver=solver, tol=tol, max_iter=max_iter, seed=seed)

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        assert self.solver in ['cd', 'mu']
        assert self.beta_loss in ['frobenius', 'kullback-leibler', 'itakura-saito']
        assert self.init_method in [None, 'random', 'nndsvd', 'nndsvda', 'nndsvdar', 'custom']
        if self.solver == 'mu':
            raise NotImplementedError("NMFSklearn: solver='mu' is not built (scikit-learn's multiplicative update is not the WNMF "
                                      "update of this package); use solver='cd', or the WNMF model")
        if self.beta_loss != 'frobenius':
            raise NotImplementedError(f"NMFSklearn: beta_loss={self.beta_loss!r} needs scikit-learn's multiplicative-update solver, which "
                                      "is not built; WNMF has a Kullback-Leibler loss of its own")
        if self.init_method is None:
            raise NotImplementedError("NMFSklearn: init_method=None (scikit-learn's choice between 'nndsvda' and 'random') is not "
                                      "built; name the initialiser")
        if self.k is None or self.k > 64:
            raise NotImplementedError(f"NMFSklearn: k={self.k}: the coordinate-descent kernel holds a row of k <= 64 values")
        if int(self.max_iter) < 1:
            raise ValueError("NMFSklearn: max_iter must be at least 1")

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._refuse_sharded()
        super().fit(X_train, X_val, X_test, **kwargs)
        if not self._boolean:
            raise NotImplementedError("this model's GPU path takes a Boolean (0/1) matrix")
        self._engine = self._make_engine()
        self._fit()
        self.X_pd = None   # the 0.5 / 0.5 threshold prediction, built on first access
        self.finish(show_logs=self.show_logs, save_model=self.save_model, show_result=self.show_result)

    @staticmethod
    def _refuse_sharded():
        try:
            import torch.distributed as dist
        except ImportError:
            return
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("NMFSklearn runs on one GPU: a sweep of V needs X^T U over all rows, and no exchange is built for it")

    def _make_engine(self):
        from ..nmf import NMFEngine
        return NMFEngine(self._bits, self.k)

    def _make_X_pd(self):
        from ..device_ops import boolean_product_csr
        return boolean_product_csr(np.asarray(to_dense(self.U)), np.asarray(to_dense(self.V)), u=0.5, v=0.5, device=self.device)

    def _initial_factors(self):
        """(W, H) as scikit-learn's _check_w_h leaves them."""
        shape = (self.m, self.n)
        if self.init_method == 'custom':
            W, H = np.array(to_dense(self.U), dtype=np.float64), np.array(to_dense(self.V), dtype=np.float64).T
            if W.shape != (self.m, self.k) or H.shape != (self.k, self.n):
                raise ValueError(f"init_method='custom': U, V of shapes {W.shape}, {H.T.shape}, expected {(self.m, self.k)}, {(self.n, self.k)}")
            if not (np.isfinite(W).all() and np.isfinite(H).all()) or W.min() < 0 or H.min() < 0 or W.max() == 0 or H.max() == 0:
                raise ValueError("init_method='custom': U and V must be finite, non-negative and not all zero")
            return W, H
        if self.init_method == 'random':
            return random_init(shape, self._x_mean, self.k, self.rng)
        return nndsvd_init(shape, self._x_mean, self.k, self.init_method, self.rng, self._engine.product)

    def _fit(self):
        eng = self._engine
        W, H = self._initial_factors()
        self.U_init, self.V_init = W.copy(), H.T.copy()
        eng.load_factors(W, np.ascontiguousarray(H.T))
        tol, max_iter = float(self.tol), int(self.max_iter)
        n_iter, violation_init = 0, None
        for it in range(max_iter):
            eng.iterate(it)
            vu, vv = eng.row(it)
            violation = 0.0 + vu + vv
            n_iter = it + 1
            if it == 0:
                violation_init = violation
            if violation_init == 0:
                break
            if violation / violation_init <= tol:
                break
        if n_iter == max_iter and tol > 0:
            warnings.warn(f"NMFSklearn: maximum number of iterations {max_iter} reached; increase max_iter to improve convergence",
                          RuntimeWarning)
        U, V = eng.factors()
        self.n_iter_ = n_iter
        self.model = types.SimpleNamespace(n_iter_=n_iter, components_=V.T.copy(), n_components_=self.k,
                                           reconstruction_err_=float(np.sqrt(max(eng.rec_error(), 0.0))))
        self.U, self.V = to_sparse(U), to_sparse(V)
