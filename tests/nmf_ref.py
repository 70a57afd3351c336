"""NumPy restatement of what ``PyBMF/models/NMFSklearn.py`` runs: scikit-learn's NMF with solver='cd', beta_loss='frobenius',
shuffle=False and no regularisation -- the coordinate-descent sweep in its literal order of operations, the loop with its stopping
rule, the 'random' and NNDSVD initialisers with the randomised SVD under them.  Pinned to scikit-learn through the reference by
tests/golden/g32_nmf (made by tests/golden/make_golden_nmf.py, which is the only place scikit-learn is imported); the CPU reference of
tests/test_nmf_cd_kernel_gpu.py and the stand-in engine of tests/test_nmf_cpu.py.  No GPU, no scikit-learn.
"""
from __future__ import annotations

import numpy as np
from scipy import linalg


# ---- the sweep -----------------------------------------------------------------------------------------------------------------

def sum_slabs(slabs):
    """XHt from the fp32 slabs of the bits GEMM: added in fp64 in slab order."""
    out = np.zeros(slabs.shape[1:], dtype=np.float64)
    for s in range(slabs.shape[0]):
        out += slabs[s].astype(np.float64)
    return out


def cd_sweep(W, HHt, XHt, margins=None, live=None, jitter=None):
    """One call of _update_cdnmf_fast(W, HHt, XHt, arange(k)): W (rows x k, fp64) is updated in place, the violation is returned.
    All rows at once, the coordinates and the terms of every gradient in the literal order (one product, one sum per term).
    margins (a list): receives, per coordinate, min |W - grad / hess| / max |W| over the clamp decisions of the rows marked in `live`
    (default: all), for the callers that assert that no decision hangs on a rounding.  A cell with W == 0 and grad == 0, both exact
    (a structural zero: no term of its gradient is non-zero), is no decision: it stays 0 whatever the rounding.
    jitter ((rng, size)): every entry of HHt and XHt is scaled by 1 + size * N(0, 1) first -- a stand-in for operands that carry a
    rounding of that relative size, for the callers that ask whether a recorded run survives it."""
    rows, k = W.shape
    if jitter is not None:
        rng, size = jitter
        HHt = HHt * (1.0 + size * rng.standard_normal(HHt.shape))
        HHt = (HHt + HHt.T) / 2
        XHt = XHt * (1.0 + size * rng.standard_normal(XHt.shape))
    violation = 0.0
    for t in range(k):
        grad = -XHt[:, t].astype(np.float64)
        for r in range(k):
            grad = grad + HHt[t, r] * W[:, r]
        pg = np.where(W[:, t] == 0, np.minimum(0.0, grad), grad)
        violation += float(np.abs(pg).sum())
        hess = HHt[t, t]
        if hess != 0:
            new = W[:, t] - grad / hess
            decided = ~((W[:, t] == 0) & (grad == 0))
            seen = new[decided if live is None else (decided & live)]
            if margins is not None and seen.size:
                margins.append(float(np.abs(seen).min() / max(np.abs(W).max(), 1e-300)))
            W[:, t] = np.maximum(new, 0.0)
    return violation


def block_maxima(W, rows_pad, kp):
    """max |(float32) W| per 128-row block and column of the padded factor: [rows_pad / 128][kp]."""
    F = np.zeros((rows_pad, kp), dtype=np.float32)
    F[: W.shape[0], : W.shape[1]] = W.astype(np.float32)
    return np.abs(F).reshape(rows_pad // 128, 128, kp).max(axis=1)


def fit_cd(X, W, H, tol=1e-4, max_iter=1000, margins=None, jitter=None):
    """_fit_coordinate_descent: returns (W, H, n_iter, [violation / violation_init per iteration])."""
    X = np.asarray(X, dtype=np.float64)
    W, Ht = np.array(W, dtype=np.float64, order="C"), np.array(H.T, dtype=np.float64, order="C")
    ratios, n_iter, violation_init = [], 0, None
    live_rows, live_cols = X.any(axis=1), X.any(axis=0)   # (a row of X without a one: its row of W is driven to exactly 0)
    for n_iter in range(1, max_iter + 1):
        violation = 0.0
        violation += cd_sweep(W, Ht.T @ Ht, X @ Ht, margins, live_rows, jitter)
        violation += cd_sweep(Ht, W.T @ W, X.T @ W, margins, live_cols, jitter)
        if n_iter == 1:
            violation_init = violation
        if violation_init == 0:
            ratios.append(0.0)
            break
        ratios.append(violation / violation_init)
        if violation / violation_init <= tol:
            break
    return W, Ht.T.copy(), n_iter, ratios


def reconstruction_err(X, W, H):
    """NMF.reconstruction_err_: ||X - W H||_F."""
    X = np.asarray(X, dtype=np.float64)
    return float(np.sqrt(max(((X - W @ H) ** 2).sum(), 0.0)))


# ---- the initialisers ----------------------------------------------------------------------------------------------------------

def random_init(X, k, rng):
    avg = np.sqrt(X.mean() / k)
    H = avg * rng.standard_normal(size=(k, X.shape[1]))
    W = avg * rng.standard_normal(size=(X.shape[0], k))
    return np.abs(W), np.abs(H)


def randomized_svd(X, k, rng, diag=None):
    """_randomized_svd(X, k, random_state=rng) with its defaults: 10 oversamples, n_iter 'auto', LU-normalised power iterations, a
    transposed problem when m < n, svd_flip."""
    m, n = X.shape
    n_iter = 7 if k < 0.1 * min(m, n) else 4
    transpose = m < n
    A = X.T if transpose else X
    Q = rng.normal(size=(A.shape[1], k + 10))
    for _ in range(n_iter):
        Q, _ = linalg.lu(A @ Q, permute_l=True, check_finite=False)
        Q, _ = linalg.lu(A.T @ Q, permute_l=True, check_finite=False)
    Q, _ = linalg.qr(A @ Q, mode="economic", check_finite=False)
    B = Q.T @ A
    Uhat, s, Vt = linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    U = Q @ Uhat
    if diag is not None:
        diag["singular"] = s[: k + 1].copy()
    if not transpose:
        signs = np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])
    else:
        signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    U, Vt = U * signs[np.newaxis, :], Vt * signs[:, np.newaxis]
    if transpose:
        return Vt[:k, :].T, s[:k], U[:, :k].T
    return U[:, :k], s[:k], Vt[:k, :]


def nndsvd_init(X, k, variant, rng, eps=1e-6, diag=None):
    """_initialize_nmf(X, k, init=variant, random_state=rng) for variant in 'nndsvd', 'nndsvda', 'nndsvdar'.  diag (a dict): receives the
    top k + 1 singular values, the (positive, negative) weight of every pair and the factors before the truncation at eps."""
    if k > min(X.shape):
        raise ValueError("k > min(m, n)")
    if variant not in ("nndsvd", "nndsvda", "nndsvdar"):
        raise ValueError(variant)
    U, S, Vt = randomized_svd(X, k, rng, diag)
    A, B = U, Vt.T                                          # the singular vectors as the columns of A (m x k) and B (n x k)
    Ap, An, Bp, Bn = np.clip(A, 0, None), np.clip(-A, 0, None), np.clip(B, 0, None), np.clip(-B, 0, None)
    length = lambda M: np.sqrt(np.array([np.dot(M[:, j], M[:, j]) for j in range(M.shape[1])]))  # noqa: E731
    ap, an, bp, bn = length(Ap), length(An), length(Bp), length(Bn)
    pos, neg = ap * bp, an * bn
    take_pos = pos > neg                                    # strict '>': equal weights keep the negative parts
    with np.errstate(divide="ignore", invalid="ignore"):    # (the part not taken may be all zero)
        a = np.where(take_pos, Ap / ap, An / an)
        b = np.where(take_pos, Bp / bp, Bn / bn)
    gain = np.sqrt(S * np.where(take_pos, pos, neg))
    W, H = gain * a, np.ascontiguousarray((gain * b).T)
    W[:, 0], H[0, :] = np.sqrt(S[0]) * np.abs(A[:, 0]), np.sqrt(S[0]) * np.abs(B[:, 0])   # the leading pair: one-signed, taken whole
    if diag is not None:
        diag["pairs"], diag["W_raw"], diag["H_raw"] = list(zip(pos[1:], neg[1:])), W.copy(), H.copy()
    fill = X.mean()
    for F in (W, H):                                        # W before H: the order of the 'ar' draws
        F[F < eps] = 0
        empty = F == 0
        if variant == "nndsvda":
            F[empty] = fill
        elif variant == "nndsvdar":
            F[empty] = np.abs(fill * rng.standard_normal(int(empty.sum())) / 100)
    return W, H


def initialize(X, k, method, seed, U=None, V=None, diag=None):
    """(W, H) as NMFSklearn(k, init_method=method, seed=seed) starts from; 'custom': U, V as given (H = V^T)."""
    X = np.asarray(X, dtype=np.float64)
    rng = np.random.RandomState(seed)
    if method == "custom":
        return np.array(U, dtype=np.float64), np.array(V, dtype=np.float64).T.copy()
    if method == "random":
        return random_init(X, k, rng)
    return nndsvd_init(X, k, method, rng, diag=diag)


# ---- a stand-in for pybmf_amd.nmf.NMFEngine ---------------------------------------------------------------------------------------

class NumpyEngine:
    """The interface of NMFEngine over a dense NumPy X: what the model's host loop drives when no GPU is there."""

    def __init__(self, X, k):
        self.Xd, self.k = np.asarray(X, dtype=np.float64), int(k)
        self.rows = {}
        self.products = 0

    def product(self, T, transposed=False):
        self.products += 1
        return (self.Xd.T if transposed else self.Xd) @ np.asarray(T, dtype=np.float64)

    def load_factors(self, U0, V0):
        self.W, self.Ht = np.array(U0, dtype=np.float64, order="C"), np.array(V0, dtype=np.float64, order="C")

    def iterate(self, it):
        vu = cd_sweep(self.W, self.Ht.T @ self.Ht, self.Xd @ self.Ht)
        vv = cd_sweep(self.Ht, self.W.T @ self.W, self.Xd.T @ self.W)
        self.rows[it] = (vu, vv)

    def row(self, it):
        return self.rows[it]

    def factors(self):
        return self.W.copy(), self.Ht.copy()

    def rec_error(self):
        return float((self.Xd ** 2).sum() - 2.0 * (self.W * (self.Xd @ self.Ht)).sum() + ((self.W.T @ self.W) * (self.Ht.T @ self.Ht)).sum())
