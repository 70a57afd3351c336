#!/usr/bin/env python3
"""Generate g32_nmf.{npz,json} by running the *reference* NMFSklearn (PyBMF @ 2024_10_08), which hands the fit to scikit-learn.

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses) and scikit-learn is installed; nothing
of either is written here, only inputs and recorded outputs.  This script is the one place in the repository that imports
scikit-learn: the tests read the fixture and tests/nmf_ref.py.

    python tests/golden/make_golden_nmf.py          (a few minutes: most seeds fail one of the margins below)

Cases (tol = 1e-4, max_iter = 1000 unless noted):
  a  70 x 45, k = 5, planted with 3 % flips, init 'nndsvd'
  b  the same X, 'random'
  c  the same X, 'nndsvda'
  d  the same X, 'nndsvdar'
  e  the same X, 'custom' (U, V drawn uniformly in (0, 1))
  f  45 x 70, 'nndsvd': the SVD runs on the transposed matrix
  g  600 x 400, k = 33, 'nndsvd': 33 disjoint blocks of graded sizes under 0.1 % flips (the top 34 singular values must be 5 % apart:
     the blocks' are sqrt(area), 5.5 % apart by construction, and the flips stay below the smallest; 300 x 200 has no room for 33
     such blocks above the noise); 31 padded columns of a 64-column factor
  h  200 x 150, k = 64: 64 disjoint 3 x 2 blocks under 1 % flips, 'custom' from the planted factors scaled by 0.7 plus 0.2 uniform noise.
     (A planted matrix of lower rank under 'random' is no fixture at k = 64: the factors are barely determined, a jitter of 1e-6 moves
     them by 1e-3 within 28 iterations, and the fit takes 1000 iterations of 50 ms each in tests/nmf_ref.py.)
  i  a matrix of case a's kind, 'nndsvd', max_iter = 3: not converged
  j  30 x 20 of zeros, k = 3, 'random': the factors start at zero, violation_init == 0, n_iter_ == 1
  k  60 x 40, k = 4, planted, with an all-zero row and an all-zero column, 'random'
  l  120 x 80, k = 5, 'nndsvd': k < 0.1 min(m, n), seven power iterations, at k + 10 = 15 columns.  Case g runs seven as well
     (33 < 0.1 * 400) at 43 columns; the four-iteration branch is covered by cases a-f and i, all at k = 5
Stored per case: X, the initial W, H (scikit-learn's _initialize_nmf with the model's seed; 'custom': the matrices given), the final
U, V, n_iter_, reconstruction_err_, X_pd as packed bits, and the violation ratio of every iteration from tests/nmf_ref.py.

Asserted here (a failing case moves on to the next seed of its matrix and of its model), so that no recorded decision hangs on a
rounding:
  * tests/nmf_ref.py gives scikit-learn's initial W, H, n_iter_ and final factors to 1e-12 of the largest entry;
  * the ratio at the stopping iteration is <= 0.95 tol and the one before is >= 1.05 tol (case i: every ratio >= 1.05 tol);
  * every clamp decision W - grad / hess is at least 1e-5 max|W| away from 0 -- except in the rows of U (V) whose row (column) of X is
    all zero (case k): such a row is driven to exactly 0 coordinate by coordinate, and its last coordinate comes out as w - (h w) / h,
    an exact 0 or one rounding of it, far below every tolerance the fixture is compared under; and except where W and every term of
    the gradient are exact zeros, which is no decision at all.  Cases g and h record their smallest margin and do not assert it: it
    is 0.0 by construction.  Their matrices are disjoint blocks, so once the factors have taken the blocks' supports HHt is diagonal
    there and XHt is 0 outside a block; a cell outside its block that still holds w > 0 then comes out as w - (h w) / h, the same
    exact 0 or one rounding of it as in the zero-row case (seen in the first V sweep of g and the second of h).  Next to those, a few
    of their several hundred thousand ordinary decisions land within 1e-5 as well (3e-6 in both cases);
  * every case: three reruns of tests/nmf_ref.py whose Gram and numerator entries are scaled by 1 + 1e-6 N(0, 1) in every sweep (ten
    times the rounding of a 24-bit operand) stop at the same iteration with factors within 1e-4 of the largest entry, the gate of
    the GPU tests (measured on case a: the factors move by 15 times the jitter), and threshold at 0.5 to the same bits -- what the
    margins above are for, asked directly;
  * no final entry of U or V is within 1e-3 of 0.5;
  * the 'nndsvd*' cases: neighbours among the top k + 1 singular values differ by >= 5 % (relative to the larger), |m_p - m_n| is >= 1 % of
    the larger for every pair, and no entry before the truncation lies in [0.5e-6, 2e-6].  Case g is exempt from the last: among the
    33 000 entries of its singular vectors, which the flips smear over every magnitude, some lie in that band under every seed (their
    number is recorded as `at_eps`); under plain 'nndsvd' such an entry, kept or zeroed, moves the start by at most 2e-6 and nothing
    else hangs on it (no fill, no further draw).
"""
import json
import os
import sys
import warnings

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import FIT_KW, load_reference, quiet  # noqa: E402
from make_golden_grecond import planted  # noqa: E402
import nmf_ref  # noqa: E402


def graded_blocks(m, n, k, first, flips, seed):
    """k disjoint all-ones blocks, the smallest of area `first`, the areas growing by at least 12 % from one to the next (singular
    values sqrt(area), each at most 0.945 of the one before), then `flips` of the cells flipped."""
    shapes, area = [], first - 1
    while len(shapes) < k:
        area = max(area + 1, int(np.ceil(area * 1.12)))
        while True:   # the most compact a x b = area with b <= a <= 3 b, else the next area
            fits = [(a, area // a) for a in range(1, area + 1) if area % a == 0 and area // a <= a <= 3 * (area // a)]
            if fits:
                break
            area += 1
        shapes.append(min(fits, key=lambda s: (s[0] + s[1], -s[0])))
    X = np.zeros((m, n), dtype=bool)
    r = c = 0
    for a, b in reversed(shapes):
        assert r + a <= m and c + b <= n, (r + a, c + b)
        X[r:r + a, c:c + b] = True
        r, c = r + a, c + b
    X ^= np.random.RandomState(seed).rand(m, n) < flips
    return X.astype(np.uint8)


def blocks64(seed):
    """200 x 150 with 64 disjoint 3 x 2 blocks of ones and 1 % of the cells flipped; (X, the planted U, the planted V)."""
    U, V = np.zeros((200, 64)), np.zeros((150, 64))
    for j in range(64):
        U[3 * j:3 * j + 3, j] = 1
        V[2 * j:2 * j + 2, j] = 1
    X = (U @ V.T > 0) ^ (np.random.RandomState(seed).rand(200, 150) < 0.01)
    return X.astype(np.uint8), U, V


def zero_lines(X):
    X = X.copy()
    X[7, :] = 0
    X[:, 11] = 0
    return X


class Retry(Exception):
    pass


def need(ok, what):
    if not ok:
        raise Retry(what)


def run_case(name, make_X, k, init, seed, tol=1e-4, max_iter=1000):
    from PyBMF.models import NMFSklearn
    from sklearn.decomposition._nmf import _initialize_nmf
    X = make_X(seed)
    Xs = csr_matrix(X.astype(np.float64))
    U0 = V0 = None
    if init == "custom":
        rng = np.random.RandomState(seed + 1000)
        U0, V0 = rng.rand(X.shape[0], k), rng.rand(X.shape[1], k)
        if name == "h":   # a start near the planted factors
            _, Ut, Vt = blocks64(3400 + seed)
            U0, V0 = 0.7 * Ut + 0.2 * U0, 0.7 * Vt + 0.2 * V0
    with quiet(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = NMFSklearn(k=k, U=None if U0 is None else U0.copy(), V=None if V0 is None else V0.copy(), init_method=init, tol=tol,
                           max_iter=max_iter, seed=seed)
        model.fit(Xs, **FIT_KW)
        if init == "custom":
            W0, H0 = U0.copy(), V0.T.copy()
        else:
            W0, H0 = _initialize_nmf(Xs, k, init=init, random_state=np.random.RandomState(seed))
    U, V = np.asarray(model.U.todense()), np.asarray(model.V.todense())
    n_iter, err = int(model.model.n_iter_), float(model.model.reconstruction_err_)
    assert np.array_equal(model.model.components_.T, V)
    X_pd = np.asarray(csr_matrix(model.X_pd).todense()).astype(np.uint8)
    assert np.array_equal(X_pd, ((U > 0.5).astype(int) @ (V > 0.5).astype(int).T > 0).astype(np.uint8))

    # tests/nmf_ref.py against scikit-learn
    diag = {}
    Wr, Hr = nmf_ref.initialize(X, k, init, seed, U0, V0, diag=diag)
    scale = lambda A: max(np.abs(A).max(), 1e-300)  # noqa: E731
    assert np.abs(Wr - W0).max() <= 1e-12 * scale(W0) and np.abs(Hr - H0).max() <= 1e-12 * scale(H0), (name, "init")
    margins = []
    Uf, Hf, it_ref, ratios = nmf_ref.fit_cd(X, Wr, Hr, tol, max_iter, margins)
    assert it_ref == n_iter, (name, it_ref, n_iter)
    assert np.abs(Uf - U).max() <= 1e-12 * scale(U) and np.abs(Hf.T - V).max() <= 1e-12 * scale(V), (name, "fit")
    assert abs(nmf_ref.reconstruction_err(X, Uf, Hf) - err) <= 1e-9 * max(err, 1.0)

    # no recorded decision hangs on a rounding
    if n_iter < max_iter:
        if ratios[-1] != 0.0 or n_iter > 1:
            need(ratios[-1] <= 0.95 * tol and (n_iter == 1 or ratios[-2] >= 1.05 * tol), "stopping ratio")
    else:
        need(min(ratios) >= 1.05 * tol, "a ratio near tol in a run that must not converge")
    if name not in "gh":
        need(not margins or min(margins) >= 1e-5, "clamp margin %g" % (min(margins) if margins else 0))
    need(np.abs(U - 0.5).min() >= 1e-3 and np.abs(V - 0.5).min() >= 1e-3, "an entry near 0.5")
    if init.startswith("nndsvd"):
        s = diag["singular"]
        need(((s[:-1] - s[1:]) >= 0.05 * s[:-1]).all(), "singular gap")
        need(all(abs(p - q) >= 0.01 * max(p, q) for p, q in diag["pairs"]), "m_p against m_n")
        raw = np.concatenate([diag["W_raw"].ravel(), diag["H_raw"].ravel()])
        at_eps = int(((raw >= 0.5e-6) & (raw <= 2e-6)).sum())
        need(name == "g" or at_eps == 0, "an entry at the truncation threshold")
    for trial in range(3):
        Uj, Hj, it_j, _ = nmf_ref.fit_cd(X, Wr, Hr, tol, max_iter, jitter=(np.random.RandomState(100 * seed + trial), 1e-6))
        need(it_j == n_iter and np.abs(Uj - U).max() <= 1e-4 * scale(U) and np.abs(Hj.T - V).max() <= 1e-4 * scale(V), "a jittered rerun differs")
        need(np.array_equal(Uj > 0.5, U > 0.5) and np.array_equal(Hj.T > 0.5, V > 0.5), "a jittered rerun thresholds differently")
    arrays = dict(X=X, W0=W0, H0=H0, U=U, V=V, X_pd=np.packbits(X_pd, axis=1, bitorder="little"), ratios=np.array(ratios))
    meta = dict(shape=list(X.shape), k=k, init=init, seed=seed, tol=tol, max_iter=max_iter, n_iter=n_iter, reconstruction_err=err,
                min_clamp_margin=(min(margins) if margins else None))
    if init.startswith("nndsvd"):
        meta["at_eps"] = at_eps
    return arrays, meta


def main():
    load_reference()
    Xa = lambda s: planted(70, 45, 5, 0.3, 0.03, 3200 + s)  # noqa: E731
    plans = [
        ("a", Xa, 5, "nndsvd", {}), ("b", Xa, 5, "random", {}), ("c", Xa, 5, "nndsvda", {}), ("d", Xa, 5, "nndsvdar", {}),
        ("e", Xa, 5, "custom", {}), ("f", lambda s: planted(45, 70, 5, 0.3, 0.03, 3300 + s), 5, "nndsvd", {}),
        ("g", lambda s: graded_blocks(600, 400, 33, 12, 0.001, 3600 + s), 33, "nndsvd", {}),
        ("h", lambda s: blocks64(3400 + s)[0], 64, "custom", {}),
        ("i", Xa, 5, "nndsvd", dict(max_iter=3)),
        ("j", lambda s: np.zeros((30, 20), dtype=np.uint8), 3, "random", {}),
        ("k", lambda s: zero_lines(planted(60, 40, 4, 0.3, 0.03, 3500 + s)), 4, "random", {}),
        ("l", lambda s: planted(120, 80, 5, 0.3, 0.03, 3700 + s), 5, "nndsvd", {}),
    ]
    arrays, meta = {}, {"cases": {}}
    for name, make_X, k, init, kw in plans:
        for seed in range(2024, 2024 + 4000):
            try:
                arr, m = run_case(name, make_X, k, init, seed, **kw)
                break
            except Retry as why:
                print(f"  case {name}, seed {seed}: {why}; next seed", flush=True)
        else:
            raise SystemExit(f"case {name}: no seed passes the margins")
        for key, A in arr.items():
            arrays[f"{name}_{key}"] = A
        meta["cases"][name] = m
        print(name, m)
    np.savez_compressed(os.path.join(HERE, "g32_nmf.npz"), **arrays)
    with open(os.path.join(HERE, "g32_nmf.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
