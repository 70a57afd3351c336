#!/usr/bin/env python3
"""Golden g33: BinaryMFThreshold of the *reference* at a rank 64 < k <= 128 (the reference has no rank limit).

    python tests/golden/make_golden_threshold_wide.py        (build container only: the reference is read from make_golden.REF)

Writes g33_threshold_wide.npz / .json.  Factors as in g4 / g20: a WNMF(k, W='full', init_method='normal') fit of a planted Boolean
matrix with a few per cent of flipped cells.  Cases:

  a  130 x 100, k = 72,  W='full', lamda = 10 and 100, from (u, v) = (0.5, 0.5)
  b  150 x 140, k = 128, W='full', lamda = 100
  c   90 x 70,  k = 65,  W='full', lamda = 10          (the second 64-column block holds one column)
  d  case a's matrix as a csr with ~40 % of its cells stored (ones and explicit zeros; row D_EMPTY_ROW and column D_EMPTY_COL hold no
     stored cell), the class default W='mask', from (0.3, 0.3), lamda = 10, max_iter = 40; case a's factors
  e  case a's matrix split by cell into train / val / test as in g20, task='prediction', W='mask', from (0.3, 0.3), lamda = 10,
     max_iter = 30; case a's factors

Per case: X as packed bits (a, b, c) or as cell lists (d, e), U and V (fp64, as the reference used them), F and dF of the reference on
the 4 x 4 grid GRID x GRID of (u, v), every row of logs['updates'], the final (u, v), and TP / FP / FN / TN of the training matrix
against the Boolean product at the final thresholds.

A case is only written when its recorded search does not hang on less than the gates the GPU kernels are held to (checked here on the
CPU, from the reference and the oracle alone; a case that fails moves on to the next seed):
  * oracle.threshold_fit reproduces the reference's number of rows and (u, v, F) of every row to 1e-9;
  * three reruns of the oracle fit with every F value multiplied by 1 + 1e-11 g and every dF component moved by 1e-9 (max|dF| + 1) g
    (g standard normal, drawn once per point: a point asked for twice answers the same, like the model's memo) keep the number of
    rows, (u, v, F) of every row within 1e-7 and the final counts;
  * no entry of U lies within 1e-6 of the final u, none of V within 1e-6 of the final v: the counts are decided.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import FIT_KW, df_rows, load_reference, quiet, staged_fit  # noqa: E402

import oracle as orc  # noqa: E402

GRID = [0.1, 0.3, 0.5, 0.7]
D_EMPTY_ROW, D_EMPTY_COL = 17, 23
JITTER_F, JITTER_DF = 1e-11, 1e-9      # the gates of the kernel tests (tests/test_thresh_wide_kernels_gpu.py)


def planted(m, n, kt, density, flip, rs):
    A = (rs.rand(m, kt) < density).astype(int)
    B = (rs.rand(n, kt) < density).astype(int)
    X = np.minimum(A @ B.T, 1)
    return np.where(rs.rand(m, n) < flip, 1 - X, X).astype(np.float64)


def wnmf_factors(PyBMF, X, k, seed):
    from PyBMF.models import WNMF
    with quiet():
        w = WNMF(k=k, W="full", init_method="normal", max_iter=40, seed=seed)
        w.fit(X.copy(), **FIT_KW)
    return np.array(w.U, dtype=np.float64), np.array(w.V, dtype=np.float64)


def reference_run(PyBMF, k, U, V, X_train, W, u, v, lam, max_iter, task="reconstruction", X_val=None, X_test=None):
    from PyBMF.models import BinaryMFThreshold
    with quiet():
        mdl = BinaryMFThreshold(k=k, U=U.copy(), V=V.copy(), W=W, u=u, v=v, lamda=lam, min_diff=1e-3, max_iter=max_iter)
        if X_val is None:
            staged_fit(mdl, X_train.copy())
        else:
            kw = dict(FIT_KW)
            kw["task"] = task
            mdl.check_params(**kw)
            mdl.load_dataset(X_train=X_train.copy(), X_val=X_val.copy(), X_test=X_test.copy())
            mdl.init_model()
        Fg = np.array([[mdl.F([a, b]) for b in GRID] for a in GRID])
        dFg = np.array([[mdl.dF([a, b]) for b in GRID] for a in GRID])
        mdl._fit()
    return df_rows(mdl.logs["updates"]), float(mdl.u), float(mdl.v), Fg, dFg


def oracle_fit(Xd, Wd, U, V, u, v, lam, max_iter, jitter_seed=None):
    """oracle.threshold_fit; with a seed, on an objective perturbed at the level of the kernel gates."""
    glob = orc.threshold_fit.__globals__
    F0, G0 = glob["thresh_F"], glob["thresh_dF"]
    if jitter_seed is not None:
        rs = np.random.RandomState(jitter_seed)
        memo_f, memo_g = {}, {}

        def F(X, W, U_, V_, a, b, lamda):
            key = (float(a), float(b))
            if key not in memo_f:
                memo_f[key] = F0(X, W, U_, V_, a, b, lamda) * (1.0 + JITTER_F * rs.randn())
            return memo_f[key]

        def G(X, W, U_, V_, a, b, lamda):
            key = (float(a), float(b))
            if key not in memo_g:
                g = G0(X, W, U_, V_, a, b, lamda)
                memo_g[key] = g + JITTER_DF * (np.abs(g).max() + 1.0) * rs.randn(2)
            return memo_g[key].copy()
        glob["thresh_F"], glob["thresh_dF"] = F, G
    try:
        return orc.threshold_fit(Xd, U, V, Wd, u=u, v=v, lamda=lam, min_diff=1e-3, max_iter=max_iter)
    finally:
        glob["thresh_F"], glob["thresh_dF"] = F0, G0


def decided(Xd, Wd, U, V, ref_rows, ref_u, ref_v, u, v, lam, max_iter):
    """The three conditions of the module docstring; returns the final counts or None."""
    want = np.array(ref_rows["rows"])[:, :4]
    res = oracle_fit(Xd, Wd, U, V, u, v, lam, max_iter)
    mine = np.array([r[:4] for r in res["rows"]])
    if mine.shape != want.shape or not np.allclose(mine, want, rtol=1e-9, atol=1e-12):
        return None
    counts = tuple(int(c) for c in res["rows"][-1][4:])
    for seed in (1, 2, 3):
        jit = oracle_fit(Xd, Wd, U, V, u, v, lam, max_iter, jitter_seed=seed)
        rows = np.array([r[:4] for r in jit["rows"]])
        if rows.shape != want.shape or not np.allclose(rows, want, rtol=1e-7, atol=1e-7):
            return None
        if tuple(int(c) for c in jit["rows"][-1][4:]) != counts:
            return None
    if np.abs(U - ref_u).min() <= 1e-6 or np.abs(V - ref_v).min() <= 1e-6:
        return None
    return counts


def cells_of(M):
    coo = M.tocoo()
    return coo.row.astype(np.int32), coo.col.astype(np.int32), coo.data.astype(np.uint8)


def dense_of(M):
    X, W = np.zeros(M.shape), np.zeros(M.shape)
    coo = M.tocoo()
    X[coo.row, coo.col], W[coo.row, coo.col] = coo.data, 1.0
    return X, W


def full_case(PyBMF, name, m, n, k, lams, seed0, out, meta):
    for seed in range(seed0, seed0 + 20):
        rs = np.random.RandomState(seed)
        X = planted(m, n, 9, 0.2, 0.03, rs)
        U, V = wnmf_factors(PyBMF, X, k, seed)
        runs = {}
        for lam in lams:
            rows, u, v, Fg, dFg = reference_run(PyBMF, k, U, V, X, "full", 0.5, 0.5, lam, 100)
            counts = decided(X, None, U, V, rows, u, v, 0.5, 0.5, lam, 100)
            if counts is None:
                break
            runs[lam] = (rows, u, v, Fg, dFg, counts)
        if len(runs) == len(lams):
            break
    else:
        raise SystemExit(f"case {name}: no seed passes the conditions")
    out.update({f"{name}_X_bits": np.packbits(X.astype(np.uint8), axis=1, bitorder="little"), f"{name}_shape": np.array(X.shape),
                f"{name}_U": U, f"{name}_V": V})
    meta[name] = {"k": k, "seed": seed, "W": "full", "u0": 0.5, "v0": 0.5, "max_iter": 100, "lamdas": list(lams)}
    for lam, (rows, u, v, Fg, dFg, counts) in runs.items():
        out[f"{name}_F_grid_lam{lam}"], out[f"{name}_dF_grid_lam{lam}"] = Fg, dFg
        meta[name][f"lam{lam}"] = {"rows": rows, "u": u, "v": v, "counts": list(counts)}
    return X, U, V


def main():
    from scipy.sparse import csr_matrix
    PyBMF = load_reference()
    out, meta = {}, {"grid": GRID}
    Xa, Ua, Va = full_case(PyBMF, "a", 130, 100, 72, (10, 100), 100, out, meta)
    full_case(PyBMF, "b", 150, 140, 128, (100,), 200, out, meta)
    full_case(PyBMF, "c", 90, 70, 65, (10,), 300, out, meta)
    m, n = Xa.shape
    # d: ~40 % of case a's cells stored, ones and explicit zeros, one row and one column without a stored cell
    for seed in range(400, 420):
        keep = np.random.RandomState(seed).rand(m, n) < 0.4
        keep[D_EMPTY_ROW, :] = False
        keep[:, D_EMPTY_COL] = False
        r, c = np.nonzero(keep)
        Xd = csr_matrix((Xa[r, c], (r, c)), shape=(m, n))
        assert Xd.nnz == r.size and (Xd.data == 0).any() and (Xd.data == 1).any()
        rows, u, v, Fg, dFg = reference_run(PyBMF, 72, Ua, Va, Xd, "mask", 0.3, 0.3, 10, 40)
        dense, mask = dense_of(Xd)
        counts = decided(dense, mask, Ua, Va, rows, u, v, 0.3, 0.3, 10, 40)
        if counts is not None:
            break
    else:
        raise SystemExit("case d: no seed passes the conditions")
    rr, cc, vv = cells_of(Xd)
    out.update(d_rows=rr, d_cols=cc, d_vals=vv, d_F_grid=Fg, d_dF_grid=dFg)
    meta["d"] = {"k": 72, "seed": seed, "W": "mask", "u0": 0.3, "v0": 0.3, "lamda": 10, "max_iter": 40, "rows": rows, "u": u, "v": v,
                 "counts": list(counts), "empty_row": D_EMPTY_ROW, "empty_col": D_EMPTY_COL}
    # e: train / val / test by cell, task='prediction'
    for seed in range(500, 520):
        part = np.random.RandomState(seed).rand(m, n)
        sets = {}
        for name, lo, hi in (("train", 0.0, 0.35), ("val", 0.35, 0.43), ("test", 0.43, 0.52)):
            r, c = np.nonzero((part >= lo) & (part < hi))
            sets[name] = csr_matrix((Xa[r, c], (r, c)), shape=(m, n))
            assert sets[name].nnz == r.size
        rows, u, v, Fg, dFg = reference_run(PyBMF, 72, Ua, Va, sets["train"], "mask", 0.3, 0.3, 10, 30, task="prediction",
                                            X_val=sets["val"], X_test=sets["test"])
        dense, mask = dense_of(sets["train"])
        counts = decided(dense, mask, Ua, Va, rows, u, v, 0.3, 0.3, 10, 30)
        if counts is not None:
            break
    else:
        raise SystemExit("case e: no seed passes the conditions")
    for name in sets:
        rr, cc, vv = cells_of(sets[name])
        out.update({f"e_{name}_rows": rr, f"e_{name}_cols": cc, f"e_{name}_vals": vv})
    out.update(e_F_grid=Fg, e_dF_grid=dFg)
    meta["e"] = {"k": 72, "seed": seed, "W": "mask", "task": "prediction", "u0": 0.3, "v0": 0.3, "lamda": 10, "max_iter": 30, "rows": rows,
                 "u": u, "v": v, "counts": list(counts)}
    np.savez_compressed(os.path.join(HERE, "g33_threshold_wide.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "g33_threshold_wide.json"), "w"), indent=1)
    print({k_: (meta[k_].get("seed"), [len(meta[k_][q]["rows"]["rows"]) for q in meta[k_] if q.startswith("lam") and q != "lamda" and q != "lamdas"]
                or len(meta[k_]["rows"]["rows"])) for k_ in "abcde"})


if __name__ == "__main__":
    main()
