#!/usr/bin/env python3
"""Generate g22_faststep.{npz,json} by running the *reference* FastStep (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_faststep.py

Cases (96 x 72, k = 4, planted factors with 3 % flips, max_round = 2, max_iter = 5):
  a  tau = 20, W = 'full'
  b  tau = 2,  W = 'full'
  c  tau = 2,  W = 'mask' on a csr that stores the ones and an equal number of sampled explicit zeros
For each: X (and the stored pattern), the factors after to_interval, every row of logs['updates'], the integer TP / FP / FN / TN of
the final X_pd, the final U, V, and at three (k, point) pairs along the run the inputs (U, V, u, v) with the reference's F and dF.
"""
import json
import os
import sys

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, df_rows, load_reference, quiet  # noqa: E402

M, N, K = 96, 72, 4


def planted(seed):
    rng = np.random.RandomState(seed)
    U = rng.rand(M, K) < 0.2
    V = rng.rand(N, K) < 0.2
    X = (U.astype(int) @ V.astype(int).T > 0)
    flip = rng.rand(M, N) < 0.03
    return (X ^ flip).astype(np.int64)


def with_sampled_zeros(X, seed):
    """csr that stores the ones of X and an equal number of explicit zeros."""
    rng = np.random.RandomState(seed)
    r1, c1 = np.nonzero(X)
    r0, c0 = np.nonzero(X == 0)
    pick = rng.choice(len(r0), size=len(r1), replace=False)
    rows = np.concatenate([r1, r0[pick]])
    cols = np.concatenate([c1, c0[pick]])
    data = np.concatenate([np.ones(len(r1)), np.zeros(len(r1))])
    return csr_matrix((data, (rows, cols)), shape=X.shape)


def run_case(PyBMF, X_in, tau, W, seed):
    from PyBMF.models import FastStep
    from PyBMF.utils import to_interval
    with quiet():
        model = FastStep(k=K, W=W, tau=tau, max_round=2, max_iter=5, seed=seed)
        # fit() split where the starting factors exist (models/FastStep.py:30-40)
        model.check_params(**FIT_KW)
        model.load_dataset(X_train=X_in, X_val=None, X_test=None)
        model.init_model()
        model.U = to_interval(model.U, 1e-5, 0.01)
        model.V = to_interval(model.V, 1e-5, 0.01)
        U0, V0 = model.U.copy(), model.V.copy()
        pattern = np.asarray(model.W).copy()

        calls = []
        dF_ref = model.dF

        def dF_logged(params, k):
            calls.append((model.U.copy(), model.V.copy(), np.array(params, dtype=np.float64), int(k)))
            return dF_ref(params, k=k)
        model.dF = dF_logged
        model._fit()
        model.dF = dF_ref
        X_pd = (model.U @ model.V.T > tau).astype(int)
        points = []
        for idx in (0, len(calls) // 2, len(calls) - 1):
            U, V, params, k = calls[idx]
            keep = model.U, model.V
            model.U, model.V = U.copy(), V.copy()
            points.append(dict(U=U, V=V, params=params, k=k, F=float(model.F(params, k=k)), dF=np.asarray(model.dF(params, k=k), dtype=np.float64)))
            model.U, model.V = keep
    X_dense = np.asarray(X_in.todense()) if hasattr(X_in, "todense") else np.asarray(X_in)
    return dict(X=X_dense.astype(np.uint8), pattern=pattern.astype(np.uint8), U0=U0, V0=V0, U=model.U.copy(), V=model.V.copy(),
                log=df_rows(model.logs["updates"]), counts=counts_of(PyBMF, csr_matrix(X_dense), csr_matrix(X_pd)), points=points)


def main():
    PyBMF = load_reference()
    X = planted(2201)
    cases = {"a": run_case(PyBMF, csr_matrix(X), 20, "full", 5),
             "b": run_case(PyBMF, csr_matrix(X), 2, "full", 5),
             "c": run_case(PyBMF, with_sampled_zeros(X, 2202), 2, "mask", 5)}
    arrays, meta = {}, {"shape": [M, N], "k": K, "max_round": 2, "max_iter": 5, "cases": {}}
    for name, c in cases.items():
        for key in ("X", "pattern", "U0", "V0", "U", "V"):
            arrays[f"{name}_{key}"] = c[key]
        for i, p in enumerate(c["points"]):
            for key in ("U", "V", "params", "dF"):
                arrays[f"{name}_p{i}_{key}"] = p[key]
        meta["cases"][name] = {"tau": {"a": 20, "b": 2, "c": 2}[name], "W": "mask" if name == "c" else "full", "log": c["log"],
                               "counts": c["counts"], "points": [{"k": p["k"], "F": p["F"]} for p in c["points"]]}
        print(name, "rows:", len(c["log"]["rows"]), "counts:", c["counts"], "stored cells:", int(c["pattern"].sum()),
              "F at points:", [p["F"] for p in c["points"]])
    np.savez_compressed(os.path.join(HERE, "g22_faststep.npz"), **arrays)
    with open(os.path.join(HERE, "g22_faststep.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
