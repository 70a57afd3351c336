#!/usr/bin/env python3
"""Generate g23_grecond.{npz,json} by running the *reference* GreConD (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_grecond.py          (about a minute and a half, nearly all of it case b)

Cases (planted Boolean factors, fixed RandomState seeds):
  a  96 x 72, 4 planted factors, 3 % flips, k = 6                      stops on "Reach requested factor"
  b  200 x 150, 6 planted factors, 3 % flips, k = None, tol = 0.02    stops on error <= tol: the factor added last is truncated
  c  40 x 30, noise-free product of 4 factors, k = None, tol = 0      runs until the error is 0 (same truncation)
  d  the ones of case a's X dealt to train / val / test (70 / 15 / 15 %), k = 6, task = 'reconstruction'
  e  20 x 15 of zeros, k = None                                         get_concept returns score 0 at once.  The reference then
     fails inside its own "No pattern found" stop (early_stop calls _early_stop without the `verbose` argument it requires:
     TypeError), so there is no final state to record: the fixture keeps X, the one get_concept result and the exception's name
For each: the matrices (uint8), every row of logs['updates'] with the `shape` list flattened to two integers
(k, score, |u|, |v|, then the four metrics per data set), the final U, V, the integer TP / FP / FN / TN of the final X_pd against
X_train; for the first, a middle and the last get_concept call of cases a and b the residual that went in and (score, u, v) that
came out.
"""
import json
import os
import sys

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402


def planted(m, n, k, density, flips, seed):
    rng = np.random.RandomState(seed)
    U = rng.rand(m, k) < density
    V = rng.rand(n, k) < density
    X = (U.astype(int) @ V.astype(int).T > 0)
    if flips:
        X = X ^ (rng.rand(m, n) < flips)
    return X.astype(np.uint8)


def deal(X, seed):
    """The ones of X dealt to three matrices: 70 % train, 15 % val, 15 % test."""
    rng = np.random.RandomState(seed)
    lot = rng.rand(*X.shape)
    ones = X != 0
    return ((ones & (lot < 0.7)).astype(np.uint8), (ones & (lot >= 0.7) & (lot < 0.85)).astype(np.uint8),
            (ones & (lot >= 0.85)).astype(np.uint8))


def dense_u8(A):
    return np.asarray(A.todense()).astype(np.uint8)


def flat_log(df):
    """Rows of the log without the time stamp; the `shape` cell [|u|, |v|] becomes two columns."""
    cols = [str(c[-1]) if c[0] == "" else "{}/{}".format(c[0], c[-1]) for c in df.columns]   # ('', '', 'k'), ('train', 0, 'Recall')
    names, rows = [], []
    for _, r in df.iterrows():
        names, row = [], []
        for name, v in zip(cols, r.tolist()):
            if name == "time":
                continue
            if name == "shape":
                names += ["n_u", "n_v"]
                row += [int(v[0]), int(v[1])]
            elif name in ("k", "score"):
                names.append(name)
                row.append(int(v))
            else:
                names.append(name)
                row.append(float(v))
        rows.append(row)
    return {"columns": names, "rows": rows}


def run_case(PyBMF, X, k, tol, X_val=None, X_test=None, want_points=False, may_raise=()):
    from PyBMF.models import GreConD
    mod = sys.modules["PyBMF.models.GreConD"]   # the module, not the class of the same name
    calls = []
    get_concept = mod.get_concept

    def logged(X_gt, X_rs):
        rs = dense_u8(X_rs) if want_points else None
        score, u, v = get_concept(X_gt, X_rs)
        calls.append((rs, int(score), dense_u8(u).ravel(), dense_u8(v).ravel()))
        return score, u, v
    mod.get_concept = logged
    raised = None
    try:
        with quiet():
            model = GreConD(k=k, tol=tol)
            try:
                model.fit(csr_matrix(X.astype(np.float64)), None if X_val is None else csr_matrix(X_val.astype(np.float64)),
                          None if X_test is None else csr_matrix(X_test.astype(np.float64)), **FIT_KW)
            except may_raise as exc:
                raised = type(exc).__name__
    finally:
        mod.get_concept = get_concept
    if raised is not None:
        return dict(X=X, n_calls=len(calls), raised=raised, log={"columns": [], "rows": []}, counts=None,
                    points=[dict(index=i, X_rs=dense_u8(csr_matrix(X)), score=c[1], u=c[2], v=c[3]) for i, c in enumerate(calls)])
    out = dict(X=X, U=dense_u8(model.U), V=dense_u8(model.V), n_calls=len(calls), raised=None,
               log=flat_log(model.logs["updates"]) if "updates" in model.logs else {"columns": [], "rows": []})
    X_pd = getattr(model, "X_pd", None)
    X_pd = csr_matrix(X.shape) if X_pd is None else csr_matrix(X_pd)
    out["counts"] = counts_of(PyBMF, csr_matrix(X.astype(np.float64)), X_pd)
    out["points"] = [dict(index=i, X_rs=calls[i][0], score=calls[i][1], u=calls[i][2], v=calls[i][3])
                     for i in ((0, len(calls) // 2, len(calls) - 1) if want_points else ())]
    return out


def main():
    PyBMF = load_reference()
    Xa = planted(96, 72, 4, 0.2, 0.03, 2301)
    Xb = planted(200, 150, 6, 0.2, 0.03, 2302)
    Xc = planted(40, 30, 4, 0.25, 0.0, 2303)
    tr, va, te = deal(Xa, 2304)
    params = {"a": dict(k=6, tol=0), "b": dict(k=None, tol=0.02), "c": dict(k=None, tol=0), "d": dict(k=6, tol=0), "e": dict(k=None, tol=0)}
    cases = {"a": run_case(PyBMF, Xa, want_points=True, **params["a"]),
             "b": run_case(PyBMF, Xb, want_points=True, **params["b"]),
             "c": run_case(PyBMF, Xc, **params["c"]),
             "d": run_case(PyBMF, tr, X_val=va, X_test=te, **params["d"]),
             "e": run_case(PyBMF, np.zeros((20, 15), dtype=np.uint8), may_raise=(TypeError,), **params["e"])}
    cases["d"]["X_val"], cases["d"]["X_test"] = va, te
    arrays, meta = {}, {"cases": {}}
    for name, c in cases.items():
        for key in ("X", "U", "V", "X_val", "X_test"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        for i, p in enumerate(c["points"]):
            for key in ("X_rs", "u", "v"):
                arrays[f"{name}_p{i}_{key}"] = p[key]
        meta["cases"][name] = dict(params[name], shape=list(c["X"].shape), log=c["log"], counts=c["counts"], n_calls=c["n_calls"],
                                   raised=c["raised"], points=[{"index": p["index"], "score": p["score"]} for p in c["points"]])
        print(name, "rows:", len(c["log"]["rows"]), "factors kept:", c["U"].shape[1] if "U" in c else None, "get_concept calls:",
              c["n_calls"], "counts:", c["counts"], "ones:", int(c["X"].sum()), "raised:", c["raised"])
    np.savez_compressed(os.path.join(HERE, "g23_grecond.npz"), **arrays)
    with open(os.path.join(HERE, "g23_grecond.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
