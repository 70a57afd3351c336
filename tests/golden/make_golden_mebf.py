#!/usr/bin/env python3
"""Generate g27_mebf.{npz,json} by running the *reference* MEBF (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_mebf.py          (about ten seconds)

(i) Full fits under the defined tie rule.  The reference orders scores with np.flip(np.argsort(scores)) and NumPy's default sort is
not stable: which member of a tie group lands on the median position depends on the sort kernel of the host.  This build defines the
order as (score descending, index descending) = np.flip(np.argsort(scores, kind='stable')), so for these fits the `np` that the
reference's MEBF module sees is a proxy (StableNumpy below) whose argsort is stable and which is NumPy in everything else.
  a  96 x 72, 4 planted factors, 3 % flips, k = 6, t = 0.8             stops on "Reach requested factor"
  b  40 x 30, noise-free product of 4 factors, k = None, tol = 0, t = 0.9   runs to residual 0; error <= tol truncates the last factor
  c  case a's X, k = None, t = 0.3                                      reaches weak_signal_detection and goes on
  d  case a's X, k = None, t = 0.2, w_fp = 2, w_fn = 1                  weak signal, then "Cost stops decreasing": the reference's own
     early_stop raises TypeError there (it calls _early_stop without `verbose`); the name, the log rows and the factors so far are kept
  e  20 x 15 of zeros, t = 0.8                                          "No pattern found" at once, the same TypeError
  f  33 x 65, 3 planted factors (density 0.3, 3 % flips, seed 9), k = 3, t = 0.5, w_fp = w_fn = 0.5
  g  case a's X, k = 8, t = 0.8, tol = 0.15                           error <= tol fires on the first factor (error 0.1395), which is
     truncated; the next round still sees the residual and X_pd WITH that factor (the reference refreshes them only after the next
     set_factors) but scores its candidates on the truncated U, V: no candidate lowers the cost and "Cost stops decreasing" raises
     the TypeError of case d.  A larger tol gives the same run
  g2 the same with tol = 0.13                                           the truncation fires three times (factor indices 1, 2, 3) and the
     fit goes on in between, leaving an empty column in U, V; it ends like g
  h  case a's ones dealt to train / val / test (70 / 15 / 15 %), k = 6, t = 0.8
For each: the matrices (uint8), every row of logs['updates'] (cost, |u|, |v|, rs, then the four metrics per data set), the final U
and V, the integer TP / FP / FN / TN of the final X_pd against X_train, the exception's name where the run raises.

(ii) The reference as shipped (the default argsort), cases a and c: for the first, a middle and the last get_factor call the residual
that went in, the axis, the `mid` the reference picked (from the order its own argsort call returned) and the (a, b) it returned.
"""
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402
from make_golden_grecond import deal, dense_u8, planted  # noqa: E402


class StableNumpy:
    """NumPy with a stable argsort; records what every argsort call returned."""

    def __init__(self, stable):
        self.stable, self.orders = stable, []

    def __getattr__(self, name):
        return getattr(np, name)

    def argsort(self, a, *args, **kwargs):
        if self.stable:
            kwargs["kind"] = "stable"
        order = np.argsort(a, *args, **kwargs)
        self.orders.append(np.array(order))
        return order


def flat_log(df):
    cols = [str(c[-1]) if c[0] == "" else "{}/{}".format(c[0], c[-1]) for c in df.columns]
    names, rows = [], []
    for _, r in df.iterrows():
        names, row = [], []
        for name, v in zip(cols, r.tolist()):
            if name == "time":
                continue
            if name == "shape":
                names += ["n_u", "n_v"]
                row += [int(v[0]), int(v[1])]
            elif name == "rs":
                names.append(name)
                row.append(int(v))
            else:
                names.append(name)
                row.append(float(v))
        rows.append(row)
    return {"columns": names, "rows": rows}


def vec(x, length):
    """A factor vector of get_factor as a flat uint8 array (the reference returns csr_matrix([]) when there is no positive score)."""
    x = np.asarray(csr_matrix(x).todense()).ravel()
    return (x != 0).astype(np.uint8) if x.size == length else np.zeros(length, dtype=np.uint8)


def run_case(PyBMF, X, params, X_val=None, X_test=None, stable=True, want_points=False, may_raise=()):
    from PyBMF.models import MEBF
    mod = sys.modules["PyBMF.models.MEBF"]   # the module, not the class of the same name
    proxy, calls, cuts = StableNumpy(stable), [], []
    get_factor = MEBF.get_factor

    def logged(self, axis):
        rs = dense_u8(csr_matrix(self.X_rs)) if want_points else None
        seen = len(proxy.orders)
        u, v = get_factor(self, axis)
        a, b = (u, v) if axis == 0 else (v, u)
        calls.append(dict(X_rs=rs, axis=int(axis), order=proxy.orders[seen], a=vec(a, X.shape[axis]), b=vec(b, X.shape[1 - axis])))
        return u, v

    def sp(A):
        return None if A is None else csr_matrix(A.astype(np.float64))
    saved_np, mod.np, MEBF.get_factor = mod.np, proxy, logged
    raised, t0 = None, time.time()
    try:
        with quiet():
            model = MEBF(**params)
            truncate = model.truncate_factors
            model.truncate_factors = lambda k: (cuts.append(int(k)), truncate(k))[1]
            try:
                model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
            except may_raise as exc:
                raised = type(exc).__name__
    finally:
        mod.np, MEBF.get_factor = saved_np, get_factor
    seconds = time.time() - t0
    log = flat_log(model.logs["updates"]) if "updates" in getattr(model, "logs", {}) else {"columns": [], "rows": []}
    f = len(log["rows"]) if raised else model.U.shape[1]
    out = dict(X=X, U=dense_u8(csr_matrix(model.U))[:, :f], V=dense_u8(csr_matrix(model.V))[:, :f], raised=raised, log=log,
               n_calls=len(calls), truncations=cuts, seconds=seconds)
    X_pd = csr_matrix(model.X_pd) if getattr(model, "X_pd", None) is not None else csr_matrix(X.shape)
    out["counts"] = counts_of(PyBMF, sp(X), X_pd)
    out["points"] = []
    for i in ((0, len(calls) // 2, len(calls) - 1) if want_points else ()):
        c = calls[i]
        scores = c["X_rs"].astype(np.int64).sum(axis=c["axis"])
        idx = [int(j) for j in np.flip(c["order"]) if scores[j] > 0]
        mid = idx[len(idx) // 2] if idx else -1
        if mid >= 0:
            assert (c["a"] == (c["X_rs"][:, mid] if c["axis"] == 0 else c["X_rs"][mid])).all()
        out["points"].append(dict(index=i, axis=c["axis"], mid=mid, X_rs=c["X_rs"], a=c["a"], b=c["b"]))
    return out


def main():
    PyBMF = load_reference()
    Xa = planted(96, 72, 4, 0.2, 0.03, 2301)
    Xb = planted(40, 30, 4, 0.25, 0.0, 2303)
    Xf = planted(33, 65, 3, 0.3, 0.03, 9)
    tr, va, te = deal(Xa, 2304)
    params = {"a": dict(k=6, tol=0, t=0.8, w_fp=1, w_fn=1), "b": dict(k=None, tol=0, t=0.9, w_fp=1, w_fn=1),
              "c": dict(k=None, tol=0, t=0.3, w_fp=1, w_fn=1), "d": dict(k=None, tol=0, t=0.2, w_fp=2, w_fn=1),
              "e": dict(k=None, tol=0, t=0.8, w_fp=1, w_fn=1), "f": dict(k=3, tol=0, t=0.5, w_fp=0.5, w_fn=0.5),
              "g": dict(k=8, tol=0.15, t=0.8, w_fp=1, w_fn=1), "g2": dict(k=8, tol=0.13, t=0.8, w_fp=1, w_fn=1),
              "h": dict(k=6, tol=0, t=0.8, w_fp=1, w_fn=1)}
    cases = {"a": run_case(PyBMF, Xa, params["a"]), "b": run_case(PyBMF, Xb, params["b"]), "c": run_case(PyBMF, Xa, params["c"]),
             "d": run_case(PyBMF, Xa, params["d"], may_raise=(TypeError,)),
             "e": run_case(PyBMF, np.zeros((20, 15), dtype=np.uint8), params["e"], may_raise=(TypeError,)),
             "f": run_case(PyBMF, Xf, params["f"])}
    cases["g"] = run_case(PyBMF, Xa, params["g"], may_raise=(TypeError,))
    cases["g2"] = run_case(PyBMF, Xa, params["g2"], may_raise=(TypeError,))
    cases["h"] = run_case(PyBMF, tr, params["h"], X_val=va, X_test=te)
    cases["h"]["X_val"], cases["h"]["X_test"] = va, te
    shipped = {"a": run_case(PyBMF, Xa, params["a"], stable=False, want_points=True),
               "c": run_case(PyBMF, Xa, params["c"], stable=False, want_points=True)}
    arrays, meta = {}, {"cases": {}, "shipped": {}}
    for name, c in cases.items():
        for key in ("X", "U", "V", "X_val", "X_test"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        meta["cases"][name] = dict(params[name], shape=list(c["X"].shape), log=c["log"], counts=c["counts"], n_calls=c["n_calls"],
                                   raised=c["raised"], truncations=c["truncations"])
        print(name, "rows:", len(c["log"]["rows"]), "factors kept:", c["U"].shape[1], "get_factor calls:", c["n_calls"], "counts:",
              c["counts"], "truncations:", c["truncations"], "raised:", c["raised"], "tol:", params[name]["tol"],
              "seconds per factor: {:.3f}".format(c["seconds"] / max(1, len(c["log"]["rows"]))))
    for name, c in shipped.items():
        for i, p in enumerate(c["points"]):
            for key in ("X_rs", "a", "b"):
                arrays[f"s{name}_p{i}_{key}"] = p[key]
        meta["shipped"][name] = dict(params[name], points=[{"index": p["index"], "axis": p["axis"], "mid": p["mid"]} for p in c["points"]])
        print("shipped", name, [(p["index"], p["axis"], p["mid"]) for p in c["points"]])
    np.savez_compressed(os.path.join(HERE, "g27_mebf.npz"), **arrays)
    with open(os.path.join(HERE, "g27_mebf.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
