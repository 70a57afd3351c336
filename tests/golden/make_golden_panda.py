#!/usr/bin/env python3
"""Generate g28_panda.{npz,json} by running the *reference* Panda (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_panda.py          (about a minute)

(i) Full fits under the defined tie rule.  The reference orders its extension list E with np.flip(np.argsort(scores)) and NumPy's
default sort is not stable: the order inside a tie group depends on the sort kernel of the host, and on the 96 x 72 matrix below the
shipped reference and a stable sort give different factors for all three init_methods.  This build defines the order as
np.flip(np.argsort(scores, kind='stable')) applied to E in its current order, so for these fits the `np` that the reference's Panda
module sees is the StableNumpy proxy of make_golden_mebf.py.
  a, b, c  96 x 72, 4 planted factors, 3 % flips, k = 5, init_method frequency / couples-frequency / correlation: 6 factors each
           (early_stop sees n_factors before it is incremented)
  d  the same X, k = None, w_model = 0.5, w_fp = 2, w_fn = 1, correlation: runs until "Error starts increasing.", where the
     reference's own early_stop raises TypeError (it calls _early_stop without `verbose`); the rows and factors so far are kept
  e  33 x 65, 3 planted factors (density 0.3, 3 % flips, seed 9), k = 4, exact_decomp = True
  f  the same X, k = None, defaults: many 1-row patterns, then the TypeError stop
  g  40 x 30, noise-free product of 4 factors, k = None: error <= tol = 0 truncates the last factor
  h  the same X, k = 8, w_model = 0.3, w_fp = 0.7, w_fn = 1.1, correlation
  i  the X of e, k = 6, w_model = 2, w_fp = 1, w_fn = 1.5, couples-frequency
  j  20 x 15 of zeros, k = 3: "No pattern found." at once, the same TypeError
  k  case a's ones dealt to train / val / test (70 / 15 / 15 %), k = 5, defaults
For each: the matrices (uint8), every row of logs['updates'] without `time` (cost, |T|, |I|, then the four metrics per data set), the
final U and V, the integer TP / FP / FN / TN of the final X_pd against X_train, the exception's name where the run raises.  For b, c
and d also, per factor, (T, I, E, cost_now) after find_core and after extend_core.

Every decision of the reference is `quantity <= 0` in fp64: the core's d_cost, the extension's cost_new - cost_old and the row rule's
d.  They are read from the running reference with a line tracer; for the weights of cases h and i every one of
them must be more than 1e-9 away from zero, or the fixture would pin a rounding.  The weights of case d (0.5, 2, 1) are multiples of
1 / 2: every quantity is an exact multiple of 1 / 2, some are exactly zero -- ties that no rounding can move -- and that is what
is asserted there.

(ii) The reference as shipped (the default argsort), cases a and c: for the first, a middle and the last sort_items call the method,
the residual and T that went in, and E before and after.
"""
import json
import linecache
import os
import sys
import time

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402
from make_golden_grecond import deal, dense_u8, planted  # noqa: E402
from make_golden_mebf import StableNumpy, flat_log  # noqa: E402

MARGIN = 1e-9
DECISION_LINES = {"find_core": ("if d_cost <= 0", lambda f: [f["d_cost"]]),
                  "extend_core": ("if cost_new <= cost_old", lambda f: [f["cost_new"] - f["cost_old"]]),
                  "extend_core rows": ("idx = to_dense(d_cost", lambda f: np.asarray(f["d_cost"], dtype=np.float64).ravel().tolist())}


def flat(x):
    return (np.asarray(csr_matrix(x).todense()).ravel() != 0).astype(np.uint8)


class DecisionTracer:
    """Collects the quantities the reference compares with zero, read from its frames as the lines that test them are reached."""

    def __init__(self):
        self.seen = {name: [] for name in DECISION_LINES}

    def __call__(self, frame, event, arg):
        code = frame.f_code
        if code.co_name in ("find_core", "extend_core") and code.co_filename.endswith("Panda.py"):
            return self.local
        return None

    def local(self, frame, event, arg):
        if event == "line":
            text = linecache.getline(frame.f_code.co_filename, frame.f_lineno).strip()
            for name, (start, read) in DECISION_LINES.items():
                if name.split()[0] == frame.f_code.co_name and text.startswith(start):
                    self.seen[name] += [float(v) for v in read(frame.f_locals)]
        return self.local

    def margin(self):
        return min([abs(v) for vs in self.seen.values() for v in vs] or [np.inf])

    def halves(self):
        return all(2 * v == int(2 * v) for vs in self.seen.values() for v in vs)


def run_case(PyBMF, X, params, X_val=None, X_test=None, stable=True, want_steps=False, want_sorts=False, may_raise=(), trace=True):
    from PyBMF.models import Panda
    mod = sys.modules["PyBMF.models.Panda"]   # the module, not the class of the same name
    proxy, steps, sorts = StableNumpy(stable), [], []
    find_core, extend_core, sort_items = Panda.find_core, Panda.extend_core, Panda.sort_items

    def snap(self, stage):
        steps.append(dict(stage=stage, T=flat(self.T), I=flat(self.I), E=[int(e) for e in self.E], cost=float(self.cost_now)))

    def logged_core(self):
        find_core(self)
        snap(self, "core")

    def logged_ext(self):
        extend_core(self)
        snap(self, "ext")

    def logged_sort(self, method):
        before = [int(e) for e in self.E]
        rec = dict(method=method, X_rs=dense_u8(csr_matrix(self.X_rs)), T=flat(self.T) if self.T.shape[0] == X.shape[0] else None,
                   before=before)
        sort_items(self, method)
        rec["after"] = [int(e) for e in self.E]
        sorts.append(rec)

    def sp(A):
        return None if A is None else csr_matrix(A.astype(np.float64))
    saved_np, mod.np = mod.np, proxy
    if want_steps:
        Panda.find_core, Panda.extend_core = logged_core, logged_ext
    if want_sorts:
        Panda.sort_items = logged_sort
    tracer, raised, t0 = DecisionTracer(), None, time.time()
    try:
        with quiet():
            model = Panda(**params)
            sys.settrace(tracer if trace else None)
            try:
                model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
            except may_raise as exc:
                raised = type(exc).__name__
            finally:
                sys.settrace(None)
    finally:
        mod.np, Panda.find_core, Panda.extend_core, Panda.sort_items = saved_np, find_core, extend_core, sort_items
    seconds = time.time() - t0
    log = flat_log(model.logs["updates"]) if "updates" in getattr(model, "logs", {}) else {"columns": [], "rows": []}
    f = len(log["rows"]) if raised else model.U.shape[1]
    out = dict(X=X, U=dense_u8(csr_matrix(model.U))[:, :f], V=dense_u8(csr_matrix(model.V))[:, :f], raised=raised, log=log, steps=steps,
               sorts=sorts, seconds=seconds, margin=tracer.margin(), halves=tracer.halves(), decisions={k: len(v) for k, v in tracer.seen.items()})
    X_pd = csr_matrix(model.X_pd) if getattr(model, "X_pd", None) is not None else csr_matrix(X.shape)
    out["counts"] = counts_of(PyBMF, sp(X), X_pd)
    return out


def main():
    PyBMF = load_reference()
    Xa = planted(96, 72, 4, 0.2, 0.03, 2301)
    Xe = planted(33, 65, 3, 0.3, 0.03, 9)
    Xg = planted(40, 30, 4, 0.25, 0.0, 2303)
    tr, va, te = deal(Xa, 2304)

    def P(k, w_model=1, w_fp=1, w_fn=1, init_method="correlation", exact_decomp=False):
        return dict(k=k, tol=0, w_model=w_model, w_fp=w_fp, w_fn=w_fn, init_method=init_method, exact_decomp=exact_decomp)
    params = {"a": P(5, init_method="frequency"), "b": P(5, init_method="couples-frequency"), "c": P(5),
              "d": P(None, w_model=0.5, w_fp=2, w_fn=1), "e": P(4, exact_decomp=True), "f": P(None), "g": P(None),
              "h": P(8, w_model=0.3, w_fp=0.7, w_fn=1.1), "i": P(6, w_model=2, w_fp=1, w_fn=1.5, init_method="couples-frequency"),
              "j": P(3), "k": P(5)}
    data = {"a": Xa, "b": Xa, "c": Xa, "d": Xa, "e": Xe, "f": Xe, "g": Xg, "h": Xg, "i": Xe, "j": np.zeros((20, 15), dtype=np.uint8), "k": tr}
    cases = {}
    for name in params:
        extra = dict(X_val=va, X_test=te) if name == "k" else {}
        cases[name] = run_case(PyBMF, data[name], params[name], want_steps=name in "bcd", may_raise=(TypeError,), **extra)
        cases[name].update(extra)
    plain = run_case(PyBMF, Xa, params["c"], trace=False)
    assert plain["log"] == cases["c"]["log"]
    print("c without the line tracer: seconds per factor: {:.3f}".format(plain["seconds"] / len(plain["log"]["rows"])))
    shipped = {name: run_case(PyBMF, Xa, params[name], stable=False, want_sorts=True) for name in ("a", "c")}
    arrays, meta = {}, {"cases": {}, "shipped": {}}
    for name, c in cases.items():
        p = params[name]
        if name in "hi":
            assert c["margin"] > MARGIN, (name, c["margin"])
        if name == "d":      # multiples of 1 / 2: every quantity is exact, a zero among them is a tie and no rounding
            assert all(2 * float(p[w]) == int(2 * p[w]) for w in ("w_model", "w_fp", "w_fn")) and c["halves"], name
        for key in ("X", "U", "V", "X_val", "X_test"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        if c["steps"]:
            width = max(len(s["E"]) for s in c["steps"])
            arrays[f"{name}_steps_T"] = np.array([s["T"] for s in c["steps"]], dtype=np.uint8)
            arrays[f"{name}_steps_I"] = np.array([s["I"] for s in c["steps"]], dtype=np.uint8)
            arrays[f"{name}_steps_E"] = np.array([s["E"] + [-1] * (width - len(s["E"])) for s in c["steps"]], dtype=np.int16)
        meta["cases"][name] = dict(p, shape=list(c["X"].shape), log=c["log"], counts=c["counts"], raised=c["raised"],
                                   steps=[dict(stage=s["stage"], cost=s["cost"]) for s in c["steps"]])
        rows = len(c["log"]["rows"])
        print(name, "rows:", rows, "factors kept:", c["U"].shape[1], "counts:", c["counts"], "raised:", c["raised"], "decisions:",
              c["decisions"], "margin: {:.3g}".format(c["margin"]), "seconds per factor: {:.3f}".format(c["seconds"] / max(1, rows)))
    for name, c in shipped.items():
        calls = c["sorts"]
        points = [calls[i] for i in (0, len(calls) // 2, len(calls) - 1)]
        for i, s in enumerate(points):
            arrays[f"s{name}_p{i}_X_rs"] = s["X_rs"]
            arrays[f"s{name}_p{i}_T"] = s["T"] if s["T"] is not None else np.zeros(Xa.shape[0], dtype=np.uint8)
            arrays[f"s{name}_p{i}_before"] = np.array(s["before"], dtype=np.int16)
            arrays[f"s{name}_p{i}_after"] = np.array(s["after"], dtype=np.int16)
        meta["shipped"][name] = dict(params[name], n_calls=len(calls), points=[dict(method=s["method"]) for s in points])
        print("shipped", name, "sort_items calls:", len(calls), [s["method"] for s in points], "rows:", len(c["log"]["rows"]))
    np.savez_compressed(os.path.join(HERE, "g28_panda.npz"), **arrays)
    with open(os.path.join(HERE, "g28_panda.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
