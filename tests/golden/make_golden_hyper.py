#!/usr/bin/env python3
"""Generate g30_hyper.{npz,json} by running the *reference* Hyper (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_hyper.py          (a few minutes: the reference evaluates one candidate per sparse-matrix pass)

Two things are put in place of what the reference's Hyper module sees:
  * `apriori` (mlxtend is absent): `apriori` below, a small dense miner of the definition this build adopts -- levels ascend, inside a
    level the itemsets are in lexicographic order of their ascending column tuples, an itemset is frequent iff count / m >=
    min_support in fp64.  Believed to be mlxtend's set and order; not checked against mlxtend.
  * `np`: the StableNumpy proxy of make_golden_mebf.py, so that sort_by_cost's argsort is stable, the order this build defines.
Cases:
  a  40 x 30, noise-free product of 4 factors (density 0.3, seed 2), min_support 0.3    thousands of head evaluations (`iter`)
  b  33 x 65, 3 planted factors (density 0.3, 3 % flips, seed 9), min_support 0.52     a few dozen itemsets
  c  case a's X, min_support 0.99                                      above every pair's support: singletons only
  d  24 x 16 noise-free, column 7 a copy of column 3, min_support 0.25   tied costs: the stable rule decides
  e  a noise-free planted matrix found by a seed search (below) in which a stale head is accepted: the T of at least one factor
     differs from find_hyper of its itemset on the residual of that moment
  f  20 x 15 of zeros                                                  no candidate survives, no round runs
  g  12 x 1                                                            c[1] on a list of one: IndexError
  h  case a's ones dealt to train / val / test (70 / 15 / 15 %), min_support 0.2
For each: the matrices (uint8), min_support, the mined itemsets in order with their counts, every row of logs['updates'] without the
time stamp (k, iter, |T|, |I|, then the four metrics per data set), T, I, U, V, k, the integer TP / FP / FN / TN of the final X_pd
against X_train, per factor whether its T was stale, the exception's name where the run raises.

Every `c[0] > c[1]` decision of the fits is traced: the two costs are ratios of small integers, and each decision is asserted to be
either an exact equality of the two rationals or more than 1e-9 apart, so no recorded decision hangs on a rounding.
"""
import inspect
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pandas as pd
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402
from make_golden_grecond import deal, dense_u8, planted  # noqa: E402
from make_golden_mebf import StableNumpy  # noqa: E402


def apriori(df, min_support):
    """The stand-in miner: a DataFrame with `support` and `itemsets` (frozensets), singletons included, in the defined order."""
    X = np.asarray(df) != 0
    m, n = X.shape
    out, level = [], [(j,) for j in range(n)]
    while level:
        found = []
        for cols in level:
            count = int(X[:, list(cols)].all(axis=1).sum())
            if np.float64(count) / m >= min_support:
                found.append((cols, count))
        out += found
        level = sorted(cols + (j,) for cols, _ in found for j in range(cols[-1] + 1, n))
    return pd.DataFrame({"support": [c / m for _, c in out], "itemsets": [frozenset(cols) for cols, _ in out], "count": [c for _, c in out]})


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
            elif name in ("k", "iter"):
                names.append(name)
                row.append(int(v))
            else:
                names.append(name)
                row.append(float(v))
        rows.append(row)
    return {"columns": names, "rows": rows}


def run_case(PyBMF, X, min_support, X_val=None, X_test=None):
    from PyBMF.models import Hyper
    mod = sys.modules["PyBMF.models.Hyper"]   # the module, not the class of the same name
    mined, stale, decisions = [], [], []

    def miner(df, min_support):
        out = apriori(df, min_support)
        mined.append(out)
        return out[["support", "itemsets"]].copy()

    src, first = inspect.getsourcelines(Hyper._fit)
    test_line = first + next(i for i, line in enumerate(src) if "while self.c[0] > self.c[1]" in line)
    code = Hyper._fit.__code__

    def cost_of(model, i):
        """The cost of list position i as a rational: its numerator is known, its denominator is the integer that gives the float."""
        if model.c[i] == np.inf:
            return None
        num = len(model.T[i]) + len(model.I[i])
        den = int(round(num / model.c[i]))
        assert np.float64(num) / np.float64(den) == model.c[i]
        return Fraction(num, den)

    def local_trace(frame, event, arg):
        if event == "line" and frame.f_lineno == test_line:
            model = frame.f_locals["self"]
            if len(model.c) >= 2:
                a, b = cost_of(model, 0), cost_of(model, 1)
                if a is not None and b is not None:
                    assert a == b or abs(model.c[0] - model.c[1]) > 1e-9, (a, b)
                    decisions.append(a == b)
        return local_trace

    def tracer(frame, event, arg):
        return local_trace if frame.f_code is code else None

    def sp(A):
        return None if A is None else csr_matrix(A.astype(np.float64))
    saved = mod.np, mod.apriori
    mod.np, mod.apriori = StableNumpy(True), miner
    raised, t0 = None, time.time()
    try:
        with quiet():
            model = Hyper(min_support=min_support)
            set_factors = model.set_factors

            def logged(k, u, v):
                fresh, _ = Hyper.find_hyper(I=model.I[0], X_gt=model.X_train, X_rs=model.X_rs)
                stale.append(set(fresh) != set(model.T[0]))
                return set_factors(k, u=u, v=v)
            model.set_factors = logged
            sys.settrace(tracer)
            try:
                model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
            except IndexError as exc:
                raised = type(exc).__name__
            finally:
                sys.settrace(None)
    finally:
        mod.np, mod.apriori = saved
    seconds = time.time() - t0
    log = flat_log(model.logs["updates"]) if "updates" in getattr(model, "logs", {}) else {"columns": [], "rows": []}
    sets = mined[0][mined[0]["itemsets"].apply(len) > 1]
    out = dict(X=X, U=dense_u8(csr_matrix(model.U)), V=dense_u8(csr_matrix(model.V)), raised=raised, log=log, stale=stale,
               itemsets=[sorted(int(j) for j in s) for s in sets["itemsets"]], itemset_counts=[int(c) for c in sets["count"]],
               decisions=len(decisions), ties=int(sum(decisions)), seconds=seconds)
    if not raised:
        out.update(T=[sorted(int(t) for t in T) for T in model.T], I=[sorted(int(j) for j in I) for I in model.I], k=int(model.k))
    X_pd = csr_matrix(model.X_pd) if getattr(model, "X_pd", None) is not None else csr_matrix(X.shape)
    out["counts"] = counts_of(PyBMF, sp(X), X_pd)
    return out


def main():
    PyBMF = load_reference()
    Xa = planted(40, 30, 4, 0.3, 0.0, 2)
    Xb = planted(33, 65, 3, 0.3, 0.03, 9)
    Xd = planted(24, 16, 3, 0.3, 0.0, 3001)
    Xd[:, 7] = Xd[:, 3]
    Xe = planted(*STALE[:3], STALE[3], 0.0, STALE[4])
    Xg = (np.arange(12)[:, None] % 3 != 0).astype(np.uint8)
    tr, va, te = deal(Xa, 3004)
    support = {"a": 0.3, "b": 0.52, "c": 0.99, "d": 0.25, "e": STALE[5], "f": 0.5, "g": 0.5, "h": 0.2}
    cases = {"a": run_case(PyBMF, Xa, support["a"]), "b": run_case(PyBMF, Xb, support["b"]), "c": run_case(PyBMF, Xa, support["c"]),
             "d": run_case(PyBMF, Xd, support["d"]), "e": run_case(PyBMF, Xe, support["e"]),
             "f": run_case(PyBMF, np.zeros((20, 15), dtype=np.uint8), support["f"]), "g": run_case(PyBMF, Xg, support["g"]),
             "h": run_case(PyBMF, tr, support["h"], X_val=va, X_test=te)}
    cases["h"]["X_val"], cases["h"]["X_test"] = va, te
    assert any(cases["e"]["stale"]), "case e holds no stale head: search another seed"
    arrays, meta = {}, {"cases": {}}
    for name, c in cases.items():
        for key in ("X", "U", "V", "X_val", "X_test"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        meta["cases"][name] = dict(min_support=support[name], shape=list(c["X"].shape), log=c["log"], counts=c["counts"], raised=c["raised"],
                                   itemsets=c["itemsets"], itemset_counts=c["itemset_counts"], stale=[bool(x) for x in c["stale"]],
                                   decisions=c["decisions"], ties=c["ties"], T=c.get("T"), I=c.get("I"), k=c.get("k"))
        print(name, "itemsets:", len(c["itemsets"]), "rows:", len(c["log"]["rows"]), "iter:", [r[1] for r in c["log"]["rows"]], "stale:",
              [int(x) for x in c["stale"]], "decisions:", c["decisions"], "ties:", c["ties"], "counts:", c["counts"], "raised:", c["raised"],
              "seconds: {:.1f}".format(c["seconds"]))
    meta["cases"]["d"]["duplicate"] = [3, 7]
    np.savez_compressed(os.path.join(HERE, "g30_hyper.npz"), **arrays)
    with open(os.path.join(HERE, "g30_hyper.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


# case e: (m, n, planted factors, density, seed, min_support), the first hit of a search over seeds 3100 .. with the stand-in replay
STALE = (30, 20, 4, 0.3, 3100, 0.3)

if __name__ == "__main__":
    main()
