#!/usr/bin/env python3
"""Generate g25_asso_refine.{npz,json} by running the *reference* AssoIter and AssoOpt (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_asso_refine.py          (about a minute, most of it the exhaustive searches)

The model that goes in is the reference's Asso on the case's X (tau 0.4, k = 6, w_fp = 0.5) unless said otherwise; "stand-in" is an
object with k, U, V, logs and random factors.  X is planted(m, n, 5, 0.2, 0.06, seed) of make_golden_grecond.

  Iter-a, b, c  96 x 72, seed 11;  AssoIter weights w_fp = 0.3 / w_fp = 0.7 / w_fp = 1, w_fn = 1
  Iter-d        the first seed from 12 on whose run (w_fp = 0.7) goes into a second round and refines a column after a skipped one
  Iter-e        the ones of Iter-a's X dealt to train / val / test (70 / 15 / 15 %), w_fp = 0.3; the first deal seed from 2504 on whose
                run logs a row
  Opt-a, b      96 x 72, seed 11, k = 6;  AssoOpt weights 1 / 1 and 0.3 / 0.7
  Opt-c         40 x 30, Asso with k = 1, weights 1 / 1
  Opt-d         40 x 30, stand-in with k = 8, weights 0.3 / 0.7
  Opt-e         24 x 20, stand-in with k = 4 whose factor 2 is empty in V, a row of X all zero, weights 1 / 1

Recorded per case: X (and X_val, X_test), U and V that go in, U that comes out, the counts of X_pd against X, the rows of
logs['refinements'] without the time stamp.  AssoIter: every column visit as (k, error, refined or skipped), from a wrapped
get_refined_column and the module's ERR.  AssoOpt: the j that set_optimal_row returned per row, the name of the exception the
reference ends in (AttributeError: it has no attribute 'w'; U and X_pd are final by then, nothing is logged) and the seconds it took.
The generator asserts that at least one cell of U changes in Iter-a .. d and Opt-a, b, d.
"""
import json
import os
import sys
import time
import types

import numpy as np
from scipy.sparse import csr_matrix, lil_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402
from make_golden_asso import flat_log  # noqa: E402
from make_golden_grecond import deal, dense_u8, planted  # noqa: E402


def sp(X):
    return None if X is None else csr_matrix(X.astype(np.float64))


def asso_model(X, k, X_val=None, X_test=None, tau=0.4):
    from PyBMF.models import Asso
    show = Asso.show_matrix
    Asso.show_matrix = lambda self, *a, **kw: None    # init_model plots unconditionally
    try:
        with quiet():
            model = Asso(tau=tau, k=k, w_fp=0.5)
            model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
    finally:
        Asso.show_matrix = show
    assert model.U.shape[1] == k
    return model


def stand_in(m, n, k, seed, empty=()):
    rng = np.random.RandomState(seed)
    U, V = (rng.rand(m, k) < 0.3).astype(np.float64), (rng.rand(n, k) < 0.3).astype(np.float64)
    V[:, list(empty)] = 0
    return types.SimpleNamespace(k=k, U=lil_matrix(U), V=lil_matrix(V), logs={})


def run_iter(model, X, w_fp, w_fn, X_val=None, X_test=None):
    from PyBMF.models import AssoIter
    mod = sys.modules["PyBMF.models.AssoIter"]
    model = types.SimpleNamespace(k=model.k, U=model.U.copy(), V=model.V.copy(), logs={})
    U_in, V_in = dense_u8(model.U), dense_u8(model.V)
    errors, cols = [], []
    err = mod.ERR

    def logged_err(gt, pd):
        errors.append(float(err(gt=gt, pd=pd)))
        return errors[-1]
    mod.ERR = logged_err
    try:
        with quiet():
            ref = AssoIter(model=model, w_fp=w_fp, w_fn=w_fn)
            inner = ref.get_refined_column
            ref.get_refined_column = lambda k: (cols.append(int(k)), inner(k))[1]
            t0 = time.time()
            ref.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
            seconds = time.time() - t0
    finally:
        mod.ERR = err
    assert len(errors) == len(cols) + 1
    best, visits = errors[0], []
    for k, e in zip(cols, errors[1:]):
        visits.append([k, e, bool(e < best)])
        best = min(best, e)
    log = flat_log(ref.logs["refinements"]) if "refinements" in ref.logs else {"columns": [], "rows": []}
    assert len(log["rows"]) == sum(v[2] for v in visits)
    return dict(X=X, U_in=U_in, V=V_in, U=dense_u8(ref.U), counts=counts_of(None, sp(X), csr_matrix(ref.X_pd)), log=log, visits=visits,
                error0=errors[0], seconds=seconds, w_fp=w_fp, w_fn=w_fn, k=int(model.k))


def run_opt(model, X, w_fp, w_fn):
    from PyBMF.models import AssoOpt
    model = types.SimpleNamespace(k=model.k, U=model.U.copy(), V=model.V.copy(), logs={})
    U_in, V_in = dense_u8(model.U), dense_u8(model.V)
    chosen, raised = {}, None
    with quiet():
        ref = AssoOpt(model=model, w_fp=w_fp, w_fn=w_fn)
        inner = ref.set_optimal_row

        def logged(i):
            chosen[int(i)] = int(inner(i))
            return chosen[int(i)]
        ref.set_optimal_row = logged
        t0 = time.time()
        try:
            ref.fit(sp(X), **FIT_KW)
        except AttributeError as exc:
            raised = type(exc).__name__
        seconds = time.time() - t0
    assert sorted(chosen) == list(range(X.shape[0]))
    log = flat_log(ref.logs["refinements"]) if "refinements" in ref.logs else {"columns": [], "rows": []}
    return dict(X=X, U_in=U_in, V=V_in, U=dense_u8(ref.U), counts=counts_of(None, sp(X), csr_matrix(ref.X_pd)), log=log,
                j=np.array([chosen[i] for i in range(X.shape[0])], dtype=np.int32), raised=raised, seconds=seconds, w_fp=w_fp, w_fn=w_fn,
                k=int(model.k))


def changed(c):
    return int((c["U"] != c["U_in"]).sum())


def main():
    load_reference()
    Xa = planted(96, 72, 5, 0.2, 0.06, 11)
    base = asso_model(Xa, 6)
    cases = {"iter_a": run_iter(base, Xa, 0.3, None), "iter_b": run_iter(base, Xa, 0.7, None), "iter_c": run_iter(base, Xa, 1.0, 1.0)}
    for seed in range(12, 80):               # the first seed with a second round and a refinement after a skip
        Xd = planted(96, 72, 5, 0.2, 0.06, seed)
        try:
            d = run_iter(asso_model(Xd, 6), Xd, 0.7, None)
        except (AssertionError, TypeError):  # Asso found fewer than 6 factors on this seed
            continue
        flags = [v[2] for v in d["visits"]]
        if len(flags) > d["k"] and any((not a) and any(flags[i + 1:]) for i, a in enumerate(flags)):
            cases["iter_d"] = dict(d, seed=seed)
            break
    d = cases["iter_d"]
    flags = [v[2] for v in d["visits"]]
    assert len(flags) > d["k"] and any((not a) and any(flags[i + 1:]) for i, a in enumerate(flags))
    for seed in range(2504, 2544):           # the first deal whose run logs a row, so that the val / test columns are recorded
        tr, va, te = deal(Xa, seed)
        try:
            e = run_iter(asso_model(tr, 6, va, te), tr, 0.3, None, va, te)
        except (AssertionError, TypeError):
            continue
        if e["log"]["rows"]:
            cases["iter_e"] = dict(e, X_val=va, X_test=te, seed=seed)
            break
    assert cases["iter_e"]["log"]["rows"]
    cases["opt_a"] = run_opt(base, Xa, 1, 1)
    cases["opt_b"] = run_opt(base, Xa, 0.3, 0.7)
    Xc = planted(40, 30, 4, 0.25, 0.06, 2505)
    cases["opt_c"] = run_opt(asso_model(Xc, 1), Xc, 1, 1)
    cases["opt_d"] = run_opt(stand_in(40, 30, 8, 2506), Xc, 0.3, 0.7)
    Xe = planted(24, 20, 3, 0.3, 0.05, 2507)
    Xe[5] = 0
    cases["opt_e"] = run_opt(stand_in(24, 20, 4, 2508, empty=(2,)), Xe, 1, 1)
    for name in ("iter_a", "iter_b", "iter_c", "iter_d", "opt_a", "opt_b", "opt_d"):
        assert changed(cases[name]) >= 1, name
    arrays, meta = {}, {"cases": {}}
    for name, c in cases.items():
        for key in ("X", "X_val", "X_test", "U_in", "V", "U", "j"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        meta["cases"][name] = {key: c[key] for key in ("w_fp", "w_fn", "k", "counts", "log", "visits", "error0", "raised", "seconds", "seed")
                               if key in c}
        meta["cases"][name].update(shape=list(c["X"].shape), cells_changed=changed(c))
        print(name, "k:", c["k"], "cells of U changed:", changed(c), "rows logged:", len(c["log"]["rows"]), "visits:", len(c.get("visits", [])),
              "counts:", c["counts"], "raised:", c.get("raised"), "seconds: %.2f" % c["seconds"])
    np.savez_compressed(os.path.join(HERE, "g25_asso_refine.npz"), **arrays)
    with open(os.path.join(HERE, "g25_asso_refine.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
