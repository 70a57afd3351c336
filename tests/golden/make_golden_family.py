#!/usr/bin/env python3
"""Generate g26_boolean_family.{npz,json} by running the *reference* GreConD, Asso, AssoIter and AssoOpt (PyBMF @ 2024_10_08) on the
edge-case family of tests/boolean_family.py.

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only recorded outputs.  The inputs are not stored: family() and refine_start() of tests/boolean_family.py rebuild them from their
seeds (the fixture keeps each matrix's shape and number of ones as a guard).

    python tests/golden/make_golden_family.py          (about two minutes; most of it AssoOpt's subsets at 2049 rows)

Per model and case, one or two parameter sets of the case's grid:
  GreConD   the first of grecond_grid: k = None where the exact decomposition is short, else k = 3
  Asso      (tau 0.5, weights 0.5 / 0.5), (tau 0.3, weights 1 / 1) and (tau 0.3, weights 0.3 / 0.7), k = the case's k.  The products of
            0.3 and 0.7 with the counts are inexact and the reference adds them row by row, so where the largest score of a sweep is
            reached by two candidates, or equals the inherited best, exactly -- 7 T - 3 F equal as integers, which duplicate columns
            and equal blocks produce -- the reference's choice is an accident of rounding (make_golden_asso.py chooses its case g to
            avoid that).  integer_ties() finds such sweeps on the host stand-in; the record is then marked `rounding: true` and not
            compared.  The two exact weight pairs carry those cases.
  AssoIter  the flipped start of refine_start, weights 0.3 / 0.7
  AssoOpt   the flipped start, weights 1 / 1
Recorded: the log rows (time stamp dropped), U, V and X_pd as packed bits, the counts of X_pd against X_train, and per model what its
check in tests/test_{grecond,asso,asso_refine}_cpu.py reads (candidates kept and winners; column visits; j per row).

How the reference ends is recorded as `raised`.  A case on which the reference raises is kept for the property tests only (`usable:
false`): the TypeError inside the message stops of GreConD ("No pattern found": zeros, and every matrix of one row or one column,
where the reference finds no concept at all) and of Asso ("Candidate list is empty", "No pattern found.": zeros, low_rank), and the
IndexError of Asso on a matrix of one column.  AssoOpt is the exception to that rule: the reference always ends in an AttributeError
after U is final and before it logs, which is what check_opt of tests/test_asso_refine_cpu.py expects, so there a case is usable when
that is how it ended.  The generator asserts that per model the reference completes in this sense on at least three quarters of the
family, and writes the shares into the json.
"""
import json
import os
import sys
import time
import types

import numpy as np
from scipy.sparse import lil_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import load_reference  # noqa: E402
import make_golden_asso as MA  # noqa: E402
import make_golden_asso_refine as MR  # noqa: E402
import make_golden_grecond as MG  # noqa: E402
import boolean_family as F  # noqa: E402

ASSO_SETS = {"half": dict(tau=0.5, w_fp=0.5, w_fn=0.5), "ones": dict(tau=0.3, w_fp=1.0, w_fn=1.0), "skew": dict(tau=0.3, w_fp=0.3, w_fn=0.7)}

ITER_SET = dict(flipped=True, w_fp=0.3, w_fn=0.7)
OPT_SET = dict(flipped=True, w_fp=1.0, w_fn=1.0)
SHARE = 0.75


def attempt(run):
    """run() or the name of what it raised (the runners catch the known endings themselves)."""
    t0 = time.time()
    try:
        out = run()
        out["state"] = True
    except Exception as exc:      # noqa: BLE001  whatever the reference dies of on an edge case is the finding
        out = {"state": False, "raised": type(exc).__name__}
    out["seconds"] = time.time() - t0
    return out


def integer_ties(name, tau):
    """Whether a sweep of the case's Asso fit at weights 0.3 / 0.7 has an exact tie at its top: 10 x score = 7 T - 3 F as integers."""
    import test_asso_cpu as A
    ties = []

    def factory(model):
        eng = A.numpy_engine(model)
        best = eng.best

        def logged(best_score, w_fp, w_fn, block=None):
            tp, fp = eng.row_counts()
            T, Fp, _, _, _ = A.score_block(eng.X, eng.pd, eng.basis, eng.m, eng.list, tp, fp, w_fp, w_fn, best_score)
            tenfold, inherited = 7 * T - 3 * Fp, int(round(10 * best_score))
            if tenfold.size:
                top = int(tenfold.max())
                ties.append(top == inherited or (top > inherited and int((tenfold == top).sum()) > 1))
            return best(best_score, w_fp, w_fn, block)
        eng.best = logged
        return eng
    A.fit_case(dict(F.family()[name], tau=tau, w_fp=0.3, w_fn=0.7), factory)
    return any(ties)


def stand_in(name, flipped):
    U, V = F.refine_start(name, flipped)
    return types.SimpleNamespace(k=U.shape[1], U=lil_matrix(U.astype(np.float64)), V=lil_matrix(V.astype(np.float64)), logs={})


def main():
    PyBMF = load_reference()
    fam = F.family()
    arrays, meta = {}, {"cases": {}, "guard": {n: [c["shape"], int(c["X"].sum())] for n, c in fam.items()}}
    keep = {"GreConD": ("U", "V"), "Asso": ("U", "V", "X_pd", "kept"), "AssoIter": ("U",), "AssoOpt": ("U", "j")}
    scalars = ("counts", "log", "raised", "n_calls", "winners", "visits", "k", "w_fp", "w_fn", "tau", "cells_changed", "state", "completed", "usable", "rounding")
    for name, c in fam.items():
        X, va, te = c["X"], c.get("X_val"), c.get("X_test")
        runs = {}
        k_g = F.grecond_grid(name)[0]["k"]
        runs["GreConD/" + name] = dict(attempt(lambda: MG.run_case(PyBMF, X, k_g, 0, va, te, may_raise=(TypeError,))), k=k_g)
        for tag, p in ASSO_SETS.items():
            runs[f"Asso/{name}/{tag}"] = dict(attempt(lambda: MA.run_case(PyBMF, X, p["tau"], c["k"], 0, p["w_fp"], p["w_fn"], va, te,
                                                                           may_raise=(TypeError,))), k=c["k"], **p)
        U_in = F.refine_start(name, True)[0]
        it = attempt(lambda: MR.run_iter(stand_in(name, True), X, ITER_SET["w_fp"], ITER_SET["w_fn"], va, te))
        op = attempt(lambda: MR.run_opt(stand_in(name, True), X, OPT_SET["w_fp"], OPT_SET["w_fn"]))
        for r in (it, op):
            if r["state"]:
                assert (r["U_in"] == U_in).all()
                r["cells_changed"] = int((r["U"] != U_in).sum())
        runs["AssoIter/" + name], runs["AssoOpt/" + name] = it, op
        for key, r in runs.items():
            for a in keep[key.split("/")[0]]:
                if r.get(a) is not None and r["state"]:      # (a state the reference left behind an exception is kept for the record)
                    arr = np.asarray(r[a])
                    arrays[f"{key}/{a}"] = arr.astype(np.int32) if a in ("kept", "j") else np.packbits(arr.astype(bool).ravel())
                    r.setdefault("shapes", {})[a] = list(arr.shape)
            r["completed"] = bool(r["state"] and r.get("raised") == ("AttributeError" if key.startswith("AssoOpt/") else None))
            if key.endswith("/skew") and r["state"]:
                r["rounding"] = bool(integer_ties(name, r["tau"]))
            r["usable"] = bool(r["completed"] and not r.get("rounding", False))
            meta["cases"][key] = {s: r[s] for s in scalars + ("shapes",) if s in r}      # (no timings: a second run writes the same json)
            print(f"{key:28s} state: {r['state']!s:5s} raised: {r.get('raised')!s:15s} rows: {len(r.get('log', {}).get('rows', []))} "
                  f"{r['seconds']:.1f} s", flush=True)
    meta["share"] = {}
    for model in keep:
        mine = [r for key, r in meta["cases"].items() if key.startswith(model + "/")]
        by_case = {}
        for key, r in meta["cases"].items():
            if key.startswith(model + "/"):
                by_case.setdefault(key.split("/")[1], []).append(r)
        done = [name for name, rs in by_case.items() if all(r["completed"] for r in rs)]
        meta["share"][model] = {"completed": len(done), "of": len(by_case), "not_completed": sorted(set(by_case) - set(done))}
        print(f"{model}: {len(mine)} runs; the reference completes on {len(done)} of {len(by_case)} cases ({len(done) / len(by_case):.0%}); "
              f"not on {meta['share'][model]['not_completed']}")
        assert len(done) >= SHARE * len(by_case), f"{model}: the reference completes on too few cases of the family; replace cases"
    np.savez_compressed(os.path.join(HERE, "g26_boolean_family.npz"), **arrays)
    with open(os.path.join(HERE, "g26_boolean_family.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
