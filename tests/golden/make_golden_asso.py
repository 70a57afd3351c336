#!/usr/bin/env python3
"""Generate g24_asso.{npz,json} by running the *reference* Asso (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_asso.py          (about half a minute, most of it case b)

Cases (planted Boolean factors of make_golden_grecond.planted, fixed RandomState seeds):
  a  96 x 72, tau 0.4, k = 5, weights 0.5 / 0.5                        stops on "Reach requested factor"
  b  200 x 150, tau 0.35, k = None, tol = 0.11                         error <= tol fires at the fifth factor (see below)
  c  40 x 30, tau 0.5, k = None, tol = 0                                runs until no candidate improves the score
  d  the ones of case a's X dealt to train / val / test (70 / 15 / 15 %), k = 5, task = 'reconstruction'
  e  20 x 15 of zeros, k = None                                         the candidate list is empty at once
  f  case a's X, tau 0.6, weights 1 / 1, k = 4
  g  96 x 72, tau 0.4, w_fp = 0.3 (w_fn = None: 1 - 0.3), k = 5         weights whose products with the counts are inexact

What the reference does, as recorded (the fixtures are the authority):
  * the winner of a sweep is the candidate with the LARGEST score above the inherited best_score, the first of equals (the loop
    replaces its best on every strict improvement);
  * `is_improving = early_stop(error=..., k=k)` is overwritten by `is_improving = early_stop(n_factor=k+1)` on the next line.  With
    k = None the tolerance stop therefore truncates the factor just added and the fit GOES ON: the next factor lands in column k + 1
    behind an empty column k, X_pd is rebuilt from the truncated factors, best_score stays inherited.  In case b the sweep that
    follows the truncation finds nothing above the inherited score, and the fit ends in the message stop.
  * both message stops ("Candidate list is empty", "No pattern found.") raise a TypeError inside early_stop (it calls _early_stop
    without `verbose`), so cases b, c and e end in that exception: the fixture records the log rows, U, V and X_pd as they stood.
For each case: the matrices (uint8), the candidate matrix before empty rows are dropped and the kept row indices, every log row with
`shape` flattened to n_u, n_v and array cells written as floats, U, V, the counts of X_pd against X_train.  For cases a and b the
input (X_pd, s_old, list, best_score) and full output (score and vector per candidate) of the first and a middle get_vector sweep.
For every sweep of every case: the relative margin of the winner's score to the nearest other candidate's score and to the
inherited best_score (of the largest score to best_score when nothing wins); case g's seed is chosen so that all exceed 1e-9.
The reference's time per factor of case b on this CPU goes into the json (`seconds_per_factor`).
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

MARGIN = 1e-9


def flat_log(df):
    """Rows of the log without the time stamp; `shape` [|u|, |v|] becomes two integer columns, every other cell a float."""
    cols = [str(c[-1]) if c[0] == "" else "{}/{}".format(c[0], c[-1]) for c in df.columns]
    names, rows = [], []
    for _, r in df.iterrows():
        names, row = [], []
        for name, v in zip(cols, r.tolist()):
            if name == "time":
                continue
            if name == "train/shape":
                names += ["train/n_u", "train/n_v"]
                row += [int(v[0]), int(v[1])]
            elif name == "k":
                names.append(name)
                row.append(int(v))
            else:
                names.append(name)
                row.append(float(v))
        rows.append(row)
    return {"columns": names, "rows": rows}


def run_case(PyBMF, X, tau, k, tol, w_fp=0.5, w_fn=None, X_val=None, X_test=None, keep_sweeps=False, may_raise=()):
    from PyBMF.models import Asso
    from PyBMF.utils import binarize
    mod = sys.modules["PyBMF.models.Asso"]   # the module, not the class of the same name
    sweeps = []                               # one per factor attempt: dict(s_old, X_old, scores, vectors)
    get_vector = mod.get_vector

    def logged(X_gt, X_old, s_old, basis, basis_dim, w_fp, w_fn):
        if not sweeps or sweeps[-1]["s_old"] is not s_old:
            sweeps.append(dict(s_old=s_old, X_old=dense_u8(X_old), scores=[], vectors=[]))
        score, vector = get_vector(X_gt=X_gt, X_old=X_old, s_old=s_old, basis=basis, basis_dim=basis_dim, w_fp=w_fp, w_fn=w_fn)
        sweeps[-1]["scores"].append(float(score))
        sweeps[-1]["vectors"].append(dense_u8(vector).ravel())
        return score, vector
    mod.get_vector = logged
    show = Asso.show_matrix
    Asso.show_matrix = lambda self, *a, **kw: None    # init_model plots unconditionally
    raised = None
    t0 = time.time()
    try:
        with quiet():
            model = Asso(tau=tau, k=k, tol=tol, w_fp=w_fp, w_fn=w_fn)
            try:
                model.fit(csr_matrix(X.astype(np.float64)), None if X_val is None else csr_matrix(X_val.astype(np.float64)),
                          None if X_test is None else csr_matrix(X_test.astype(np.float64)), **FIT_KW)
            except may_raise as exc:
                raised = type(exc).__name__
    finally:
        mod.get_vector = get_vector
        Asso.show_matrix = show
    seconds = time.time() - t0
    full = dense_u8(binarize(model.assoc, tau))
    kept = np.nonzero(full.sum(axis=1) != 0)[0]
    log = flat_log(model.logs["updates"]) if "updates" in model.logs else {"columns": [], "rows": []}
    X_pd = getattr(model, "X_pd", None)
    X_pd = csr_matrix(X.shape) if X_pd is None else csr_matrix(X_pd)
    out = dict(X=X, U=dense_u8(model.U), V=dense_u8(model.V), X_pd=dense_u8(X_pd), basis=full, kept=kept.astype(np.int32),
               raised=raised, log=log, counts=counts_of(PyBMF, csr_matrix(X.astype(np.float64)), X_pd), seconds=seconds)
    # replay the list: which candidates each sweep saw, who won, and by what margin
    alive, best, margins, winners, points = list(kept), 0.0, [], [], []
    for j, s in enumerate(sweeps):
        sc = np.array(s["scores"])
        assert sc.size == len(alive)
        pos = int(np.argmax(sc)) if sc.size and sc.max() > best else -1
        others = np.delete(sc, pos) if pos >= 0 else sc
        top = sc[pos] if pos >= 0 else (sc.max() if sc.size else 0.0)
        gaps = [abs(top - best)] + ([float(np.abs(others - top).min())] if pos >= 0 and others.size else [])
        gaps = [g for g in gaps if g > 0 or pos < 0]     # an equal later score loses to the first of equals: no margin needed
        margins.append(min(gaps) / max(abs(top), 1.0) if gaps else 1.0)
        points.append(dict(index=j, best_score=best, list=np.array(alive, dtype=np.int32), X_pd=s["X_old"],
                           s_old=np.asarray(s["s_old"], dtype=np.float64).ravel(), scores=sc,
                           vectors=np.array(s["vectors"], dtype=np.uint8).reshape(len(alive), X.shape[0]), winner=pos))
        winners.append(int(alive[pos]) if pos >= 0 else -1)
        if pos >= 0:
            best = float(sc[pos])
            assert best == log["rows"][j][log["columns"].index("train/score")]
            del alive[pos]
    assert sum(w >= 0 for w in winners) == len(log["rows"])
    out.update(margins=margins, winners=winners, n_sweeps=len(sweeps))
    out["points"] = [points[i] for i in sorted({0, len(points) // 2})] if keep_sweeps and points else []
    return out


def main():
    PyBMF = load_reference()
    Xa = planted(96, 72, 4, 0.2, 0.03, 2401)
    Xb = planted(200, 150, 6, 0.2, 0.03, 2402)
    Xc = planted(40, 30, 4, 0.25, 0.02, 2403)
    tr, va, te = deal(Xa, 2404)
    err = (TypeError,)
    params = {"a": dict(tau=0.4, k=5, tol=0), "b": dict(tau=0.35, k=None, tol=0.11), "c": dict(tau=0.5, k=None, tol=0),
              "d": dict(tau=0.4, k=5, tol=0), "e": dict(tau=0.4, k=None, tol=0), "f": dict(tau=0.6, k=4, tol=0, w_fp=1.0, w_fn=1.0),
              "g": dict(tau=0.4, k=5, tol=0, w_fp=0.3, w_fn=None)}
    cases = {"a": run_case(PyBMF, Xa, keep_sweeps=True, **params["a"]),
             "b": run_case(PyBMF, Xb, keep_sweeps=True, may_raise=err, **params["b"]),
             "c": run_case(PyBMF, Xc, may_raise=err, **params["c"]),
             "d": run_case(PyBMF, tr, X_val=va, X_test=te, **params["d"]),
             "e": run_case(PyBMF, np.zeros((20, 15), dtype=np.uint8), may_raise=err, **params["e"]),
             "f": run_case(PyBMF, Xa, **params["f"])}
    for seed in range(2407, 2427):           # the first seed whose every sweep is decided by more than rounding
        g = run_case(PyBMF, planted(96, 72, 4, 0.2, 0.03, seed), **params["g"])
        if min(g["margins"]) > MARGIN:
            cases["g"] = g
            params["g"]["seed"] = seed
            break
    assert "g" in cases and all(m > MARGIN for m in cases["g"]["margins"])
    cases["d"]["X_val"], cases["d"]["X_test"] = va, te
    arrays, meta = {}, {"cases": {}}
    for name, c in cases.items():
        for key in ("X", "U", "V", "X_pd", "X_val", "X_test", "basis", "kept"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        for i, p in enumerate(c["points"]):
            for key in ("list", "s_old", "scores"):
                arrays[f"{name}_p{i}_{key}"] = p[key]
            for key in ("X_pd", "vectors"):
                arrays[f"{name}_p{i}_{key}"] = np.packbits(p[key], axis=1, bitorder="little")
        n_factors = max(len(c["log"]["rows"]), 1)
        meta["cases"][name] = dict(params[name], shape=list(c["X"].shape), log=c["log"], counts=c["counts"], raised=c["raised"],
                                   n_sweeps=c["n_sweeps"], winners=c["winners"], margins=c["margins"],
                                   seconds_per_factor=c["seconds"] / n_factors,
                                   points=[{"index": p["index"], "best_score": p["best_score"], "winner": p["winner"]} for p in c["points"]])
        print(name, "rows:", len(c["log"]["rows"]), "U:", c["U"].shape, "sweeps:", c["n_sweeps"], "winners:", c["winners"],
              "counts:", c["counts"], "ones:", int(c["X"].sum()), "raised:", c["raised"], "min margin: %.3g" % min(c["margins"] or [1.0]),
              "s/factor: %.2f" % (c["seconds"] / n_factors))
    np.savez_compressed(os.path.join(HERE, "g24_asso.npz"), **arrays)
    with open(os.path.join(HERE, "g24_asso.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
