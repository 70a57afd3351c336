#!/usr/bin/env python3
"""Generate g29_grecondplus.{npz,json} by running the *reference* GreConDPlus (PyBMF @ 2024_10_08).

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_grecondplus.py          (about a minute, nearly all of it case b)

(i) Full fits.  Where the reference ends in its own TypeError ("No pattern found": early_stop calls _early_stop without `verbose`) the
log rows and the factors so far are kept.
  a  96 x 72, 4 planted factors, 3 % flips, k = 5, defaults (w_fp = 0.5, w_fn = None)
  b  the same X, k = None, w_fp = 0.3: dozens of factors, long expansions, remove_covered() at work, then the TypeError
  c  33 x 65, 3 planted factors (density 0.3, 3 % flips, seed 9), k = 6, w_fn = 1.0
  d  40 x 30, noise-free product of 4 factors, k = None: exact data, ends at score 0 (TypeError)
  e  20 x 15 of zeros, k = 3: no log row, the TypeError at once
  f  case a's X, k = 6, w_fp = 0.9
  g  case a's ones dealt to train / val / test (70 / 15 / 15 %), k = 5, defaults
  h  a planted matrix found by the seed search below, k = 4, defaults: holds an expansion that stops on r_score == c_score > 0 if
     cases a - g hold none
For each: the matrices (uint8), every row of logs['updates'] without `time` (k, score, |u|, |v| of the factor as set, then the four
metrics per data set), the final U, V, U_exp, V_exp, the integer TP / FP / FN / TN of the final X_pd against X_train, the exception's
name, and the whole expansion trace: one row (call, axis, index, r_score, c_score) per step of every expansion() call, read by wrapping
_expansion; axis 1 = a row joined, 0 = a column, -1 = the stop.  The script asserts that the traces hold a stop on
r_score == c_score > 0 and a stop with both scores <= 0, and records where.

(ii) remove_covered() and remove_overlapped() on states set by hand on a model object (X_train, U, V, U_exp, V_exp, m, n): the state
before and after each call.  In 14 natural fits remove_overlapped() never removed anything, so its paths are reached this way:
  row        a row of an extension is removed
  column     a column of an extension is removed
  stale      factor 0 loses row 2, and its column 2 is then tested over the rows taken BEFORE the row loop: row 2 is still read, with its
             count already decremented to 1, so the column stays; with the rows as they are after the row loop it would leave
  twice      factor 0 loses row 2 and then column 2, whose removal decrements cell (2, 2) a second time: factor 1's extension row 2
             then reads 1 where two factors still cover the cell, and stays; with freshly counted coverage it would leave
  single     the subset test passes (the row of X holds v) but the cells are covered once: nothing is removed
  nothing    no extension at all
  hole       every cell under the extension row is covered twice but one is a zero of X: the subset test fails, nothing is removed
The script runs a restatement with freshly recomputed rows and coverage beside the reference on `stale` and `twice` and asserts that the
outcomes differ.

With the SciPy installed here the reference as shipped cannot finish a removal: `coverage` is a csr matrix and `coverage[i, j_idx] -= 1`
raises NotImplementedError (a nonzero scalar subtracted from a sparse matrix), which is why no natural fit ever shows one.  For (ii) the
script therefore hands remove_overlapped() the same counts as a dense np.matrix (DenseCounts; the module's `matmul` wrapped for that call), so
that every line of it runs as written; `shipped_raises` records the states where the unwrapped call raises: exactly those with a removal.
"""
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import csr_matrix, lil_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402
from make_golden_grecond import deal, dense_u8, flat_log, planted  # noqa: E402


def run_case(PyBMF, X, params, X_val=None, X_test=None):
    from PyBMF.models import GreConDPlus
    mod = sys.modules["PyBMF.models.GreConDPlus"]   # the module, not the class of the same name
    expansion, _expansion = mod.expansion, mod._expansion
    calls, pending = [], []

    def logged_inner(X_gt, X_old, u, v, w_fp, w_fn, axis):
        score, index = _expansion(X_gt, X_old, u, v, w_fp, w_fn, axis)
        pending.append((axis, float(score), int(index)))
        return score, index

    def logged_outer(**kw):
        pending.clear()
        out = expansion(**kw)
        assert len(pending) % 2 == 0
        steps = []
        for (ax_r, r_score, r_index), (ax_c, c_score, c_index) in zip(pending[0::2], pending[1::2]):
            assert (ax_r, ax_c) == (1, 0)
            axis = 1 if (r_score > c_score and r_score > 0) else (0 if (c_score > r_score and c_score > 0) else -1)
            steps.append((axis, r_index if axis == 1 else (c_index if axis == 0 else -1), r_score, c_score))
        assert steps[-1][0] == -1 and all(s[0] >= 0 for s in steps[:-1])
        assert sum(s[0] == 1 for s in steps) == int(out[0].sum()) and sum(s[0] == 0 for s in steps) == int(out[1].sum())
        calls.append(steps)
        return out

    def sp(A):
        return None if A is None else csr_matrix(A.astype(np.float64))
    mod.expansion, mod._expansion = logged_outer, logged_inner
    raised, t0 = None, time.time()
    try:
        with quiet():
            model = GreConDPlus(**params)
            try:
                model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
            except TypeError as exc:
                raised = type(exc).__name__
    finally:
        mod.expansion, mod._expansion = expansion, _expansion
    seconds = time.time() - t0
    log = flat_log(model.logs["updates"]) if "updates" in getattr(model, "logs", {}) else {"columns": [], "rows": []}
    f = model.U.shape[1] if log["rows"] else 0       # before the first factor U still holds init_model's empty columns
    fe = model.U_exp.shape[1] if hasattr(model, "U_exp") else 0
    out = dict(X=X, U=dense_u8(csr_matrix(model.U))[:, :f], V=dense_u8(csr_matrix(model.V))[:, :f],
               U_exp=dense_u8(csr_matrix(model.U_exp))[:, :fe] if fe else np.zeros((X.shape[0], 0), np.uint8),
               V_exp=dense_u8(csr_matrix(model.V_exp))[:, :fe] if fe else np.zeros((X.shape[1], 0), np.uint8),
               raised=raised, log=log, calls=calls, seconds=seconds)
    X_pd = csr_matrix(model.X_pd) if getattr(model, "X_pd", None) is not None else csr_matrix(X.shape)
    out["counts"] = counts_of(PyBMF, sp(X), X_pd)
    return out


def stops(calls):
    """(index of the first call that stops on r == c > 0, of the first that stops with both <= 0), -1 where there is none."""
    tie = [i for i, s in enumerate(calls) if s[-1][2] == s[-1][3] > 0]
    low = [i for i, s in enumerate(calls) if s[-1][2] <= 0 and s[-1][3] <= 0]
    return (tie[0] if tie else -1), (low[0] if low else -1)


# ---- constructed states ---------------------------------------------------------------------------------------------------------
def state(m, n, ones, factors):
    """X with `ones` (list of (rows, cols) rectangles); factors: [(rows, cols, ext rows, ext cols)]."""
    X = np.zeros((m, n), np.uint8)
    for rows, cols in ones:
        X[np.ix_(rows, cols)] = 1
    f = len(factors)
    U, V, Ue, Ve = np.zeros((m, f), np.uint8), np.zeros((n, f), np.uint8), np.zeros((m, f), np.uint8), np.zeros((n, f), np.uint8)
    for k, (rows, cols, er, ec) in enumerate(factors):
        U[rows, k], V[cols, k], Ue[er, k], Ve[ec, k] = 1, 1, 1, 1
        assert set(er) <= set(rows) and set(ec) <= set(cols)
    return X, U, V, Ue, Ve


class DenseCounts(np.matrix):
    """U @ V.T as a dense matrix that slices like the sparse one (a row stays 2-d) and takes `coverage[rows, j] -= 1`."""

    def __setitem__(self, key, value):
        np.ndarray.__setitem__(self, key, np.asarray(value).reshape(np.asarray(self)[key].shape))


def reference_model(X, U, V, Ue, Ve):
    from PyBMF.models import GreConDPlus
    model = GreConDPlus.__new__(GreConDPlus)
    model.X_train = csr_matrix(X.astype(np.float64))
    model.U, model.V = lil_matrix(U.astype(np.float64)), lil_matrix(V.astype(np.float64))
    model.U_exp, model.V_exp = lil_matrix(Ue.astype(np.float64)), lil_matrix(Ve.astype(np.float64))
    model.m, model.n = X.shape
    return model


def read_model(model):
    return tuple(dense_u8(csr_matrix(A)) for A in (model.U, model.V, model.U_exp, model.V_exp))


def fresh_overlapped(X, U, V, Ue, Ve):
    """remove_overlapped() as it would be with the rows, columns and coverage taken anew before every test: NOT what the reference does."""
    U, V, Ue, Ve = (A.astype(np.int64).copy() for A in (U, V, Ue, Ve))
    for k in range(U.shape[1]):
        for i in np.nonzero(Ue[:, k])[0]:
            cov, j_idx = U @ V.T, np.nonzero(V[:, k])[0]
            if (cov[i, j_idx] * X[i, j_idx]).min() >= 2:
                U[i, k] = Ue[i, k] = 0
        for j in np.nonzero(Ve[:, k])[0]:
            cov, i_idx = U @ V.T, np.nonzero(U[:, k])[0]
            if (cov[i_idx, j] * X[i_idx, j]).min() >= 2:
                V[j, k] = Ve[j, k] = 0
    return tuple(A.astype(np.uint8) for A in (U, V, Ue, Ve))


def constructed_states():
    R = range
    full = [(list(R(6)), list(R(6)))]
    out = {}
    # factor 0 = rows 0-2 x cols 0-2 with extension row 2; factor 1 covers row 2 x cols 0-2 as well
    out["row"] = state(6, 6, full, [([0, 1, 2], [0, 1, 2], [2], []), ([2, 3], [0, 1, 2], [], [])])
    out["column"] = state(6, 6, full, [([0, 1, 2], [0, 1, 2], [], [2]), ([0, 1, 2], [2, 3], [], [])])
    out["stale"] = state(6, 6, full, [([0, 1, 2], [0, 1, 2], [2], [2]), ([2, 3], [0, 1, 2], [], []), ([0, 1], [2, 3], [], [])])
    out["twice"] = state(6, 6, full, [([0, 1, 2], [0, 1, 2], [2], [2]), ([2, 3], [2], [2], []), ([0, 1, 2], [0, 1, 2], [], [])])
    out["single"] = state(6, 6, full, [([0, 1, 2], [0, 1, 2], [2], [2]), ([4, 5], [4, 5], [], [])])
    out["nothing"] = state(6, 6, [(list(R(4)), list(R(4)))], [([0, 1], [0, 1], [], []), ([2, 3], [1, 2, 3], [], [])])
    # a zero of X under the extension row: the subset test fails although every cell is covered twice
    X, U, V, Ue, Ve = state(6, 6, full, [([0, 1, 2], [0, 1, 2], [2], []), ([2, 3], [0, 1, 2], [], [])])
    X[2, 1] = 0
    out["hole"] = (X, U, V, Ue, Ve)
    return out


def covered_states():
    """(U, V, U_exp, V_exp, k): factor k against the others."""
    m, n = 8, 7
    _, U, V, Ue, Ve = state(m, n, [], [([0, 1], [0, 1], [], []), ([0, 1, 2, 3], [0, 1, 2], [3], [2]), ([2, 3], [1, 2], [], []),
                                       ([0, 1, 2, 3], [0, 1, 2, 3], [], [3]), ([4, 5], [0, 1], [5], []), ([0, 1, 2, 3], [0, 1, 2], [], [])])
    return {"inside": (U, V, Ue, Ve, 1),          # 0, 2 and the equal factor 5 lie inside 1; 3 and 4 do not
            "all_but_one": (U, V, Ue, Ve, 3),     # 0, 1, 2, 5 lie inside 3
            "none": (U, V, Ue, Ve, 4),
            "rows_only": (U, V, Ue, Ve, 0)}       # nothing lies inside the smallest


def main():
    PyBMF = load_reference()
    Xa = planted(96, 72, 4, 0.2, 0.03, 2301)
    Xc = planted(33, 65, 3, 0.3, 0.03, 9)
    Xd = planted(40, 30, 4, 0.25, 0.0, 2303)
    tr, va, te = deal(Xa, 2304)

    def P(k, w_fp=0.5, w_fn=None):
        return dict(k=k, tol=0, w_fp=w_fp, w_fn=w_fn)
    params = {"a": P(5), "b": P(None, w_fp=0.3), "c": P(6, w_fn=1.0), "d": P(None), "e": P(3), "f": P(6, w_fp=0.9), "g": P(5)}
    data = {"a": Xa, "b": Xa, "c": Xc, "d": Xd, "e": np.zeros((20, 15), dtype=np.uint8), "f": Xa, "g": tr}
    cases = {}
    for name in params:
        extra = dict(X_val=va, X_test=te) if name == "g" else {}
        cases[name] = run_case(PyBMF, data[name], params[name], **extra)
        cases[name].update(extra)
    found = {name: stops(c["calls"]) for name, c in cases.items()}
    if not any(t >= 0 for t, _ in found.values()):
        for seed in range(3000, 3400):        # the search: the first planted 48 x 40 whose fit holds a stop on equal positive scores
            Xh = planted(48, 40, 3, 0.3, 0.05, seed)
            c = run_case(PyBMF, Xh, P(4))
            if stops(c["calls"])[0] >= 0:
                params["h"], data["h"], cases["h"] = dict(P(4), seed=seed), Xh, c
                found["h"] = stops(c["calls"])
                break
    assert any(t >= 0 for t, _ in found.values()), "no expansion stops on r_score == c_score > 0"
    assert any(l >= 0 for _, l in found.values()), "no expansion stops with both scores <= 0"
    arrays, meta = {}, {"cases": {}, "overlapped": {}, "covered": {}}
    for name, c in cases.items():
        for key in ("X", "U", "V", "U_exp", "V_exp", "X_val", "X_test"):
            if key in c:
                arrays[f"{name}_{key}"] = c[key]
        rows = [[i, s[0], s[1], s[2], s[3]] for i, steps in enumerate(c["calls"]) for s in steps]
        arrays[f"{name}_trace"] = np.array(rows, dtype=np.float64).reshape(len(rows), 5)
        meta["cases"][name] = dict(params[name], shape=list(c["X"].shape), log=c["log"], counts=c["counts"], raised=c["raised"],
                                   n_calls=len(c["calls"]), stop_on_tie=found[name][0], stop_on_low=found[name][1])
        n_rows = len(c["log"]["rows"])
        print(name, "rows:", n_rows, "factors:", c["U"].shape[1], "extension columns:", c["U_exp"].shape[1], "counts:", c["counts"],
              "raised:", c["raised"], "steps:", [len(s) for s in c["calls"]][:12], "tie / low stop at call:", found[name],
              "k:", [r[0] for r in c["log"]["rows"]][:12], "seconds per log row: {:.3f}".format(c["seconds"] / max(1, n_rows)))
    for name, (X, U, V, Ue, Ve) in constructed_states().items():
        shipped = None
        try:
            with quiet():
                reference_model(X, U, V, Ue, Ve).remove_overlapped()
        except NotImplementedError as exc:
            shipped = type(exc).__name__
        model = reference_model(X, U, V, Ue, Ve)
        mod = sys.modules["PyBMF.models.GreConDPlus"]
        matmul = mod.matmul
        mod.matmul = lambda *a, **kw: matmul(*a, **kw).toarray().view(DenseCounts)   # the same counts in a container that takes `-= 1`
        try:
            with quiet():
                model.remove_overlapped()
        finally:
            mod.matmul = matmul
        after = read_model(model)
        assert (shipped is not None) == (after[2].sum() < Ue.sum() or after[3].sum() < Ve.sum()), name
        fresh = fresh_overlapped(X, U, V, Ue, Ve)
        differs = any((a != b).any() for a, b in zip(after, fresh))
        if name in ("stale", "twice"):
            assert differs, name
            assert after[2].sum() < Ue.sum(), name          # a row did leave
        if name == "twice":
            assert after[3].sum() < Ve.sum()                # and a column
        if name == "row":
            assert after[2].sum() == Ue.sum() - 1 and (after[1] == V).all()
        if name == "column":
            assert after[3].sum() == Ve.sum() - 1 and (after[0] == U).all()
        if name in ("single", "nothing", "hole"):
            assert all((a == b).all() for a, b in zip(after, (U, V, Ue, Ve))), name
        for key, A in zip(("X", "U0", "V0", "Ue0", "Ve0", "U1", "V1", "Ue1", "Ve1"), (X, U, V, Ue, Ve) + after):
            arrays[f"o_{name}_{key}"] = A
        meta["overlapped"][name] = dict(differs_from_fresh=bool(differs), shipped_raises=shipped, rows_removed=int(Ue.sum() - after[2].sum()),
                                        columns_removed=int(Ve.sum() - after[3].sum()))
        print("overlapped", name, meta["overlapped"][name])
    for name, (U, V, Ue, Ve, k) in covered_states().items():
        model = reference_model(np.zeros((U.shape[0], V.shape[0]), np.uint8), U, V, Ue, Ve)
        with quiet():
            model.remove_covered(k)
        after = read_model(model)
        for key, A in zip(("U0", "V0", "Ue0", "Ve0", "U1", "V1", "Ue1", "Ve1"), (U, V, Ue, Ve) + after):
            arrays[f"c_{name}_{key}"] = A
        meta["covered"][name] = dict(k=k, kept=int(after[0].shape[1]))
        print("covered", name, meta["covered"][name])
    np.savez_compressed(os.path.join(HERE, "g29_grecondplus.npz"), **arrays)
    with open(os.path.join(HERE, "g29_grecondplus.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
