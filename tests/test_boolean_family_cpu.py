"""The four bit-set models on the edge-case family of tests/boolean_family.py, without a GPU: every model x case x parameter set of the
grids through the NumPy stand-in engines.

  * the properties that define a correct result, checked without the stand-in (helpers of boolean_family): GreConD's factors are closed
    rectangles of ones whose scores are the drops of the residual, with no false positive; Asso's logged TP / FP are a dense recount of
    its factors and its score is w_fn TP - w_fp FP; AssoIter's error falls strictly over the logged visits and the fit ends with k
    fruitless ones; AssoOpt's j is the brute-force argmax per row;
  * the degenerate matrices (zeros, ones, one_cell, row, col) against factors and counts written out by hand;
  * the stand-ins against what the reference produced on this family (tests/golden/g26_boolean_family.*, written by
    tests/golden/make_golden_family.py), by the rules of check_fit / check_iter / check_opt: integers equal, the score equal (==) for
    weights whose products are exact and within 1e-12 relative otherwise.  A case on which the reference raised is not compared (the
    fixture names what it raised): it has the property tests only.
"""
import json
import os

import numpy as np
import pytest

import boolean_family as F
import test_asso_cpu as A
import test_asso_refine_cpu as R
import test_grecond_cpu as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- B1: properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CASES)
def test_grecond_properties(name):
    X = F.family()[name]["X"]
    by_k = {}
    for p in F.grecond_grid(name):
        snap = F.snapshot(F.fit_grecond(name, **p), "GreConD")
        F.grecond_invariants(X, snap["rows"], *snap["factors"], snap["counts"]["train"], snap["residual_sum"], snap["X_pd"])
        if p["k"] is None:       # runs until X is reconstructed
            assert (snap["X_pd"] == (X != 0)).all() and snap["residual_sum"] == 0
        else:
            assert len(snap["rows"]) <= p["k"]
        if p["k"] in by_k:       # the block size is a speed knob only
            F.assert_same_fit(snap, by_k[p["k"]], True)
        by_k.setdefault(p["k"], snap)
    assert len(by_k) == len({p["k"] for p in F.grecond_grid(name)}) and len(F.grecond_grid(name)) >= 2 * len(by_k)


@pytest.mark.parametrize("name", F.CASES)
def test_asso_properties(name):
    c = F.family()[name]
    first = {}
    for p in F.asso_grid(name):
        snap = F.snapshot(F.fit_asso(name, **p), "Asso")
        F.asso_invariants(c["X"], snap, p["w_fp"], p["w_fn"])
        assert len(snap["rows"]) <= c["k"]
        if p["tau"] == 1.0:
            assert snap["rows"] == [] and snap["list"] == [] and not snap["X_pd"].any()
        key = (p["tau"], p["w_fp"], p["w_fn"])
        if key in first:
            F.assert_same_fit(snap, first[key], True)
        first.setdefault(key, snap)
    assert len(first) < len(F.asso_grid(name))


@pytest.mark.parametrize("name", F.CASES)
def test_refiner_properties(name):
    X = F.family()[name]["X"]
    changed = 0
    for p in F.refine_grid(name):
        U0, V = F.refine_start(name, p["flipped"])
        it = F.snapshot(F.fit_refine(name, "AssoIter", **p), "AssoIter")
        F.iter_invariants(X, it, U0, V)
        opt = F.snapshot(F.fit_refine(name, "AssoOpt", **p), "AssoOpt")
        F.opt_invariants(X, opt, V, p["w_fp"], p["w_fn"])
        changed += int((it["U"] != (U0 != 0)).sum()) + int((opt["U"] != (U0 != 0)).sum())
    assert changed > 0           # no case passes by handing every U back
    if name not in F.DEGENERATE:
        assert (F.refine_start(name, True)[0] != F.refine_start(name, False)[0]).any()


# ---- B1: the degenerate matrices by hand --------------------------------------------------------------------------------------
def hand(name):
    """(X, u, v) of the one factor that reconstructs a degenerate matrix; u, v None for zeros."""
    X = F.family()[name]["X"] != 0
    if name == "zeros":
        return X, None, None
    return X, X.any(axis=1), X.any(axis=0)


def test_the_degenerate_matrices_are_what_the_hand_written_results_assume():
    fam = F.family()
    assert [fam[n]["shape"] for n in F.DEGENERATE] == [[12, 9], [12, 9], [1, 1], [1, 70], [70, 1]]
    assert not fam["zeros"]["X"].any() and fam["ones"]["X"].all() and fam["one_cell"]["X"].all()
    for name in ("row", "col"):
        x = fam[name]["X"].ravel()
        assert x[0] == 0 and x[1] == 1 and 35 < x.sum() < 70          # more ones than zeros, the first cell empty


@pytest.mark.parametrize("name", F.DEGENERATE)
@pytest.mark.parametrize("k", [None, 3])
def test_grecond_on_a_degenerate_matrix(name, k):
    X, u, v = hand(name)
    m, n = X.shape
    for block in (None, 1, 7):
        snap = F.snapshot(F.fit_grecond(name, k, block), "GreConD")
        assert snap["U"].shape == (m, 0) and snap["V"].shape == (n, 0)      # zeros: nothing found; else the tolerance stop (error 0) drops the factor
        if u is None:
            assert snap["rows"] == [] and snap["counts"]["train"] == (0, 0, 0, m * n) and not snap["X_pd"].any()
            assert snap["factors"][0].shape == (m, 0)
            continue
        s = int(X.sum())
        assert len(snap["rows"]) == 1 and snap["rows"][0][:6] == [0, s, int(u.sum()), int(v.sum()), 1.0, 1.0]
        assert snap["factors"][0][:, 0].tolist() == u.tolist() and snap["factors"][1][:, 0].tolist() == v.tolist()
        assert (snap["X_pd"] == X).all() and snap["counts"]["train"] == (s, 0, 0, m * n - s) and snap["residual_sum"] == 0


@pytest.mark.parametrize("name", F.DEGENERATE)
@pytest.mark.parametrize("w_fp,w_fn", F.WEIGHTS)
def test_asso_on_a_degenerate_matrix(name, w_fp, w_fn):
    """One candidate reconstructs the matrix (on `ones` nine equal candidates: the first wins); every row with a one takes it, a row
    without one does not (its score would fall, or with w_fp = 0 stay: strict >).  Error 0 then fires the tolerance stop, which drops the
    factor from U, V and from the prediction, as in the reference; the log row keeps what was counted before."""
    X, u, v = hand(name)
    m, n = X.shape
    s = int(X.sum())
    for tau in (0.3, 0.5):
        snap = F.snapshot(F.fit_asso(name, tau, w_fp, w_fn, None), "Asso")
        assert snap["U"].shape == (m, 0) and snap["V"].shape == (n, 0) and not snap["X_pd"].any()
        assert snap["counts"]["train"] == (0, 0, s, m * n - s)
        if u is None:
            assert snap["rows"] == [] and snap["history"] == [] and snap["list"] == []
            continue
        assert len(snap["rows"]) == 1
        r = snap["rows"][0]
        assert r[0] == 0 and r[1] == w_fn * s and r[2] == 0.5 * s and [r[4], r[5]] == [int(u.sum()), int(v.sum())]
        assert [r[6], r[8], r[10]] == [s, 0, 0] and r[3] == int(u.sum()) + int(v.sum())
        assert [e[0] for e in snap["history"]] == ["apply", "truncate"] and snap["history"][1][1] == 0
        assert snap["history"][0][1].tolist() == u.tolist() and snap["history"][0][2].tolist() == v.tolist()
        assert snap["list"] == np.nonzero(v)[0][1:].tolist()          # the winner was the first column with a one


@pytest.mark.parametrize("name", F.DEGENERATE)
def test_refiners_on_a_degenerate_matrix(name):
    """Asso keeps no factor on these, so the refiners start from one factor of all ones.  Under 0.5 / 0.5 a row holds it iff it has more
    ones than zeros, strictly."""
    X, _, _ = hand(name)
    m, n = X.shape
    U0, V = F.refine_start(name, False)
    assert U0.shape == (m, 1) and U0.all() and V.shape == (n, 1) and V.all()
    want = X.sum(axis=1) > n - X.sum(axis=1)
    assert want.tolist() == {"zeros": [False] * 12, "ones": [True] * 12, "one_cell": [True], "row": [True], "col": X[:, 0].tolist()}[name]
    err0, err1 = 1 - X.sum() / X.size, 1 - (want[:, None] == X).sum() / X.size
    it = F.snapshot(F.fit_refine(name, "AssoIter", False, 0.5, 0.5), "AssoIter")
    assert it["U"][:, 0].tolist() == want.tolist()
    if err1 < err0:      # zeros, col: the first visit is logged, the second is fruitless
        assert it["visits"] == [(0, err1, True), (0, err1, False)] and len(it["rows"]) == 1 and it["rows"][0][0] == 0
    else:                # the start was the answer already
        assert it["visits"] == [(0, err0, False)] and it["rows"] == []
    opt = F.snapshot(F.fit_refine(name, "AssoOpt", False, 0.5, 0.5), "AssoOpt")
    assert opt["chosen"] == want.astype(int).tolist() and opt["U"][:, 0].tolist() == want.tolist()
    tp = int((X & want[:, None]).sum())
    assert opt["counts"]["train"][:2] == (tp, int(want.sum()) * n - tp) and opt["rows"][0][0] == 0.5 * tp - 0.5 * (int(want.sum()) * n - tp)


# ---- B2: the stand-ins against the reference on this family -------------------------------------------------------------------
META = json.load(open(os.path.join(GOLDEN, "g26_boolean_family.json")))


def load(key):
    """A record of the fixture in the form that check_fit / check_iter / check_opt of the models' own CPU tests read."""
    z = np.load(os.path.join(GOLDEN, "g26_boolean_family.npz"))
    name = key.split("/")[1]
    c = dict(F.family()[name], **META["cases"][key])
    for a, shape in c.get("shapes", {}).items():
        arr = z[f"{key}/{a}"]
        c[a] = arr if a in ("kept", "j") else np.unpackbits(arr)[: int(np.prod(shape))].reshape(shape)
    return name, c


def keys_of(model, usable=True):
    return [k for k, r in META["cases"].items() if k.startswith(model + "/") and r["usable"] == usable]


def test_the_fixture_is_of_this_family_and_the_reference_completed_on_enough_of_it():
    assert META["guard"] == {n: [c["shape"], int(c["X"].sum())] for n, c in F.family().items()}
    for model in ("GreConD", "Asso", "AssoIter", "AssoOpt"):
        share = META["share"][model]
        assert share["of"] == len(F.CASES) and share["completed"] >= 0.75 * share["of"]
        assert sorted({k.split("/")[1] for k, r in META["cases"].items() if k.startswith(model + "/") and not r["completed"]}) == share["not_completed"]
        for key in keys_of(model, False):
            r = META["cases"][key]
            assert r["raised"] in ("TypeError", "IndexError") or (r["rounding"] and key.endswith("/skew"))
    assert len([k for k in keys_of("Asso") if k.endswith("/skew")]) >= 1          # inexact weights are pinned on this family too
    assert all(META["cases"][k]["raised"] == "AttributeError" for k in keys_of("AssoOpt"))
    assert sum(META["cases"][k]["cells_changed"] > 0 for k in keys_of("AssoIter") + keys_of("AssoOpt")) >= 30


@pytest.mark.parametrize("key", keys_of("GreConD"))
def test_grecond_stand_in_reproduces_the_reference(key):
    name, c = load(key)
    assert c["k"] == F.grecond_grid(name)[0]["k"]
    G.check_fit(F.fit_grecond(name, c["k"], None), c)


@pytest.mark.parametrize("key", keys_of("Asso"))
def test_asso_stand_in_reproduces_the_reference(key):
    name, c = load(key)
    assert c["k"] == F.family()[name]["k"] and c["raised"] is None
    A.check_fit(F.fit_asso(name, c["tau"], c["w_fp"], c["w_fn"], None), c, exact_score=F.exact_weights(c["w_fp"], c["w_fn"]))


@pytest.mark.parametrize("key", keys_of("AssoIter"))
def test_assoiter_stand_in_reproduces_the_reference(key):
    name, c = load(key)
    c["U_in"], c["V"] = F.refine_start(name, True)
    c["weights"] = (c["w_fp"], c["w_fn"])
    assert c["k"] == c["V"].shape[1]
    R.check_iter(F.fit_refine(name, "AssoIter", True, c["w_fp"], c["w_fn"]), c)


@pytest.mark.parametrize("key", keys_of("AssoOpt"))
def test_assoopt_stand_in_reproduces_the_reference(key):
    name, c = load(key)
    c["U_in"], c["V"] = F.refine_start(name, True)
    c["weights"] = (c["w_fp"], c["w_fn"])
    model = F.fit_refine(name, "AssoOpt", True, c["w_fp"], c["w_fn"])
    if c.get("X_val") is None:
        R.check_opt(model, c)
    else:                # check_opt names the log's columns for a fit without val / test data; the rest of it holds here too
        assert model.chosen.tolist() == c["j"].tolist() and c["raised"] == "AttributeError" and c["log"]["rows"] == []
        rows = model.logs["refinements"].values.tolist()
        tp, fp = c["counts"][:2]
        assert len(rows) == 1 and float(rows[0][1]) == -c["w_fp"] * np.float64(fp) + c["w_fn"] * np.float64(tp)
        assert [col[0] for col in model.logs["refinements"].columns][2:] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4
        R.check_common(model, c)
