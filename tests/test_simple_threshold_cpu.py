"""SimpleThreshold without a GPU: the facts the reference's notebooks recorded hold in the restatement (tests/thresh_grid_ref.py) and
in the model's host logic, the model run on a NumPy stand-in engine equals the restatement row by row, everything the model refuses
is refused with its reason, and the new entry points of the C ABI refuse bad arguments before anything touches a device."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import thresh_grid_ref as R

FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False, verbose=False)

# what examples/ex06_1_BinaryMFThreshold.ipynb of the reference stored of its run with n_grid=40 (its log, 0-based rows)
RECORDED = dict(n_grid=40, trials=1600, rows={125: dict(iter=126, u=0.299381, v=0.297139, cell=(3, 5)), 129: dict(u=0.299381, v=0.534851, cell=(3, 9))},
                columns=["time", "iter", "u", "v", "Recall", "Precision", "Accuracy", "F1"],
                printed=dict(W="full", n_trials=100, normalize_method=None, solver="grid-search", init_method="custom"))


class NumpyEngine:
    """pybmf_amd.thresh_grid.ThreshGridEngine in NumPy: same interface, counts formed per pair from the dense Boolean product."""

    def __init__(self, sets, U, V):
        self.sets = {name: np.asarray(X) != 0 for name, X in sets.items()}
        self.U, self.V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        self.sums = {name: int(X.sum()) for name, X in self.sets.items()}
        self.calls = []

    def _pair(self, tu, tv):
        P = R.product(self.U > tu[None, :], self.V > tv[None, :])
        return {name: (int((P & X).sum()), int((P & ~X).sum())) for name, X in self.sets.items()}

    def grid_counts(self, thr_u, thr_v):
        self.calls.append("grid")
        assert (np.diff(thr_u, axis=0) >= 0).all()
        out = {name: np.zeros((len(thr_u), len(thr_v), 2), np.int64) for name in self.sets}
        for a, tu in enumerate(thr_u):
            for b, tv in enumerate(thr_v):
                for name, c in self._pair(tu, tv).items():
                    out[name][a, b] = c
        return out

    def pair_counts(self, thr_u, thr_v, pairs):
        self.calls.append("pairs")
        out = {name: np.zeros((len(pairs), 2), np.int64) for name in self.sets}
        for t, (a, b) in enumerate(pairs):
            for name, c in self._pair(thr_u[a], thr_v[b]).items():
                out[name][t] = c
        return out


def dense(X):
    return None if X is None else np.asarray(X.todense() if hasattr(X, "todense") else X)


def fit_standin(X, U, V, X_val=None, X_test=None, **params):
    """The real class on a NumPy engine."""
    from pybmf_amd.models.SimpleThreshold import SimpleThreshold

    class Model(SimpleThreshold):
        def _make_engine(self):
            sets = {"train": dense(self._X_input)}
            sets.update({name: dense(Xs) for name, Xs in (("val", self.X_val), ("test", self.X_test)) if Xs is not None})
            return NumpyEngine(sets, self.U, self.V)

    with contextlib.redirect_stdout(io.StringIO()) as out:
        model = Model(U=U, V=V, **params)
        eng_box = []
        make = model._make_engine
        model._make_engine = lambda: eng_box.append(make()) or eng_box[0]
        model.fit(X, X_val, X_test, **FIT_KW)
    model._printed, model._engine_used = out.getvalue(), eng_box[0]
    return model


def planted_case(m, n, k, seed, noise=0.02, flips=0.03):
    """Planted 0 / 1 factors times uniform (0.3, 1) plus small noise, and the flipped product (the fixture of the issue)."""
    rng = np.random.RandomState(seed)
    Ub, Vb = rng.rand(m, k) < 0.25, rng.rand(n, k) < 0.25
    X = (R.product(Ub, Vb) ^ (rng.rand(m, n) < flips)).astype(np.uint8)
    U = Ub * rng.uniform(0.3, 1.0, size=(m, k)) + noise * rng.rand(m, k)
    V = Vb * rng.uniform(0.3, 1.0, size=(n, k)) + noise * rng.rand(n, k)
    return X, U, V


def check_against_ref(model, ref, columnwise=False):
    log = model.logs["updates"]
    assert len(log) == len(ref["thresholds"])
    keys = ("us", "vs") if columnwise else ("u", "v")
    assert list(log[("", "", "iter")]) == list(range(1, len(log) + 1))
    for t, (u, v) in enumerate(ref["thresholds"]):
        got_u, got_v = log[("", "", keys[0])][t], log[("", "", keys[1])][t]
        if columnwise:
            assert isinstance(got_u, tuple) and got_u == tuple(float(x) for x in u) and got_v == tuple(float(x) for x in v)
        else:
            assert isinstance(got_u, float) and got_u == float(u) and got_v == float(v)     # bit-equal
    for name, rows in ref["metrics"].items():
        got = np.array([[log[(name, 0, mt)][t] for mt in R.METRICS] for t in range(len(log))], dtype=np.float64)
        assert np.abs(got - np.array(rows)).max() <= 1e-12
    assert (model.counts_ == ref["counts"]["train"]).all() and model.counts_.dtype == np.int64
    assert model.best_iter == ref["best"] + 1
    bu, bv = ref["thresholds"][ref["best"]]
    if columnwise:
        assert model.us == tuple(float(x) for x in bu) and model.vs == tuple(float(x) for x in bv)
    else:
        assert (model.u, model.v) == (float(bu), float(bv)) and type(model.u) is float


# ---- the recorded facts -------------------------------------------------------------------------------------------------------
def test_recorded_facts_hold_in_the_restatement():
    # factors with minimum 0 and the maxima that the recorded equal-step values imply: u_3 = 3 max / 40, v_9 = 9 max / 40
    U = np.array([[0.0, 0.299381 / 3 * 40]])
    V = np.array([[0.0, 2.377115]])
    thr = R.trial_thresholds(U, V, n_grid=RECORDED["n_grid"])
    assert len(thr) == RECORDED["trials"]
    gu, gv = R.grid(U, 40), R.grid(V, 40)
    assert gu[0] == 0.0 and gv[0] == 0.0 and np.allclose(np.diff(gu), gu[1]) and np.allclose(np.diff(gv), gv[1])
    for row, want in RECORDED["rows"].items():
        a, b = want["cell"]
        assert row == a * 40 + b                                    # u-major
        assert thr[row][0] == gu[a] and thr[row][1] == gv[b]
        assert abs(thr[row][0] - want["u"]) < 1e-6 and abs(thr[row][1] - want["v"]) < 1e-6
    assert RECORDED["rows"][125]["iter"] == 125 + 1                 # iter is 1-based


def test_recorded_facts_hold_in_the_model():
    from pybmf_amd.models.SimpleThreshold import SimpleThreshold
    import pybmf_amd.models as M
    assert M.SimpleThreshold is SimpleThreshold
    rng = np.random.RandomState(5)
    U, V = rng.rand(6, 2), rng.rand(5, 2)
    U[0, 0] = V[0, 0] = 0.0
    U[1, 1], V[1, 1] = 0.299381 / 3 * 40, 2.377115
    X = (rng.rand(6, 5) < 0.4).astype(np.uint8)
    model = fit_standin(X, U, V, by_metric="F1", columnwise=False, randomize=False, n_grid=40, seed=2024)
    for name, value in RECORDED["printed"].items():
        assert getattr(model, name) == value, name
    assert model.k == 2 and model.n_grid == 40 and model.seed == 2024
    assert "grid search with 1600 trials in total" in model._printed
    log = model.logs["updates"]
    assert len(log) == 1600
    assert [c[0] if c[0] else c[-1] for c in log.columns][:4] == ["time", "iter", "u", "v"]
    assert [(c[0], c[2]) for c in log.columns][4:] == [("train", mt) for mt in RECORDED["columns"][4:]]
    assert log[("", "", "iter")][125] == 126 and log[("", "", "iter")][0] == 1
    assert abs(log[("", "", "u")][125] - 0.299381) < 1e-6 and abs(log[("", "", "v")][125] - 0.297139) < 1e-6
    assert abs(log[("", "", "u")][129] - 0.299381) < 1e-6 and abs(log[("", "", "v")][129] - 0.534851) < 1e-6
    assert model._engine_used.calls == ["grid"] and model._engine is None
    # the defaults of n_grid: 40 for the exhaustive grid, 10 for the randomised search
    with contextlib.redirect_stdout(io.StringIO()):
        assert SimpleThreshold(U=U, V=V).n_grid == 40 and SimpleThreshold(U=U, V=V, randomize=True).n_grid == 10
        d = SimpleThreshold(U=U, V=V)
    assert (d.W, d.by_metric, d.columnwise, d.randomize, d.n_trials, d.normalize_method) == ("full", "F1", False, False, 100, None)


# ---- the grid -------------------------------------------------------------------------------------------------------------------
def test_grid_definition():
    from pybmf_amd.models.SimpleThreshold import threshold_grid
    rng = np.random.RandomState(7)
    F = rng.rand(9, 3) * 2 - 0.5
    F[:, 1] = 0.75                                                    # a constant column
    for n_grid in (1, 7, 40):
        g = threshold_grid(F, n_grid)
        assert g.shape == (n_grid,) and g[0] == F.min() and g.max() < F.max() and (g == np.linspace(F.min(), F.max(), n_grid, endpoint=False)).all()
        assert (g == R.grid(F, n_grid)).all()
        gc = threshold_grid(F, n_grid, columnwise=True)
        assert gc.shape == (n_grid, 3) and (gc == R.grid(F, n_grid, True)).all()
        assert (gc[:, 1] == 0.75).all()                               # a constant column: every threshold equals its value
        assert (gc[0] == F.min(axis=0)).all()
        for c in (0, 2):
            assert (gc[:, c] == np.linspace(F[:, c].min(), F[:, c].max(), n_grid, endpoint=False)).all()
    # the first grid point IS the minimum, so F > g[0] drops the minimal entries (strict) and F > max would be empty
    assert not (F > threshold_grid(F, 5)[0]).all() and (F > threshold_grid(F, 5)[-1]).any()


def test_all_zero_factor():
    rng = np.random.RandomState(8)
    X = (rng.rand(7, 6) < 0.5).astype(np.uint8)
    U, V = np.zeros((7, 3)), rng.rand(6, 3)
    model = fit_standin(X, U, V, n_grid=4)
    assert (model.counts_ == 0).all()
    log = model.logs["updates"]
    for mt in ("Recall", "Precision", "F1"):                          # (Accuracy is the share of zeros of X: nothing is predicted)
        assert (np.array(log[("train", 0, mt)], dtype=float) == 0).all()
    assert np.allclose(np.array(log[("train", 0, "Accuracy")], dtype=float), 1 - X.mean())
    assert model.best_iter == 1 and (model.u, model.v) == (0.0, float(V.min()))
    ref = R.search(X, U, V, n_grid=4)
    assert ref["best"] == 0
    check_against_ref(model, ref)


def test_strictly_greater_tie_rule():
    from pybmf_amd.models.SimpleThreshold import best_trial
    assert best_trial([0.1, 0.5, 0.5, 0.3, 0.5]) == 1 and R.best_of([0.1, 0.5, 0.5, 0.3, 0.5]) == 1
    assert best_trial([0, 0, 0]) == 0 and best_trial([0.2, 0.1, 0.7, 0.7]) == 2 and best_trial([0.3]) == 0
    # a plateau in a fit: U takes two values, so every u of the grid below the larger one gives the same bits
    X = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=np.uint8)
    U, V = np.array([[1.0], [1.0], [0.0]]), np.array([[1.0], [1.0], [0.0]])
    model = fit_standin(X, U, V, n_grid=4)
    f1 = np.array(model.logs["updates"][("train", 0, "F1")], dtype=float)
    assert (f1 == 1.0).all()                                          # every trial reconstructs X: sixteen equal values
    assert model.best_iter == 1 and (model.u, model.v) == (0.0, 0.0)


def test_draws_under_a_seed():
    X, U, V = planted_case(12, 9, 3, 31)
    a = fit_standin(X, U, V, randomize=True, n_trials=20, seed=7)
    b = fit_standin(X, U, V, randomize=True, n_trials=20, seed=7)
    c = fit_standin(X, U, V, randomize=True, n_trials=20, seed=8)
    assert a.n_grid == 10 and "randomized grid search with 20 trials" in a._printed and a._engine_used.calls == ["pairs"]
    ua, ub, uc = (list(zip(m_.logs["updates"][("", "", "u")], m_.logs["updates"][("", "", "v")])) for m_ in (a, b, c))
    assert ua == ub and ua != uc
    idx = np.random.RandomState(7).randint(0, 10, size=(20, 2))
    gu, gv = R.grid(U, 10), R.grid(V, 10)
    assert ua == [(float(gu[i]), float(gv[j])) for i, j in idx]
    # columnwise: one index per column and side, [t, 0, c] into column c's grid of U
    d = fit_standin(X, U, V, randomize=True, columnwise=True, n_trials=6, seed=7)
    idx = np.random.RandomState(7).randint(0, 10, size=(6, 2, 3))
    gu, gv = R.grid(U, 10, True), R.grid(V, 10, True)
    log = d.logs["updates"]
    for t in range(6):
        assert log[("", "", "us")][t] == tuple(float(gu[idx[t, 0, c], c]) for c in range(3))
        assert log[("", "", "vs")][t] == tuple(float(gv[idx[t, 1, c], c]) for c in range(3))


# ---- the model against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_metric", ["F1", "Recall", "Precision", "Accuracy"])
def test_model_equals_restatement_exhaustive(by_metric):
    X, U, V = planted_case(20, 14, 4, 41)
    model = fit_standin(X, U, V, by_metric=by_metric, n_grid=9)
    check_against_ref(model, R.search(X, U, V, by_metric=by_metric, n_grid=9))


def test_model_equals_restatement_with_extra_sets_and_draws():
    X, U, V = planted_case(20, 14, 4, 42)
    rng = np.random.RandomState(43)
    Xv, Xt = (rng.rand(20, 14) < 0.3).astype(np.uint8), (rng.rand(20, 14) < 0.1).astype(np.uint8)
    extra = {"val": Xv, "test": Xt}
    model = fit_standin(csr_matrix(X), U, V, csr_matrix(Xv), csr_matrix(Xt), n_grid=6)
    assert [c[0] for c in model.logs["updates"].columns if c[0]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4
    check_against_ref(model, R.search(X, U, V, extra=extra, n_grid=6))
    model = fit_standin(X, U, V, csr_matrix(Xv), None, randomize=True, n_trials=30, seed=3)
    check_against_ref(model, R.search(X, U, V, extra={"val": Xv}, randomize=True, n_trials=30, seed=3))
    model = fit_standin(X, U, V, randomize=True, columnwise=True, n_trials=30, n_grid=5, seed=4)
    check_against_ref(model, R.search(X, U, V, randomize=True, columnwise=True, n_trials=30, n_grid=5, seed=4), columnwise=True)
    assert model.evaluate is not None and model._score("train", ["TP", "FP"]) == list(model.counts_[model.best_iter - 1])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from pybmf_amd.models.SimpleThreshold import SimpleThreshold
    X, U, V = planted_case(10, 8, 2, 51)
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        with pytest.raises(NotImplementedError, match="task='reconstruction'"):
            SimpleThreshold(U=U, V=V).fit(X, task="prediction")
        with pytest.raises(NotImplementedError, match=r"Boolean \(0/1\)"):
            SimpleThreshold(U=U, V=V).fit(X.astype(np.float64) * 0.5, **FIT_KW)
        with pytest.raises(NotImplementedError, match=r"Boolean \(0/1\)"):
            SimpleThreshold(U=U, V=V).fit(X, X_val=csr_matrix(X * 3), **FIT_KW)
        with pytest.raises(NotImplementedError, match="k=129.*k <= 128"):
            SimpleThreshold(U=np.ones((10, 129)), V=np.ones((8, 129)))
        with pytest.raises(NotImplementedError, match=r"n_grid\^\(2k\) = 40\^4 trials"):
            SimpleThreshold(U=U, V=V, columnwise=True).fit(X, **FIT_KW)
        with pytest.raises(AssertionError, match="by_metric"):
            SimpleThreshold(U=U, V=V, by_metric="RMSE")
        import torch.distributed as dist
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        with pytest.raises(NotImplementedError, match="one GPU"):
            SimpleThreshold(U=U, V=V).fit(X, **FIT_KW)


# ---- the entry points of the C ABI refuse bad arguments without a GPU ---------------------------------------------------------------
def panels(lib, **over):
    p = C.c_void_p(4096)
    a = dict(F64=p, rows_pad=128, rows=100, k=5, kp=32, thr=p, T=3, rowbits=p, colbits=p, ldcb=4)
    a.update(over)
    return lib.bmf_thresh_panels(a["F64"], a["rows_pad"], a["rows"], a["k"], a["kp"], a["thr"], a["T"], a["rowbits"], a["colbits"], a["ldcb"], None)


def cover(lib, pair_list=False, **over):
    p = C.c_void_p(4096)
    a = dict(X=p, rows_pad=128, ldx=8, words=8, rb0=p, rb1=None, A=3, cb0=p, cb1=None, ldcb=8, kp=32, B=5, pairs=p, T=4, counts=p)
    a.update(over)
    head = (a["X"], a["rows_pad"], a["ldx"], a["words"], a["rb0"], a["rb1"], a["A"], a["cb0"], a["cb1"], a["ldcb"], a["kp"], a["B"])
    if pair_list:
        return lib.bmf_pairs_cover_count(*head, a["pairs"], a["T"], a["counts"], None)
    return lib.bmf_grid_cover_count(*head, a["counts"], None)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    for name in ("F64", "thr"):
        assert panels(lib, **{name: None}) == -1 and b"bmf_thresh_panels: null pointer" in lib.bmf_last_error(), name
    assert panels(lib, rowbits=None, colbits=None) == -1 and b"null pointer" in lib.bmf_last_error()
    for over, text in ((dict(rows_pad=100), b"multiple of 64"), (dict(rows_pad=0), b"multiple of 64"), (dict(rows=0), b"rows"), (dict(rows=129), b"rows"),
                       (dict(kp=48), b"kp"), (dict(kp=128), b"kp"), (dict(k=0), b"k="), (dict(k=33), b"k="), (dict(k=65, kp=64), b"k="),
                       (dict(T=0), b"T must"), (dict(T=-1), b"T must"), (dict(ldcb=3), b"ldcb"), (dict(ldcb=6), b"ldcb"),
                       (dict(F64=C.c_void_p(4104)), b"aligned"), (dict(colbits=C.c_void_p(4100)), b"aligned")):
        assert panels(lib, **over) == -1, over
        assert text in lib.bmf_last_error(), (over, lib.bmf_last_error())
    for pairs_mode, who in ((False, b"bmf_grid_cover_count"), (True, b"bmf_pairs_cover_count")):
        for name in ("X", "rb0", "cb0", "counts"):
            assert cover(lib, pairs_mode, **{name: None}) == -1 and who + b": null pointer" in lib.bmf_last_error(), name
        for over, text in ((dict(rb1=C.c_void_p(4096)), b"go together"), (dict(cb1=C.c_void_p(4096)), b"go together"),
                           (dict(rb1=C.c_void_p(4096), cb1=C.c_void_p(4096)), b"kp == 64"),
                           (dict(rows_pad=100), b"multiple of 64"), (dict(rows_pad=0), b"multiple of 64"), (dict(rows_pad=64 * 65536), b"rows_pad"),
                           (dict(words=0), b"words"), (dict(words=6), b"words"), (dict(ldx=4), b"ldx"), (dict(ldx=10), b"ldx"),
                           (dict(ldcb=4), b"ldcb"), (dict(ldcb=10), b"ldcb"), (dict(kp=16), b"kp"), (dict(kp=48), b"kp"),
                           (dict(A=0), b"A must"), (dict(B=0), b"A must"), (dict(B=65536), b"A must"),
                           (dict(X=C.c_void_p(4100)), b"aligned"), (dict(cb0=C.c_void_p(4104)), b"aligned")):
            assert cover(lib, pairs_mode, **over) == -1, over
            assert who in lib.bmf_last_error() and text in lib.bmf_last_error(), (over, lib.bmf_last_error())
    assert cover(lib, True, pairs=None) == -1 and b"pairs" in lib.bmf_last_error()
    assert cover(lib, True, T=0) == -1 and b"T >= 1" in lib.bmf_last_error()
    # the plan query is host arithmetic
    cw, rpb, ab = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    assert lib.bmf_grid_cover_plan(128, 8, 5, None, C.byref(rpb), C.byref(ab)) == -1 and b"bmf_grid_cover_plan: null pointer" in lib.bmf_last_error()
    for bad in ((100, 8, 5), (0, 8, 5), (128, 6, 5), (128, 0, 5), (128, 8, 0)):
        assert lib.bmf_grid_cover_plan(*bad, C.byref(cw), C.byref(rpb), C.byref(ab)) == -1, bad
        assert (cw.value, rpb.value, ab.value) == (-7, -7, -7)
    assert lib.bmf_grid_cover_plan(128, 8, 5, C.byref(cw), C.byref(rpb), C.byref(ab)) == 0
    assert cw.value == 128 and rpb.value == 64 and ab.value == 64
    assert lib.bmf_grid_cover_plan(6144, 128, 40, C.byref(cw), C.byref(rpb), C.byref(ab)) == 0 and rpb.value == 128 and rpb.value <= 512
    assert lib.bmf_grid_cover_plan(1 << 20, 128, 40, C.byref(cw), C.byref(rpb), C.byref(ab)) == 0 and rpb.value == 512   # never above 512: the packed fields
