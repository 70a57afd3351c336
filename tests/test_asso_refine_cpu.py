"""AssoIter and AssoOpt without a GPU: the models' host loops (models/AssoIter.py, AssoOpt.py) on a NumPy stand-in that offers the
calls of pybmf_amd.asso_refine.AssoRefineEngine (load_factors / refine_column / optimal_rows / chosen / counts / factor_arrays /
prediction), against what the reference produced (tests/golden/g25_asso_refine.*, written by tests/golden/make_golden_asso_refine.py).

The stand-in restates both steps on dense matrices: a column visit as the Boolean product of the other k - 1 factors, the integer TP /
FP per row with and without basis k, the reference's fp64 comparison on them, T, F = the sums of the chosen side, score = w_fn T - w_fp
F; the row search as the scores of all 2^k subsets (factor 0 the most significant bit of j) and np.argmax.  The real classes on it
must reproduce every case: U cell for cell, the sequence of column visits (k, error, refined or skipped) and so the stop point, the
counts, `error` equal (==), `score` equal (==) where the weights are dyadic (0.5 / 0.5, 1 / 1) and within 1e-12 relative otherwise
(the reference adds per-row scores, the restatement multiplies the sums -- the bound test_asso_* use for that), the metric columns
within 1e-12 (ratios of equal integers), j per row equal.

AssoOpt ends, in the reference, in an AttributeError after U is final and before it logs (the fixture records that); what is asserted
there is U, j, the prediction's counts, and that the model here finishes with one row in logs['refinements'].
"""
import contextlib
import ctypes as C
import io
import json
import os
import re
import types

import numpy as np
import pytest
from scipy.sparse import csr_matrix, lil_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
ITER_CASES = ["iter_a", "iter_b", "iter_c", "iter_d", "iter_e"]
OPT_CASES = ["opt_a", "opt_b", "opt_c", "opt_d", "opt_e"]
MUST_CHANGE = ["iter_a", "iter_b", "iter_c", "iter_d", "opt_a", "opt_b", "opt_d"]


def dyadic(w_fp, w_fn):
    return (w_fp, w_fn) in ((0.5, 0.5), (1.0, 1.0))


# ---- the two steps in NumPy -------------------------------------------------------------------------------------------------
def refine_column_numpy(X, U, V, kc, w_fp, w_fn):
    """(new column, score, T, F) of one AssoIter visit of column kc; X, U, V dense bool."""
    k = U.shape[1]
    idx = [l for l in range(k) if l != kc]
    old = (U[:, idx].astype(np.int64) @ V[:, idx].T.astype(np.int64)) > 0
    new = old | V[:, kc][None, :]
    tp_old, fp_old = (X & old).sum(axis=1), (~X & old).sum(axis=1)
    tp_new, fp_new = (X & new).sum(axis=1), (~X & new).sum(axis=1)
    take = -w_fp * fp_new.astype(np.float64) + w_fn * tp_new.astype(np.float64) > -w_fp * fp_old.astype(np.float64) + w_fn * tp_old.astype(np.float64)
    T, F = int(np.where(take, tp_new, tp_old).sum()), int(np.where(take, fp_new, fp_old).sum())
    return take, w_fn * float(T) - w_fp * float(F), T, F


def subset_scores(X, V, w_fp, w_fn):
    """scores[j, i] of subset j of the factors against row i of X, j = 0 .. 2^k - 1 with factor l = bit k - 1 - l of j; and TP, FP."""
    k = V.shape[1]
    member = (np.arange(1 << k)[:, None] >> (k - 1 - np.arange(k))[None, :]) & 1
    P = (member.astype(np.int64) @ V.T.astype(np.int64)) > 0
    TP = P.astype(np.int64) @ X.T.astype(np.int64)
    FP = P.sum(axis=1)[:, None] - TP
    return -w_fp * FP.astype(np.float64) + w_fn * TP.astype(np.float64), TP, FP


def optimal_rows_numpy(X, V, w_fp, w_fn):
    """(j per row, the new U, T, F): np.argmax over all subsets, the first of equals."""
    k = V.shape[1]
    scores, TP, FP = subset_scores(X, V, w_fp, w_fn)
    j = scores.argmax(axis=0)
    rows = np.arange(X.shape[0])
    U = ((j[:, None] >> (k - 1 - np.arange(k))[None, :]) & 1).astype(bool)
    return j.astype(np.int64), U, int(TP[j, rows].sum()), int(FP[j, rows].sum())


class NumpyRefineEngine:
    """pybmf_amd.asso_refine.AssoRefineEngine in NumPy on dense matrices, same interface."""

    def __init__(self, X, extra=None):
        self.X = np.asarray(X) != 0
        self.m, self.n = self.X.shape
        self.sum_x = int(self.X.sum())
        self.truth = {"train": self.X}
        for name, G in (extra or {}).items():
            self.truth[name] = np.asarray(G) != 0
        self.k = 0

    def load_factors(self, U, V):
        self.U, self.V = (np.asarray(U) != 0).copy(), (np.asarray(V) != 0).copy()
        assert self.U.shape[0] == self.m and self.V.shape[0] == self.n and self.U.shape[1] == self.V.shape[1] >= 1
        self.k = self.U.shape[1]

    def refine_column(self, k, w_fp, w_fn, chunk=None):
        take, score, T, F = refine_column_numpy(self.X, self.U, self.V, k, float(w_fp), float(w_fn))
        self.U[:, k] = take
        self._column = take
        return score, T, F, int(take.sum())

    def column(self):
        return self._column

    def optimal_rows(self, w_fp, w_fn, chunk=None):
        if self.k > 16:
            raise NotImplementedError("k <= 16")
        self._j, self.U, T, F = optimal_rows_numpy(self.X, self.V, float(w_fp), float(w_fn))
        return float(w_fn) * float(T) - float(w_fp) * float(F), T, F, int(self.U.sum())

    def chosen(self):
        return self._j

    def _pd(self):
        return (self.U.astype(np.int64) @ self.V.T.astype(np.int64)) > 0

    def counts(self, name="train"):
        G, P = self.truth[name], self._pd()
        tp, fp, fn = int((G & P).sum()), int((~G & P).sum()), int((G & ~P).sum())
        return tp, fp, fn, self.m * self.n - tp - fp - fn

    def factor_arrays(self):
        return self.U.astype(np.uint8), self.V.astype(np.uint8)

    def prediction(self):
        return csr_matrix(self._pd().astype(int))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g25_asso_refine.json")))
    z = np.load(os.path.join(GOLDEN, "g25_asso_refine.npz"))
    c = dict(meta["cases"][name])
    for key in ("X", "X_val", "X_test", "U_in", "V", "U", "j"):
        if f"{name}_{key}" in z.files:
            c[key] = z[f"{name}_{key}"]
    c["weights"] = (float(c["w_fp"]), 1 - c["w_fp"] if c["w_fn"] is None else float(c["w_fn"]))
    return c


def stand_in_model(U, V, k=-1):
    """An object with k, U, V, logs: all a refiner imports."""
    return types.SimpleNamespace(k=U.shape[1] if k == -1 else k, U=lil_matrix(np.asarray(U, dtype=np.float64)),
                                 V=lil_matrix(np.asarray(V, dtype=np.float64)), logs={})


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyRefineEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, kind, engine_factory=None):
    """The real class (kind: 'AssoIter' / 'AssoOpt') on case's matrices; engine_factory(model) replaces the device engine."""
    import pybmf_amd.models as M

    class Model(getattr(M, kind)):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        model = Model(model=stand_in_model(case["U_in"], case["V"]), w_fp=case["w_fp"], w_fn=case["w_fn"])
        model.fit(sp("X"), sp("X_val"), sp("X_test"), **FIT_KW)
    model.printed = out.getvalue()
    return model


def check_common(model, case):
    m, n = case["shape"]
    U, V = np.asarray(model.U.todense()), np.asarray(model.V.todense())
    from scipy.sparse import isspmatrix_lil
    assert isspmatrix_lil(model.U) and isspmatrix_lil(model.V)
    assert U.shape == case["U"].shape == (m, case["k"])
    assert (U != 0).tolist() == (case["U"] != 0).tolist() and (V != 0).tolist() == (case["V"] != 0).tolist()
    assert int(((U != 0) != (case["U_in"] != 0)).sum()) == case["cells_changed"]
    eng = model._engine
    assert list(eng.counts("train")) == case["counts"]
    X_pd = np.asarray(model.X_pd.todense()) != 0
    want = (case["U"].astype(np.int64) @ case["V"].T.astype(np.int64)) > 0
    assert X_pd.tolist() == want.tolist()
    Ue, Ve = eng.factor_arrays()
    assert (Ue != 0).tolist() == (U != 0).tolist() and (Ve != 0).tolist() == (V != 0).tolist()


def check_score(got, want, exact):
    if exact:
        assert float(got) == want
    else:
        assert abs(float(got) - want) <= 1e-12 * abs(want)


def check_iter(model, case):
    exact = dyadic(*case["weights"])
    assert [[v[0], v[1], v[2]] for v in model.visits] == [[v[0], v[1], v[2]] for v in case["visits"]]      # k, error (==), refined
    cols, want = case["log"]["columns"], case["log"]["rows"]
    got = [r[1:] for r in model.logs["refinements"].values.tolist()] if "refinements" in model.logs else []
    assert len(got) == len(want) == sum(v[2] for v in case["visits"])
    assert not want or cols[:3] == ["k", "train/score", "train/error"]
    if want:
        assert [c[-1] for c in model.logs["refinements"].columns][1:] == [c.split("/")[-1] for c in cols]
    logged = [v for v in case["visits"] if v[2]]
    for g, w, v in zip(got, want, logged):
        assert int(g[0]) == w[0] == v[0] and float(g[2]) == w[2] == v[1]
        check_score(g[1], w[1], exact)
    if want:
        G, Wt = np.array([r[3:] for r in got], dtype=np.float64), np.array([r[3:] for r in want])
        assert G.shape == Wt.shape and np.abs(G - Wt).max() <= 1e-12
    # the stop: k skipped visits in a row end the fit, nothing follows them
    k = case["k"]
    flags = [v[2] for v in model.visits]
    assert flags[-k:] == [False] * k and all(any(flags[i:i + k]) for i in range(len(flags) - k))
    assert model.printed.count("Refined column") == sum(flags) and model.printed.count("Skipped column") == len(flags) - sum(flags)
    assert model.printed.count("Error stops decreasing.") == 1
    check_common(model, case)


def check_opt(model, case):
    assert model.chosen.tolist() == case["j"].tolist()
    assert case["raised"] == "AttributeError" and case["log"]["rows"] == []      # the reference logs nothing; here the model finishes
    rows = model.logs["refinements"].values.tolist()
    assert len(rows) == 1 and [c[-1] for c in model.logs["refinements"].columns][1:] == ["score", "Recall", "Precision", "Accuracy", "F1"]
    tp, fp, fn, tn = case["counts"]
    w_fp, w_fn = case["weights"]
    assert float(rows[0][1]) == -w_fp * np.float64(fp) + w_fn * np.float64(tp)
    assert abs(rows[0][2] - tp / max(tp + fn, 1)) <= 1e-12 and abs(rows[0][4] - (tp + tn) / (tp + fp + fn + tn)) <= 1e-12
    assert "Exhaustive search finished" in model.printed
    check_common(model, case)


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_what_the_tests_rely_on():
    for name in ITER_CASES + OPT_CASES:
        case = load_case(name)
        if name in MUST_CHANGE:       # no test can pass by handing U back
            assert case["cells_changed"] >= 1 and (case["U"] != case["U_in"]).any()
    d = load_case("iter_d")
    flags = [v[2] for v in d["visits"]]
    assert len(flags) > d["k"] and any((not a) and any(flags[i + 1:]) for i, a in enumerate(flags))      # a second round; a skip, then a refinement
    e = load_case("opt_e")
    assert not e["X"][5].any() and not e["V"][:, 2].any()
    assert load_case("opt_c")["k"] == 1 and load_case("opt_d")["k"] == 8 and load_case("opt_d")["shape"] == [40, 30]
    assert "X_val" in load_case("iter_e") and "X_test" in load_case("iter_e")


@pytest.mark.parametrize("name", ITER_CASES)
def test_assoiter_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    check_iter(fit_case(case, "AssoIter", numpy_engine), case)


@pytest.mark.parametrize("name", OPT_CASES)
def test_assoopt_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    check_opt(fit_case(case, "AssoOpt", numpy_engine), case)


def test_iter_e_logs_every_data_set():
    case = load_case("iter_e")
    model = fit_case(case, "AssoIter", numpy_engine)
    assert [c[0] for c in model.logs["refinements"].columns][4:] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4
    assert [c.split("/")[0] for c in case["log"]["columns"][3:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4


def test_the_imported_model_keeps_its_own_factors_and_shares_its_logs():
    case = load_case("iter_a")
    from pybmf_amd.models import AssoIter

    class Model(AssoIter):
        def _make_engine(self):
            return numpy_engine(self)
    src = stand_in_model(case["U_in"], case["V"])
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(model=src, w_fp=0.3)
        assert model.U is src.U and model.k == src.k and model.logs is src.logs and model.w_fn is None
        model.fit(csr_matrix(case["X"].astype(np.float64)), **FIT_KW)
    assert (np.asarray(src.U.todense()) != 0).tolist() == (case["U_in"] != 0).tolist()
    assert "refinements" in src.logs


def test_refusals():
    from pybmf_amd.models import AssoIter, AssoOpt
    case = load_case("opt_c")
    X = csr_matrix(case["X"].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        for cls in (AssoIter, AssoOpt):
            with pytest.raises(NotImplementedError, match="reconstruction"):
                cls(model=stand_in_model(case["U_in"], case["V"])).fit(X, **dict(FIT_KW, task="prediction"))
            with pytest.raises(NotImplementedError, match="Boolean"):
                cls(model=stand_in_model(case["U_in"], case["V"])).fit(case["X"].astype(np.float64) * 3, **FIT_KW)
            with pytest.raises(TypeError, match="k is None"):
                cls(model=stand_in_model(case["U_in"], case["V"], k=None)).fit(X, **FIT_KW)

        # k = 17: the model refuses before it builds an engine, and so does the device engine's own check (no GPU needed for it)
        rng = np.random.RandomState(0)
        with pytest.raises(NotImplementedError, match="k <= 16"):
            AssoOpt(model=stand_in_model(rng.rand(40, 17) < 0.2, rng.rand(30, 17) < 0.2)).fit(X, **FIT_KW)
    from pybmf_amd.asso_refine import AssoRefineEngine
    eng = AssoRefineEngine.__new__(AssoRefineEngine)
    eng.ldx = 16
    for k, rows_kernel, ok in ((16, True, True), (17, True, False), (17, False, True), (1024, False, True), (1025, False, False)):
        eng.k = k
        if ok:
            assert eng._chunk(None, rows_kernel) == 0 and eng._chunk(8, rows_kernel) == 8
        else:
            with pytest.raises(NotImplementedError, match="k <= 16" if rows_kernel else "k <= 1024"):
                eng._chunk(None, rows_kernel)


class _DeviceHandles:
    """What a fitted pybmf_amd model carries as `_engine`: ctypes pointers, which do not pickle."""

    def __init__(self):
        self._stream = C.c_void_p(1)


def test_the_default_fit_saves_a_pickle_without_the_imported_model(tmp_path, monkeypatch):
    """fit() with the default save_model=True on a source model that holds device handles: the imported model is not kept, so the
    pickle is written and holds the refined factors and the logs."""
    import pickle
    from pybmf_amd.models import AssoIter, AssoOpt
    monkeypatch.setenv("HOME", str(tmp_path))
    with pytest.raises(ValueError, match="ctypes objects containing pointers"):
        pickle.dumps(_DeviceHandles())
    for cls, name in ((AssoIter, "iter_a"), (AssoOpt, "opt_c")):
        case = load_case(name)

        class Model(cls):
            def _make_engine(self):
                return numpy_engine(self)
        source = stand_in_model(case["U_in"], case["V"])
        source._engine = _DeviceHandles()
        with contextlib.redirect_stdout(io.StringIO()):
            model = Model(model=source, w_fp=case["w_fp"], w_fn=case["w_fn"])
            assert not hasattr(model, "model")
            model.fit(csr_matrix(case["X"].astype(np.float64)), task="reconstruction", show_logs=False, show_result=False)
        assert os.path.exists(model.pickle_path) and model.pickle_path.startswith(str(tmp_path))
        with open(model.pickle_path, "rb") as fh:
            saved = pickle.load(fh)
        assert "model" not in saved and saved["k"] == model.k and "refinements" in saved["logs"]
        assert np.asarray(saved["U"].todense()).tolist() == case["U"].astype(np.float64).tolist()


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {"bmf_asso_refine_chunk": 3, "bmf_asso_refine_column": 15, "bmf_asso_refine_rows": 13, "bmf_asso_refine_product": 8}


def test_entry_points_are_declared_exported_and_bound():
    from pybmf_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmf_hip.h")).read(), flags=re.S)
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in NEW_ENTRY_POINTS.items():
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in bmf_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(raw, name), f"{name} is missing from libbmf_hip.so"
        res, args = L.SIGNATURES[name]
        assert len(args) == n_args and res is C.c_int


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    from pybmf_amd import asso_refine as R
    lib = L.lib
    # the chunk: all of a bit row when k rows of it (+ 4 words each) fit 60 KiB, else the largest multiple of 4 that does
    assert lib.bmf_asso_refine_chunk(8, 128, 0) == 128 and lib.bmf_asso_refine_chunk(64, 256, 0) == 236
    assert lib.bmf_asso_refine_chunk(33, 640, 0) == 460 and lib.bmf_asso_refine_chunk(1024, 16, 0) == 8
    assert lib.bmf_asso_refine_chunk(12, 128, 1) == 128 and lib.bmf_asso_refine_chunk(16, 1024, 1) == 896
    assert lib.bmf_asso_refine_chunk(R.K_MAX_COLUMN, 16, 0) > 0 and lib.bmf_asso_refine_chunk(R.K_MAX_COLUMN + 1, 16, 0) == -1
    assert lib.bmf_asso_refine_chunk(R.K_MAX_ROWS, 16, 1) > 0 and lib.bmf_asso_refine_chunk(R.K_MAX_ROWS + 1, 16, 1) == -1
    assert lib.bmf_asso_refine_chunk(0, 16, 0) == -1 and lib.bmf_asso_refine_chunk(4, 24, 0) == -1
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    col = lambda **kw: lib.bmf_asso_refine_column(*[kw.get(a, d) for a, d in (("X", p), ("ldx", 16), ("m", 4), ("V", p), ("k", 3), ("U", p), ("kw", 1),
                                                                                ("kc", 0), ("chunk", 0), ("w_fp", 0.5), ("w_fn", 0.5), ("u", p),
                                                                                ("part", p), ("rec", p), ("stream", None))])
    assert col(V=None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert col(ldx=24) == -1 and b"multiple of 16" in lib.bmf_last_error()
    assert col(m=0) == -1 and col(k=0) == -1 and col(kc=3) == -1 and col(kc=-1) == -1 and col(kw=2) == -1
    assert col(k=1025, kw=33) == -1 and b"1024" in lib.bmf_last_error()
    assert col(chunk=6) == -1 and col(chunk=20) == -1 and b"chunk" in lib.bmf_last_error()
    assert col(w_fn=float("nan")) == -1
    assert col(X=C.c_void_p(p.value + 4)) == -1
    rows = lambda **kw: lib.bmf_asso_refine_rows(*[kw.get(a, d) for a, d in (("X", p), ("ldx", 16), ("m", 4), ("V", p), ("k", 3), ("chunk", 0),
                                                                              ("w_fp", 1.0), ("w_fn", 1.0), ("j", p), ("U", p), ("part", p),
                                                                              ("rec", p), ("stream", None))])
    assert rows(j=None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert rows(k=17) == -1 and b"16" in lib.bmf_last_error()
    assert rows(k=0) == -1 and rows(m=0) == -1 and rows(ldx=8) == -1 and rows(chunk=3) == -1 and rows(w_fp=float("nan")) == -1
    assert lib.bmf_asso_refine_product(p, 1, p, 3, 16, 4, None, None) == -1
    assert lib.bmf_asso_refine_product(p, 2, p, 3, 16, 4, p, None) == -1 and lib.bmf_asso_refine_product(p, 1, p, 3, 16, 0, p, None) == -1
