"""Hyper without a GPU: the model's host replay (models/Hyper.py) on a NumPy stand-in that offers the calls of
pybmf_amd.hyper.HyperEngine (mine / evaluate_all / commit / apply / residual_sum / counts / tidsets / committed_T / reads), against
what the reference produced (tests/golden/g30_hyper.*, written by tests/golden/make_golden_hyper.py: the reference under a stable
argsort and the stand-in miner).

The stand-in works on packed uint32 words in the engine's layout (hyper_ref.py).  The real class on it must reproduce every recorded
fit: the mined itemsets in order, every log row (k, iter, |T|, |I| as integers, the metric columns to 1e-12: ratios of equal
integers), T and I as sets, U, V and the counts cell for cell, and the exception's name where the reference raises.
"""
import contextlib
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import hyper_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
CASES = ["a", "b", "c", "d", "e", "f", "g", "h"]


class NumpyHyperEngine:
    """pybmf_amd.hyper.HyperEngine in NumPy, same layout, same interface."""

    def __init__(self, X, extra=None):
        X = np.asarray(X) != 0
        self.X, (self.m, self.n) = X, X.shape
        self.W, self.nvw = H.words_of(self.m), -(-self.n // 512) * 16
        self.x_t = H.pack_rows(X.T, self.W)
        self.rs_t, self.pd_t = self.x_t.copy(), np.zeros_like(self.x_t)
        self.sum_x = int(X.sum())
        self.truth = {"train": self.x_t}
        for name, G in (extra or {}).items():
            self.truth[name] = H.pack_rows((np.asarray(G) != 0).T, self.W)
        self._factors, self.itemsets, self.n_cand, self.reads = [], None, 0, 0

    def mine(self, min_support):
        sets, self.support_counts = H.mine(self.X, min_support)
        self.itemsets = [[j] for j in range(self.n)] + sets
        self.n_cand = C_ = len(self.itemsets)
        self._tid = np.array([np.bitwise_and.reduce(self.x_t[I], axis=0) for I in self.itemsets], dtype=np.uint32).reshape(C_, self.W)
        self._scratch, self._committed = np.zeros_like(self._tid), np.zeros_like(self._tid)
        self._rec, self._items = np.zeros((C_, 2), dtype=np.int64), H.pad_items(self.itemsets)
        self.reads += max((len(I) for I in sets), default=1)      # one read per level
        return sets

    def evaluate_all(self, ids=None):
        ids = np.arange(self.n_cand) if ids is None else np.asarray(ids)
        if len(ids):
            self._scratch[ids], self._rec[ids, 0], self._rec[ids, 1] = H.evaluate(self._tid, self.rs_t, self._items, ids)
        self.reads += 1
        return self._rec[:, 0].copy(), self._rec[:, 1].copy()

    def commit(self, ids):
        for i in ids:
            self._committed[i] = self._scratch[i]

    def apply(self, cid):
        T, I = self._committed[cid].copy(), self.itemsets[cid]
        self.rs_t[I] &= ~T
        self.pd_t[I] |= T
        v = H.pack_rows(np.isin(np.arange(self.n), I)[None, :], self.nvw)[0]
        self._factors.append((T, v))
        self.reads += 1
        return T

    def residual_sum(self):
        return H.popcount(self.rs_t)

    def counts(self, name="train"):
        G, pd = self.truth[name], self.pd_t
        if name != "train":
            self.reads += 1
        tp, n_pd, n_gt = H.popcount(pd & G), H.popcount(pd), H.popcount(G)
        return tp, n_pd - tp, n_gt - tp, self.m * self.n - n_pd - (n_gt - tp)

    def prediction(self):
        return csr_matrix(H.unpack_rows(self.pd_t[: self.n], self.m).T.astype(int))

    def tidsets(self):
        return self._tid

    def committed_T(self, cid):
        return self._committed[cid]

    def bit_matrices(self):
        return self.rs_t, self.pd_t


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_meta():
    return json.load(open(os.path.join(GOLDEN, "g30_hyper.json")))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, "g30_hyper.npz"))
    c = dict(load_meta()["cases"][name])
    for key in ("X", "U", "V", "X_val", "X_test"):
        if f"{name}_{key}" in z.files:
            c[key] = z[f"{name}_{key}"]
    return c


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyHyperEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, engine_factory=None):
    """(model, exception name or None): the real class on case's matrices; engine_factory(model) replaces the device engine."""
    from pybmf_amd.models import Hyper

    class Model(Hyper):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    raised = None
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(min_support=case["min_support"])
        try:
            model.fit(sp("X"), sp("X_val"), sp("X_test"), **FIT_KW)
        except IndexError as exc:
            raised = type(exc).__name__
    return model, raised


def log_rows(model):
    """[[k, iter, |T|, |I|, metrics ...]] of logs['updates'] (time stamp dropped, the shape cell flattened)."""
    if "updates" not in model.logs:
        return []
    return [[r[1], r[2], r[3][0], r[3][1]] + [float(x) for x in r[4:]] for r in model.logs["updates"].values.tolist()]


def check_fit(model, raised, case):
    eng = model._engine
    assert raised == case["raised"]
    assert eng.itemsets[eng.n:] == case["itemsets"] and eng.itemsets[:eng.n] == [[j] for j in range(eng.n)]
    assert [int(x) for x in eng.support_counts] == case["itemset_counts"]
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want)
    if want:
        assert case["log"]["columns"][:4] == ["k", "iter", "n_u", "n_v"]
    for g, w in zip(got, want):
        assert all(isinstance(x, (int, np.integer)) for x in g[:4]) and [int(x) for x in g[:4]] == w[:4]
        assert len(g) == len(w) and np.abs(np.array(g[4:]) - np.array(w[4:])).max() <= 1e-12
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    assert U.shape == case["U"].shape and V.shape == case["V"].shape
    assert (U == (case["U"] != 0)).all() and (V == (case["V"] != 0)).all()
    if not raised:
        assert model.k == case["k"] == U.shape[1]
        assert [sorted(T) for T in model.T] == [sorted(T) for T in case["T"]] and all(T == sorted(T) for T in model.T)
        assert [sorted(I) for I in model.I] == [sorted(I) for I in case["I"]] and all(I == sorted(I) for I in model.I)
    assert list(eng.counts("train")) == case["counts"]
    X = case["X"]
    X_pd = np.asarray(model.X_pd.todense()) if model.X_pd is not None or want else np.zeros_like(X)
    assert [int((X_pd & X).sum()), int((X_pd & (1 - X)).sum())] == case["counts"][:2]
    assert eng.residual_sum() == case["counts"][2]
    check_state(eng, X, X_pd)


def check_state(eng, X, X_pd):
    """The residual is X & ~X_pd, the cover is X_pd, nothing is set in the padding."""
    m, n = X.shape
    rs_t, pd_t = eng.bit_matrices()
    R, P = H.unpack_rows(rs_t[:n], m).T, H.unpack_rows(pd_t[:n], m).T
    assert (P == (X_pd != 0)).all() and (R == ((X != 0) & ~P)).all()
    assert H.popcount(rs_t) == int(R.sum()) and H.popcount(pd_t) == int(P.sum())


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_replay_reproduces_the_reference(name):
    case = load_case(name)
    model, raised = fit_case(case, numpy_engine)
    check_fit(model, raised, case)
    rows = case["log"]["rows"]
    if name == "a":      # the lazy greedy at work: thousands of head evaluations, an exact cover at the end
        assert sum(r[1] for r in rows) > 2000 and case["counts"][1:3] == [0, 0]
    if name == "c":
        assert case["itemsets"] == []
    if name == "e":
        assert any(case["stale"])
    if name == "f":      # X = 0: no candidate survives init_transactions, no round runs, k = U.shape[1] = 1
        assert rows == [] and raised is None and model.k == 1 and model.T == [] and model.I == []
    if name == "g":      # one column: c[1] on a list of one
        assert raised == "IndexError"
    if name == "h":
        assert [c.split("/")[0] for c in case["log"]["columns"][4:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4


def test_fixture_holds_a_stale_head_and_the_replay_accepts_it():
    """Case e: the reference accepted a head whose T came from an earlier residual.  The replay's committed T is that stale T, not
    the fresh one, and the factor is still an exact rectangle of X."""
    case = load_case("e")
    assert any(case["stale"])
    seen = []

    def factory(model):
        eng = numpy_engine(model)
        apply = eng.apply

        def logged(cid):
            fresh = H.evaluate(eng._tid, eng.rs_t, eng._items, [cid])[0][0]
            seen.append(not np.array_equal(fresh, eng.committed_T(cid)))
            return apply(cid)
        eng.apply = logged
        return eng
    model, raised = fit_case(case, factory)
    assert seen == case["stale"]
    X = case["X"] != 0
    for T, I in zip(model.T, model.I):
        assert X[np.ix_(T, I)].all()
    check_fit(model, raised, case)


def test_ties_follow_the_stable_rule():
    """Case d has a duplicated column: its singletons and every pair of itemsets that differ only in that column tie in cost."""
    case = load_case("d")
    X = case["X"]
    a, b = case["duplicate"]
    assert (X[:, a] == X[:, b]).all() and X[:, a].any()
    model, raised = fit_case(case, numpy_engine)
    check_fit(model, raised, case)


def test_stand_in_miner_on_hand_made_data():
    X = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 0], [0, 1, 1, 1]])
    assert H.mine(X, 0.5) == ([[0, 1], [0, 2], [1, 2], [0, 1, 2]], [3, 2, 3, 2])
    assert H.mine(X, 0.75) == ([[0, 1], [1, 2]], [3, 3])
    assert H.mine(X, 0.76) == ([], [])
    assert H.mine(np.zeros((3, 2)), 0.5) == ([], [])


def test_reads_are_counted_per_residual_not_per_iteration():
    case = load_case("a")
    model, _ = fit_case(case, numpy_engine)
    rows = len(case["log"]["rows"])
    assert model._engine.reads <= 4 * rows + 4 < sum(r[1] for r in case["log"]["rows"])


def test_refusals():
    from pybmf_amd.models import Hyper
    case = load_case("a")
    X = csr_matrix(case["X"].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match="reconstruction"):
            Hyper(min_support=0.3).fit(X, **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            Hyper(min_support=0.3).fit(case["X"].astype(np.float64) * 3, **FIT_KW)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {"bmf_hyper_level": 10, "bmf_hyper_eval": 12, "bmf_hyper_copy": 9}


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
    assert L.lib.bmf_version() == 501


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    p16 = C.c_void_p((p.value + 15) & ~15)
    off = C.c_void_p(p16.value + 4)
    assert lib.bmf_hyper_level(None, 4, p16, 4, 16, p16, 1, p16, p16, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_hyper_level(p16, 0, p16, 4, 16, p16, 1, p16, p16, None) == -1
    assert lib.bmf_hyper_level(p16, 4, p16, 4, 18, p16, 1, p16, p16, None) == -1 and b"multiple of 4" in lib.bmf_last_error()
    assert lib.bmf_hyper_level(p16, 4, p16, 4, 16, p16, 0, p16, p16, None) == -1 and b"count" in lib.bmf_last_error()
    assert lib.bmf_hyper_level(p16, 4, off, 4, 16, p16, 1, p16, p16, None) == -1 and b"aligned" in lib.bmf_last_error()
    assert lib.bmf_hyper_eval(p16, p16, 4, 16, None, 1, p16, 1, 4, p16, p16, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_hyper_eval(p16, p16, 4, 16, p16, 0, p16, 1, 4, p16, p16, None) == -1 and b"maxlen" in lib.bmf_last_error()
    assert lib.bmf_hyper_eval(p16, p16, 4, 16, p16, 5, p16, 1, 4, p16, p16, None) == -1 and b"maxlen" in lib.bmf_last_error()
    assert lib.bmf_hyper_eval(p16, p16, 4, 20, p16, 1, p16, 1, 0, p16, p16, None) == -1
    assert lib.bmf_hyper_eval(p16, p16, 4, 16, p16, 1, p16, 1, 4, off, p16, None) == -1 and b"aligned" in lib.bmf_last_error()
    far = C.c_void_p(p16.value + 1024)
    assert lib.bmf_hyper_copy(p16, 4, p16, None, 4, p16, 16, 1, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_hyper_copy(p16, 4, p16, p16, 4, p16, 16, 1, None) == -1 and b"different" in lib.bmf_last_error()
    assert lib.bmf_hyper_copy(p16, 4, p16, far, 4, p16, 16, 0, None) == -1 and b"count" in lib.bmf_last_error()
    assert lib.bmf_hyper_copy(p16, 4, p16, far, 0, p16, 16, 1, None) == -1
    assert lib.bmf_hyper_copy(p16, 4, p16, far, 4, p16, 6, 1, None) == -1
