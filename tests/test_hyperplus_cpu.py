"""HyperPlus without a GPU: the model's host logic (models/HyperPlus.py) on a NumPy stand-in that offers the calls of
pybmf_amd.hyperplus.HyperPlusEngine (load_factors / score_pairs / merge / order / counts / prediction / factor_arrays / bit_matrices /
factor_bits / reads), against what the reference produced (tests/golden/g31_hyperplus.*, written by
tests/golden/make_golden_hyperplus.py: the reference's HyperPlus on a reference Hyper, NumPy's `Inf` given back to it).

The stand-in works on packed uint32 words in the engine's layout (hyperplus_ref.py).  The real class on it must reproduce every
recorded fit: the pair list of every round after np.random.seed, every trial's FP and fpb (equality: the same integers, the same fp64
quotient) and whether the budget refused it, the chosen pair, every log row (k as an integer, savings inf, the rates and the metric
columns to 1e-12: ratios of equal integers), logs['U'] / ['V'] per round, T and I in list order, U, V and the counts cell for cell.
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

import hyper_ref as H
import hyperplus_ref as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
CASES = ["a", "b", "c", "d", "e", "f", "g", "h", "i"]          # case j is a second fit on case a's model: its own test


class NumpyHyperPlusEngine:
    """pybmf_amd.hyperplus.HyperPlusEngine in NumPy, same layout, same interface."""

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
        self.order, self.k_slots, self.reads = [], 0, 0

    def _apply(self, slot):
        cols = np.nonzero(H.unpack_rows(self.v[slot][None, :], self.n)[0])[0]
        self.rs_t[cols] &= ~self.u_t[slot]
        self.pd_t[cols] |= self.u_t[slot]

    def load_factors(self, T_lists, I_lists):
        k = len(T_lists)
        assert len(I_lists) == k and not self.order
        self.u_t = H.pack_rows(np.array([np.isin(np.arange(self.m), T) for T in T_lists], dtype=bool).reshape(k, self.m), self.W)
        self.v = H.pack_rows(np.array([np.isin(np.arange(self.n), I) for I in I_lists], dtype=bool).reshape(k, self.n), self.nvw)
        if k == 0:
            self.u_t, self.v = np.zeros((1, self.W), dtype=np.uint32), np.zeros((1, self.nvw), dtype=np.uint32)
        for i in range(k):
            self._apply(i)
        self.k_slots, self.order = k, list(range(k))
        self.reads += 1 if k else 0

    def score_pairs(self, pairs):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) == 0:
            return tuple(np.zeros(0, dtype=np.int64) for _ in range(5))
        self.reads += 1
        rec = HP.pair_records(self.u_t[: max(self.k_slots, 1)], self.v, self.x_t, self.pd_t, self.n, pairs)
        return tuple(rec[:, i].copy() for i in range(5))

    def merge(self, slot_a, slot_b):
        assert slot_a != slot_b and slot_a in self.order and slot_b in self.order
        self.u_t, self.v = HP.union(self.u_t, self.v, slot_a, slot_b, slot_a)
        self._apply(slot_a)
        self.order = [s for s in self.order if s not in (slot_a, slot_b)] + [slot_a]
        self.reads += 1
        return self.u_t[slot_a].copy(), self.v[slot_a].copy()

    def counts(self, name="train"):
        G, pd = self.truth[name], self.pd_t
        if name != "train":
            self.reads += 1
        tp, n_pd, n_gt = H.popcount(pd & G), H.popcount(pd), H.popcount(G)
        return tp, n_pd - tp, n_gt - tp, self.m * self.n - n_pd - (n_gt - tp)

    def prediction(self):
        return csr_matrix(H.unpack_rows(self.pd_t[: self.n], self.m).T.astype(int))

    def factor_arrays(self):
        u, v = self.factor_bits()
        return H.unpack_rows(u, self.m).T.astype(np.uint8), H.unpack_rows(v, self.n).T.astype(np.uint8)

    def bit_matrices(self):
        return self.rs_t, self.pd_t

    def factor_bits(self):
        return self.u_t[self.order].reshape(len(self.order), self.W), self.v[self.order].reshape(len(self.order), self.nvw)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_case(name):
    z = np.load(os.path.join(GOLDEN, "g31_hyperplus.npz"))
    c = dict(json.load(open(os.path.join(GOLDEN, "g31_hyperplus.json")))["cases"][name])
    for key in z.files:
        if key.startswith(name + "_"):
            c[key[len(name) + 1:]] = z[key]
    return c


def hyper_of(case):
    """A stand-in for the fitted Hyper model of the case: the six attributes HyperPlus imports."""
    h = case["hyper"]
    return types.SimpleNamespace(U=lil_matrix(case["hyper_U"].astype(np.float64)), V=lil_matrix(case["hyper_V"].astype(np.float64)),
                                 T=[list(T) for T in h["T"]], I=[list(I) for I in h["I"]], k=h["k"], logs={})


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyHyperPlusEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, hyper=None, engine_factory=None, **more):
    """The real class on case's matrices and Hyper model, after np.random.seed(case's seed); engine_factory(model) replaces the
    device engine."""
    from pybmf_amd.models import HyperPlus

    class Model(HyperPlus):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    args = dict(case["args"], **more)
    if args.get("beta") is None:
        args.pop("beta", None)
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(model=hyper_of(case) if hyper is None else hyper, **args)
        np.random.seed(case["seed"])
        model.fit(sp("X"), sp("X_val"), sp("X_test"), **FIT_KW)
    return model


def log_rows(model):
    """[[k, savings, FPR, FPB, OCR, metrics ...]] of logs['refinements'] (time stamp dropped)."""
    if "refinements" not in model.logs:
        return []
    return [r[1:] for r in model.logs["refinements"].values.tolist()]


def dense(F):
    return np.asarray(F.todense()) != 0


def check_fit(model, case, rows_before=0):
    eng = model._engine
    # rounds: pair lists, trials, chosen pairs
    assert len(model.trials) == len(case["rounds"])
    for (trials, chosen), want in zip(model.trials, case["rounds"]):
        assert [list(t[:2]) for t in trials] == want["pairs"]
        assert [list(t) for t in trials] == want["trials"]              # FP, fpb to the bit, savings inf or None (refused)
        assert (None if chosen is None else list(chosen)) == want["chosen"]
    # log
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want) and rows_before <= len(want)
    if want:
        assert case["log"]["columns"][:5] == ["k", "savings", "FPR", "FPB", "OCR"]
    for g, w in zip(got, want):
        assert isinstance(g[0], (int, np.integer)) and int(g[0]) == w[0] and g[1] == w[1] == np.inf
        assert len(g) == len(w) and np.abs(np.array(g[2:], dtype=np.float64) - np.array(w[2:])).max() <= 1e-12
    merges = len(want) - rows_before
    assert len(model.logs["U"]) == len(model.logs["V"]) == merges == sum(r["chosen"] is not None for r in case["rounds"])
    for r in range(merges):
        assert np.array_equal(dense(model.logs["U"][r]), case[f"log_U{r}"] != 0) and np.array_equal(dense(model.logs["V"][r]), case[f"log_V{r}"] != 0)
        assert model.logs["U"][r].format == "lil"
    # factors
    final = case["final"]
    assert model.k == final["k"] == model.U.shape[1] == model.V.shape[1]
    assert model.T == final["T"] and model.I == final["I"]
    assert np.array_equal(dense(model.U), case["U"] != 0) and np.array_equal(dense(model.V), case["V"] != 0)
    assert list(eng.counts("train")) == case["counts"]
    X = case["X"]
    X_pd = np.asarray(model.X_pd.todense())
    assert [int((X_pd & X).sum()), int((X_pd & (1 - X)).sum())] == case["counts"][:2]
    check_state(model, X, X_pd)


def check_state(model, X, X_pd):
    """The cover is the Boolean product of the factors, the residual is X & ~cover, the device factors are the model's, nothing is
    set in the padding."""
    eng = model._engine
    m, n = X.shape
    rs_t, pd_t = eng.bit_matrices()
    R, P = H.unpack_rows(rs_t[:n], m).T, H.unpack_rows(pd_t[:n], m).T
    assert (P == (X_pd != 0)).all() and (R == ((X != 0) & ~P)).all()
    assert H.popcount(rs_t) == int(R.sum()) and H.popcount(pd_t) == int(P.sum())
    assert (P == ((dense(model.U).astype(int) @ dense(model.V).astype(int).T) > 0)).all()
    if model.T:
        u, v = eng.factor_bits()
        assert np.array_equal(H.unpack_rows(u, m).T, dense(model.U)) and H.popcount(u) == int(dense(model.U).sum())
        assert np.array_equal(H.unpack_rows(v, n).T, dense(model.V)) and H.popcount(v) == int(dense(model.V).sum())
        U, V = eng.factor_arrays()
        assert np.array_equal(U != 0, dense(model.U)) and np.array_equal(V != 0, dense(model.V))


def check_hyper_untouched(hyper, case):
    h = case["hyper"]
    assert hyper.k == h["k"] and hyper.T == h["T"] and hyper.I == h["I"]
    assert np.array_equal(dense(hyper.U), case["hyper_U"] != 0) and np.array_equal(dense(hyper.V), case["hyper_V"] != 0)


# ---- the reference's fits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_logic_reproduces_the_reference(name):
    case = load_case(name)
    hyper = hyper_of(case)
    model = fit_case(case, hyper, numpy_engine)
    check_fit(model, case)
    check_hyper_untouched(hyper, case)
    assert model.logs is hyper.logs and not hasattr(model, "model")
    rounds = case["rounds"]
    if name == "a":      # all ten pairs, down to k = 1, where the pair list is empty
        assert len(rounds[0]["pairs"]) == 10 and model.k == 1 and rounds[-1]["pairs"] == [] and rounds[-1]["k"] == 1
        assert sorted(map(tuple, rounds[0]["pairs"])) != list(map(tuple, rounds[0]["pairs"]))      # the sample's order inside one m
    if name == "b":
        assert len(rounds[0]["pairs"]) == 3
    if name == "c":      # trials refused before one passes; a last round in which none does
        refused = [[t[4] is None for t in r["trials"]] for r in rounds]
        assert refused[0][0] and not all(refused[0]) and all(refused[-1]) and model.k > 1
    if name == "d":
        assert "refinements" not in model.logs and model.logs["U"] == [] and model.k == case["hyper"]["k"]
    if name == "e":
        assert case["args"]["target_k"] == 3 and model.k == 2
    if name == "f":      # fpb == beta to the bit: accepted
        t = [t for t in rounds[0]["trials"] if t[:2] == rounds[0]["chosen"]][0]
        assert t[3] == case["args"]["beta"] and case["ties"] >= 1
    if name == "g":
        assert case["hyper"]["k"] > 50
    if name == "h":
        assert [c.split("/")[0] for c in case["log"]["columns"][5:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4
    if name == "i":      # X = 0: Hyper left k = 1 without a set; no round
        assert model.k == 1 and model.T == [] and rounds[0]["pairs"] == [] and "refinements" not in model.logs


def test_second_fit_appends_to_the_shared_log():
    """Case j: a second HyperPlus on the Hyper model that case a's fit has used: the rows of both fits in one frame, logs['U'] / ['V']
    started again, the Hyper model's own factors as they were."""
    a, j = load_case("a"), load_case("j")
    hyper = hyper_of(a)
    first = fit_case(a, hyper, numpy_engine)
    assert sorted(hyper.logs) == ["U", "V", "refinements"] and len(hyper.logs["U"]) == len(a["log"]["rows"])
    check_hyper_untouched(hyper, a)
    second = fit_case(j, hyper, numpy_engine)
    assert second.logs is hyper.logs is first.logs
    assert j["rows_before"] == len(a["log"]["rows"]) and j["log"]["rows"][: j["rows_before"]] == a["log"]["rows"]
    check_fit(second, j, rows_before=j["rows_before"])
    check_hyper_untouched(hyper, j)


def test_import_from_a_fitted_hyper_of_this_build():
    """Hyper (on its stand-in engine), then HyperPlus: the same run as from the fixture's recorded Hyper model, the log shared."""
    import test_hyper_cpu as HC
    case = load_case("a")
    hyper, raised = HC.fit_case(HC.load_case("a"), HC.numpy_engine)
    assert raised is None and hyper.T == case["hyper"]["T"] and hyper.I == case["hyper"]["I"] and hyper.k == case["hyper"]["k"]
    model = fit_case(case, hyper, numpy_engine)
    check_fit(model, case)
    check_hyper_untouched(hyper, case)
    assert model.logs is hyper.logs and sorted(hyper.logs) == ["U", "V", "refinements", "updates"] == case["hyper_log_keys"]
    assert len(hyper.logs["updates"]) == case["hyper"]["k"]


# ---- savings='new_fp' -------------------------------------------------------------------------------------------------------
def dense_replay(X, T, I, target_k, samples, beta, savings):
    """The trial loop on dense matrices, every trial's prediction built from the other factors: (T, I, [(k, savings, FP, pair)])."""
    X = np.asarray(X) != 0
    T, I, rows = [sorted(t) for t in T], [sorted(i) for i in I], []

    def cover(fs):
        P = np.zeros_like(X)
        for t, i in fs:
            P[np.ix_(t, i)] = True
        return P
    while True:
        k = len(T)
        every = [(m, n) for m in range(k) for n in range(m + 1, k)]
        idx = np.random.choice(a=len(every), size=min(samples, len(every)), replace=False)
        pairs = [every[i] for m in range(k) for i in idx if every[i][0] == m]
        fp_now = int((cover(zip(T, I)) & ~X).sum())
        best, best_s = None, 0
        for m, n in pairs:
            Tm, Im = sorted(set(T[m]) | set(T[n])), sorted(set(I[m]) | set(I[n]))
            fp = int((cover([(T[i], I[i]) for i in range(k) if i not in (m, n)] + [(Tm, Im)]) & ~X).sum())
            if np.float64(fp) / np.float64(X.sum()) > beta:
                continue
            saved = len(T[m]) + len(T[n]) + len(I[m]) + len(I[n]) - len(Tm) - len(Im)
            s = np.inf if savings == "reference" or fp == fp_now else np.float64(saved) / np.float64(fp - fp_now)
            if s > best_s:
                best, best_s = (m, n, Tm, Im, fp), s
        if best is None:
            return T, I, rows
        m, n, Tm, Im, fp = best
        T = [T[i] for i in range(k) if i not in (m, n)] + [Tm]
        I = [I[i] for i in range(k) if i not in (m, n)] + [Im]
        rows.append((len(T), float(best_s), fp, (m, n)))
        if not (np.float64(fp) / np.float64(X.sum()) <= beta and len(T) >= target_k):
            return T, I, rows


@pytest.mark.parametrize("name,savings,beta", [("a", "new_fp", np.inf), ("g", "new_fp", np.inf), ("h", "new_fp", 0.2), ("a", "reference", np.inf)])
def test_fit_against_a_dense_replay(name, savings, beta):
    case = load_case(name)
    args = dict(case["args"], beta=beta)
    model = fit_case(dict(case, args=args), None, numpy_engine, savings=savings)
    np.random.seed(case["seed"])
    T, I, rows = dense_replay(case["X"], case["hyper"]["T"], case["hyper"]["I"], args["target_k"], args["samples"], beta, savings)
    assert model.T == T and model.I == I and model.k == len(T) and len(rows) >= 3
    got = log_rows(model)
    assert [(int(g[0]), g[1]) for g in got] == [(r[0], r[1]) for r in rows]
    assert [c for _, c in model.trials if c is not None] == [r[3] for r in rows]
    assert model._engine.counts("train")[1] == rows[-1][2]
    if savings == "new_fp":
        assert any(np.isfinite(r[1]) for r in rows)          # finite savings decided at least one round
    check_state(model, case["X"], np.asarray(model.X_pd.todense()))


def hand_built():
    """Four rectangles on 8 x 8: 0 and 1 share a row and a column (merging them adds 3 false positives and saves 2), 2 and 3 have the
    same rows and disjoint columns (merging them adds none)."""
    T, I = [[0, 1, 2], [2, 3], [4, 5], [4, 5]], [[0, 1], [1, 2], [4, 5], [6, 7]]
    X = np.zeros((8, 8), dtype=np.uint8)
    for t, i in zip(T, I):
        X[np.ix_(t, i)] = 1
    U, V = lil_matrix((8, 4)), lil_matrix((8, 4))
    for f, (t, i) in enumerate(zip(T, I)):
        U[t, f], V[i, f] = 1, 1
    return X, types.SimpleNamespace(U=U, V=V, T=T, I=I, k=4, logs={})


def test_new_fp_savings_prefer_the_merge_that_adds_no_false_positive():
    X, hyper = hand_built()
    case = dict(X=X, args=dict(target_k=4, samples=500), seed=5)
    model = fit_case(case, hyper, numpy_engine, savings="new_fp")
    (trials, chosen), = model.trials
    assert [t[:2] for t in trials][0][0] == 0 and chosen == (2, 3)
    by_pair = {t[:2]: t for t in trials}
    assert by_pair[(0, 1)][2:] == (3, 3 / 17, 2 / 3) and by_pair[(2, 3)][2:] == (0, 0.0, np.inf)
    assert by_pair[(0, 2)][4] == 0.0                           # nothing shared: saves nothing, never merged
    assert model.T == [[0, 1, 2], [2, 3], [4, 5]] and model.I == [[0, 1], [1, 2], [4, 5, 6, 7]] and model._engine.counts("train")[1] == 0
    assert log_rows(model)[0][:2] == [3, np.inf]
    X, hyper = hand_built()
    model = fit_case(case, hyper, numpy_engine)                # the reference's rule: the first listed pair
    assert model.trials[0][1] == tuple(model.trials[0][0][0][:2]) and model.trials[0][1][0] == 0 and model._engine.counts("train")[1] > 0


# ---- the identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,merges", [("a", 0), ("a", 2), ("h", 3)])
def test_trial_fp_is_the_current_fp_plus_new_fp(name, merges):
    """For every pair: FP of (the other k - 2 factors OR the merged rectangle), computed densely, is FP + new_fp."""
    case = load_case(name)
    X = case["X"] != 0
    eng = NumpyHyperPlusEngine(X)
    T, I = [list(t) for t in case["hyper"]["T"]], [list(i) for i in case["hyper"]["I"]]
    eng.load_factors(T, I)
    for r in range(merges):
        m, n = case["rounds"][r]["chosen"]
        words_T, words_I = eng.merge(eng.order[m], eng.order[n])
        rest = [i for i in range(len(T)) if i not in (m, n)]
        T = [T[i] for i in rest] + [list(np.nonzero(H.unpack_rows(words_T[None, :], eng.m)[0])[0])]
        I = [I[i] for i in rest] + [list(np.nonzero(H.unpack_rows(words_I[None, :], eng.n)[0])[0])]
    k = len(T)
    pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
    new_fp, nT, nI, nTc, nIc = eng.score_pairs([(eng.order[a], eng.order[b]) for a, b in pairs])
    fp_now = eng.counts("train")[1]
    assert (fp_now > 0) == (merges > 0)
    P_now = H.unpack_rows(eng.pd_t[: eng.n], eng.m).T
    for c, (a, b) in enumerate(pairs):
        Tm, Im = sorted(set(T[a]) | set(T[b])), sorted(set(I[a]) | set(I[b]))
        P = np.zeros_like(X)
        for i in range(k):
            if i not in (a, b):
                P[np.ix_(T[i], I[i])] = True
        P[np.ix_(Tm, Im)] = True
        assert int((P & ~X).sum()) == fp_now + new_fp[c] and new_fp[c] == HP.dense_new_fp(X, P_now, Tm, Im)
        assert (nT[c], nI[c]) == (len(Tm), len(Im)) and (nTc[c], nIc[c]) == (len(set(T[a]) & set(T[b])), len(set(I[a]) & set(I[b])))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pybmf_amd.models import Hyper, HyperPlus
    assert issubclass(HyperPlus, Hyper)
    case = load_case("a")
    X = csr_matrix(case["X"].astype(np.float64))

    class Model(HyperPlus):
        def _make_engine(self):
            return numpy_engine(self)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="savings"):
            Model(model=hyper_of(case), target_k=1, savings="exclusive")
        with pytest.raises(NotImplementedError, match="reconstruction"):
            Model(model=hyper_of(case), target_k=1).fit(X, **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            HyperPlus(model=hyper_of(case), target_k=1).fit(case["X"].astype(np.float64) * 3, **FIT_KW)
        h = hyper_of(case)
        h.k = None
        with pytest.raises(TypeError, match="k is None"):
            Model(model=h, target_k=1).fit(X, **FIT_KW)
        h = hyper_of(case)
        h.T = h.T[:-1]
        with pytest.raises(ValueError, match="4 row sets and 5 column sets"):
            Model(model=h, target_k=1).fit(X, **FIT_KW)
        h = hyper_of(case)
        h.T, h.I = h.T[:-1], h.I[:-1]
        with pytest.raises(ValueError, match="its k is 5"):
            Model(model=h, target_k=1).fit(X, **FIT_KW)
        h = hyper_of(case)
        h.U = h.U[:, :4]
        with pytest.raises(ValueError, match="shapes"):
            Model(model=h, target_k=1).fit(X, **FIT_KW)
        with pytest.raises(ValueError, match="shapes"):
            Model(model=hyper_of(case), target_k=1).fit(csr_matrix(np.ones((41, 30))), **FIT_KW)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {"bmf_hyperplus_pairs": 12, "bmf_hyperplus_union": 9}


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
    off4, off8 = C.c_void_p(p16.value + 4), C.c_void_p(p16.value + 8)
    ok = (p16, p16, 4, p16, p16, 12, 16, 16, p16, 1, p16, None)

    def pairs(**kw):
        names = ("u_t", "v", "k", "x_t", "pd_t", "n", "ld", "ldv", "pair", "count", "rec", "stream")
        return lib.bmf_hyperplus_pairs(*[kw.get(name, value) for name, value in zip(names, ok)])
    for name in ("u_t", "v", "x_t", "pd_t", "pair", "rec"):
        assert pairs(**{name: None}) == -1 and b"null pointer" in lib.bmf_last_error()
    assert pairs(k=0) == -1 and pairs(n=0) == -1
    assert pairs(ld=18) == -1 and b"multiple" in lib.bmf_last_error()
    assert pairs(ldv=2) == -1 and b"multiple" in lib.bmf_last_error()
    assert pairs(n=513) == -1 and b"32 ldv" in lib.bmf_last_error()
    assert pairs(count=0) == -1 and b"count" in lib.bmf_last_error()
    assert pairs(count=(1 << 30) + 1) == -1 and b"count" in lib.bmf_last_error()
    for name in ("u_t", "v", "x_t", "pd_t"):
        assert pairs(**{name: off8}) == -1 and b"16-byte" in lib.bmf_last_error()
    assert pairs(rec=off4) == -1 and b"8-byte" in lib.bmf_last_error()
    assert pairs(pair=C.c_void_p(p16.value + 2)) == -1 and b"4-byte" in lib.bmf_last_error()
    assert lib.bmf_hyperplus_union(None, p16, 4, 16, 16, 0, 1, 0, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_hyperplus_union(p16, p16, 4, 18, 16, 0, 1, 0, None) == -1 and b"multiple" in lib.bmf_last_error()
    for a, b, dst in ((4, 1, 0), (0, -1, 0), (0, 1, 4), (0, 1, -1)):
        assert lib.bmf_hyperplus_union(p16, p16, 4, 16, 16, a, b, dst, None) == -1 and b"[0, k)" in lib.bmf_last_error()
    assert lib.bmf_hyperplus_union(p16, off8, 4, 16, 16, 0, 1, 0, None) == -1 and b"16-byte" in lib.bmf_last_error()
