"""Asso without a GPU: the model's host loop (models/Asso.py) on a NumPy stand-in that offers the calls of pybmf_amd.asso.AssoEngine
(build_basis / best / column / apply / remove / truncate / counts / row_counts / factor_arrays / prediction), against what the
reference produced (tests/golden/g24_asso.*, written by tests/golden/make_golden_asso.py).

The stand-in works on packed uint32 words in the engine's layout (row-major bit rows of n_pad / 32 words for X, the prediction and the
candidates) and restates a sweep on counts: a = |x_r & ~pd_r & b|, c = |~pd_r & b| - a per row and candidate, the reference's fp64
comparison on TP_old + a, FP_old + c, the integer sums T, F of the chosen side, score = w_fn T - w_fp F, and the candidate with the
largest score above best_score, the first of equals.  It is first held to the recorded get_vector sweeps; the real class on it must
then reproduce every case: integer columns equal, score / score_0.5 / desc_len equal (==) where the weights are dyadic (cases a-f),
the score within 1e-12 relative otherwise (case g: the reference adds per-row scores, the restatement multiplies the sums), the
metric columns within 1e-12 (ratios of equal integers: the slack is for the order of two divisions), U and V cell for cell.

Cases b, c and e end, in the reference, in a TypeError raised inside its own message stop (the fixture records that, and the state
as it stood); what is asserted there is that state with the stop done: the same log rows, U, V and prediction.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)
CASES = ["a", "b", "c", "d", "e", "f", "g"]
DYADIC = ["a", "b", "c", "d", "e", "f"]


def popcount_rows(words) -> np.ndarray:
    """Bits per row of a 2-D uint32 array."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return POP8[w.view(np.uint8)].reshape(w.shape[0], -1).sum(axis=1)


def pack_rows(B, words):
    """Rows of a 0 / 1 matrix as `words` uint32 words each, bit i of word i // 32, zero padded."""
    B = np.asarray(B).astype(bool)
    out = np.zeros((B.shape[0], words * 32), dtype=np.uint8)
    out[:, : B.shape[1]] = B
    return np.packbits(out, axis=1, bitorder="little").view(np.uint32).copy()


def unpack(words, length):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:length].astype(bool)


def basis_bits(Xt, m, n, ldx, tau):
    """What bmf_asso_basis returns: (candidate rows as packed words, bits per row), from the transposed packed bits of X."""
    Xb = np.unpackbits(Xt[:n].view(np.uint8), axis=1, bitorder="little")[:, :m].astype(np.int64)
    Cm = Xb @ Xb.T
    s = np.diag(Cm).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        on = (Cm.astype(np.float64) / s[:, None] > tau) & (s[:, None] > 0)
    B = pack_rows(on, ldx)
    return B, popcount_rows(B)


def score_block(X, PD, B, m, cands, tp_old, fp_old, w_fp, w_fn, best_score):
    """What bmf_asso_score + bmf_asso_pick return: (T, F, score, vectors) per candidate and the position of the largest score above
    best_score, the first of equals (-1: none)."""
    not_pd = ~PD[:m]
    xn = X[:m] & not_pd
    s_old = -w_fp * fp_old.astype(np.float64) + w_fn * tp_old.astype(np.float64)
    T, F = np.zeros(len(cands), dtype=np.int64), np.zeros(len(cands), dtype=np.int64)
    score, vectors = np.zeros(len(cands), dtype=np.float64), np.zeros((len(cands), m), dtype=bool)
    first, best = -1, float(best_score)
    for i, j in enumerate(cands):
        a = popcount_rows(xn & B[j])
        c = popcount_rows(not_pd & B[j]) - a
        tp_new, fp_new = tp_old + a, fp_old + c
        take = -w_fp * fp_new.astype(np.float64) + w_fn * tp_new.astype(np.float64) > s_old
        T[i], F[i] = int(np.where(take, tp_new, tp_old).sum()), int(np.where(take, fp_new, fp_old).sum())
        score[i] = w_fn * float(T[i]) - w_fp * float(F[i])
        vectors[i] = take
        if score[i] > best:
            first, best = i, score[i]
    return T, F, score, vectors, first


class NumpyAssoEngine:
    """pybmf_amd.asso.AssoEngine in NumPy, same layout (m_pad, n_pad multiples of 512), same interface."""

    def __init__(self, X, extra=None):
        X = np.asarray(X) != 0
        self.m, self.n = X.shape
        self.W, self.ldx = -(-max(self.m, 1) // 512) * 16, -(-self.n // 512) * 16
        self.m_pad = self.W * 32
        self.X = np.zeros((self.m_pad, self.ldx), dtype=np.uint32)
        self.X[: self.m] = pack_rows(X, self.ldx)
        self.Xt = pack_rows(X.T, self.W)
        self.pd = np.zeros_like(self.X)
        self.truth = {"train": self.X}
        for name, G in (extra or {}).items():
            self.truth[name] = np.zeros_like(self.X)
            self.truth[name][: self.m] = pack_rows(np.asarray(G) != 0, self.ldx)
        self.basis = np.zeros((self.n, self.ldx), dtype=np.uint32)
        self.list = np.zeros(0, dtype=np.int32)
        self._factors, self._weights, self.launches = [], None, 0

    @property
    def n_factors(self):
        return len(self._factors)

    def build_basis(self, tau):
        self.basis, count = basis_bits(self.Xt, self.m, self.n, self.ldx, tau)
        self.list = np.nonzero(count > 0)[0].astype(np.int32)
        return int(self.list.size)

    def basis_rows(self):
        return np.unpackbits(self.basis.view(np.uint8), axis=1, bitorder="little")[:, : self.n]

    def remove(self, cand):
        self.list = self.list[self.list != cand]

    def set_list(self, cands):
        self.list = np.ascontiguousarray(cands, dtype=np.int32)

    def row_counts(self):
        tp = popcount_rows(self.X[: self.m] & self.pd[: self.m])
        return tp, popcount_rows(self.pd[: self.m]) - tp

    def best(self, best_score, w_fp, w_fn, block=None):
        w_fp, w_fn, running = float(w_fp), float(w_fn), float(best_score)
        self._weights, self.launches = (w_fp, w_fn), 0
        total = int(self.list.size)
        if total == 0:
            return None
        tp_old, fp_old = self.row_counts()
        step = total if not block else int(block)
        hit = None
        for pos in range(0, total, step):
            cands = self.list[pos:pos + step]
            T, F, score, _, first = score_block(self.X, self.pd, self.basis, self.m, cands, tp_old, fp_old, w_fp, w_fn, running)
            self.launches += 1
            if first >= 0:
                running = float(score[first])
                hit = (pos + first, int(cands[first]), running, int(T[first]), int(F[first]))
        return hit

    def column(self, cand, w_fp=None, w_fn=None):
        if w_fp is None:
            w_fp, w_fn = self._weights
        tp_old, fp_old = self.row_counts()
        _, _, _, vectors, _ = score_block(self.X, self.pd, self.basis, self.m, [cand], tp_old, fp_old, float(w_fp), float(w_fn), 0.0)
        return pack_rows(vectors, self.W)[0], self.basis[cand].copy()

    def _or_in(self, u, v):
        rows = np.nonzero(unpack(u, self.m))[0]
        self.pd[rows] |= np.asarray(v, dtype=np.uint32)

    def apply(self, u, v):
        self._or_in(u, v)
        self._factors.append((np.array(u, dtype=np.uint32), np.array(v, dtype=np.uint32)))

    def load_prediction(self, X_pd):
        self.pd[: self.m] = pack_rows(X_pd, self.ldx)

    def truncate(self, k):
        self._factors = self._factors[:k]
        self.pd[:] = 0
        for u, v in self._factors:
            self._or_in(u, v)

    def counts(self, name="train"):
        G = self.truth[name]
        tp, n_pd, n_gt = int(popcount_rows(self.pd & G).sum()), int(popcount_rows(self.pd).sum()), int(popcount_rows(G).sum())
        return tp, n_pd - tp, n_gt - tp, self.m * self.n - n_pd - (n_gt - tp)

    def factor_arrays(self):
        U = np.array([unpack(u, self.m) for u, _ in self._factors], dtype=np.uint8).reshape(len(self._factors), self.m).T
        V = np.array([unpack(v, self.n) for _, v in self._factors], dtype=np.uint8).reshape(len(self._factors), self.n).T
        return U, V

    def prediction(self):
        rows = np.unpackbits(self.pd[: self.m].view(np.uint8), axis=1, bitorder="little")[:, : self.n]
        return csr_matrix(rows.astype(int))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g24_asso.json")))
    z = np.load(os.path.join(GOLDEN, "g24_asso.npz"))
    c = dict(meta["cases"][name])
    m = c["shape"][0]
    for key in ("X", "U", "V", "X_pd", "X_val", "X_test", "basis", "kept"):
        if f"{name}_{key}" in z.files:
            c[key] = z[f"{name}_{key}"]
    for i, p in enumerate(c["points"]):
        for key in ("list", "s_old", "scores"):
            p[key] = z[f"{name}_p{i}_{key}"]
        p["X_pd"] = np.unpackbits(z[f"{name}_p{i}_X_pd"], axis=1, bitorder="little")[:, : c["shape"][1]]
        p["vectors"] = np.unpackbits(z[f"{name}_p{i}_vectors"], axis=1, bitorder="little")[:, :m]
    c["weights"] = (c.get("w_fp", 0.5), 1 - c.get("w_fp", 0.5) if c.get("w_fn") is None else c["w_fn"])
    return c


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyAssoEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, engine_factory=None, block=None):
    """The real class on case's matrices; engine_factory(model) replaces the device engine."""
    from pybmf_amd.models import Asso

    class Model(Asso):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(tau=case["tau"], k=case["k"], tol=case["tol"], w_fp=case.get("w_fp", 0.5), w_fn=case.get("w_fn"))
        model.fit(sp("X"), sp("X_val"), sp("X_test"), **dict(FIT_KW, block=block))
    return model


def log_rows(model):
    """[[k, score, score_0.5, desc_len, |u|, |v|, metrics ...]] of logs['updates'] (time stamp dropped, the shape cell flattened)."""
    if "updates" not in model.logs:
        return []
    return [[r[1], r[2], r[3], r[4], r[5][0], r[5][1]] + list(r[6:]) for r in model.logs["updates"].values.tolist()]


def recount(X, X_pd, w_fp, w_fn):
    """Per-row TP, FP of a dense prediction, independent of the packed code."""
    X, X_pd = X.astype(np.int64), X_pd.astype(np.int64)
    return (X * X_pd).sum(axis=1), ((1 - X) * X_pd).sum(axis=1)


def expected_sweep(case, p):
    """(T, F) per candidate of a recorded sweep, recounted from the recorded vectors on dense matrices."""
    T, F = [], []
    for i, j in enumerate(p["list"]):
        new = p["X_pd"] | (p["vectors"][i][:, None] & case["basis"][j][None, :])
        tp, fp = recount(case["X"], new, *case["weights"])
        T.append(int(tp.sum()))
        F.append(int(fp.sum()))
    return np.array(T), np.array(F)


def engine_at_point(engine_cls, case, p):
    eng = engine_cls(case["X"])
    assert eng.build_basis(case["tau"]) == len(case["kept"])
    eng.load_prediction(p["X_pd"])
    eng.set_list(p["list"])
    return eng


def check_fit(model, case, exact_score=True):
    got, want, cols = log_rows(model), case["log"]["rows"], case["log"]["columns"]
    eng = model._engine
    assert len(got) == len(want)
    m, n = case["shape"]
    if not want:            # case e: no candidate at all; the stop leaves zero factors
        assert model.U.shape == (m, 0) and model.V.shape == (n, 0)
        assert eng.counts("train") == (0, 0, int(case["X"].sum()), case["X"].size - int(case["X"].sum()))
        assert model.X_pd.nnz == 0
        return
    head = ["k", "train/score", "train/score_0.5", "train/desc_len", "train/n_u", "train/n_v"]
    assert cols[:6] == head
    for g, w in zip(got, want):
        assert [int(g[0]), int(g[4]), int(g[5])] == [w[0], w[4], w[5]]
        if exact_score:
            assert float(g[1]) == w[1]
        else:
            assert abs(float(g[1]) - w[1]) <= 1e-12 * abs(w[1])
        assert float(g[2]) == w[2] and float(g[3]) == w[3]
        for name, gv, wv in zip(cols[6:], g[6:], w[6:]):
            if name.split("/")[1] in ("TP", "FP", "FN"):
                assert isinstance(gv, (int, np.integer)) and int(gv) == wv, name
    G, Wt = np.array([r[6:] for r in got], dtype=np.float64), np.array([r[6:] for r in want])
    assert G.shape == Wt.shape and np.abs(G - Wt).max() <= 1e-12
    U, V = np.asarray(model.U.todense()), np.asarray(model.V.todense())
    assert U.shape == case["U"].shape and V.shape == case["V"].shape
    assert (U != 0).tolist() == (case["U"] != 0).tolist() and (V != 0).tolist() == (case["V"] != 0).tolist()
    assert list(eng.counts("train")) == case["counts"]
    X_pd = np.asarray(model.X_pd.todense())
    assert (X_pd != 0).tolist() == (case["X_pd"] != 0).tolist()
    Ue, Ve = eng.factor_arrays()     # the engine's factors are U, V
    assert (Ue != 0).tolist() == (U != 0).tolist() and (Ve != 0).tolist() == (V != 0).tolist()
    assert eng.list.tolist() == [j for j in case["kept"].tolist() if j not in case["winners"]]


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stand_in_builds_the_recorded_candidates(name):
    case = load_case(name)
    eng = NumpyAssoEngine(case["X"])
    assert eng.build_basis(case["tau"]) == len(case["kept"])
    assert eng.list.tolist() == case["kept"].tolist()
    assert eng.basis_rows().tolist() == case["basis"].tolist()
    assert popcount_rows(eng.basis).sum() == int(case["basis"].sum())      # padding bits stay zero


@pytest.mark.parametrize("name", ["a", "b"])
def test_stand_in_matches_get_vector_at_the_recorded_sweeps(name):
    case = load_case(name)
    w_fp, w_fn = case["weights"]
    assert len(case["points"]) == 2 and case["points"][1]["index"] > 0
    for p in case["points"]:
        eng = engine_at_point(NumpyAssoEngine, case, p)
        tp_old, fp_old = eng.row_counts()
        want_tp, want_fp = recount(case["X"], p["X_pd"], w_fp, w_fn)
        assert tp_old.tolist() == want_tp.tolist() and fp_old.tolist() == want_fp.tolist()
        assert (-w_fp * fp_old.astype(np.float64) + w_fn * tp_old.astype(np.float64)).tolist() == p["s_old"].tolist()
        T, F, score, vectors, first = score_block(eng.X, eng.pd, eng.basis, eng.m, p["list"], tp_old, fp_old, w_fp, w_fn, p["best_score"])
        want_T, want_F = expected_sweep(case, p)
        assert T.tolist() == want_T.tolist() and F.tolist() == want_F.tolist()
        assert vectors.tolist() == (p["vectors"] != 0).tolist()
        assert score.tolist() == p["scores"].tolist()          # dyadic weights: bit-equal
        assert first == p["winner"]
        for block in (None, 1, 7):
            hit = eng.best(p["best_score"], w_fp, w_fn, block=block)
            assert hit == (first, int(p["list"][first]), float(score[first]), int(T[first]), int(F[first]))
            assert eng.launches == (1 if block is None else -(-len(p["list"]) // block))
        u, v = eng.column(hit[1])
        assert unpack(u, eng.m).tolist() == (p["vectors"][first] != 0).tolist() and unpack(v, eng.n).tolist() == (case["basis"][hit[1]] != 0).tolist()


@pytest.mark.parametrize("name", CASES)
def test_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    model = fit_case(case, numpy_engine)
    check_fit(model, case, exact_score=name in DYADIC)
    rows = case["log"]["rows"]
    if name in ("a", "d", "f", "g"):      # "Reach requested factor" keeps all k factors
        assert len(rows) == case["k"] == model.U.shape[1] and case["raised"] is None
    if name == "b":      # error <= tol: the factor added last is dropped from U, V and from the prediction; the fit goes on and finds nothing
        err = case["log"]["columns"].index("train/ERR")
        assert rows[-1][err] <= case["tol"] < rows[-2][err]
        assert model.U.shape[1] == len(rows) - 1 and case["n_sweeps"] == len(rows) + 1 and case["raised"] == "TypeError"
    if name == "c":      # runs until no candidate improves the inherited score
        assert model.U.shape[1] == len(rows) and case["winners"][-1] == -1 and case["raised"] == "TypeError"
    if name == "d":
        assert [c.split("/")[0] for c in case["log"]["columns"][6:]] == ["train"] * 11 + ["val"] * 11 + ["test"] * 11
    if name == "g":
        assert min(case["margins"]) > 1e-9
    scores = [r[1] for r in rows]
    assert all(b > a for a, b in zip(scores, scores[1:]))


@pytest.mark.parametrize("name", ["a", "c", "d", "g"])
def test_block_size_does_not_change_the_result(name):
    case = load_case(name)
    ref = fit_case(case, numpy_engine)
    for block in (1, 7):
        model = fit_case(case, numpy_engine, block=block)
        assert log_rows(model) == log_rows(ref)
        assert (model.U != ref.U).nnz == 0 and (model.V != ref.V).nnz == 0
        check_fit(model, case, exact_score=name in DYADIC)


def test_new_metric_keys_leave_the_old_ones_alone():
    from pybmf_amd.models import ContinuousModel
    old = ["TP", "FP", "FN", "TN", "Recall", "Precision", "Accuracy", "F1", "TPR", "PPV", "ACC"]
    counts = (30, 5, 10, 55)
    vals = dict(zip(old + ["FPR", "FNR", "ERR"], ContinuousModel._metric_values(old + ["FPR", "FNR", "ERR"], None, counts)))
    assert vals["FPR"] == 1 - 55 / 60 and vals["FNR"] == 1 - 30 / 40 and vals["ERR"] == 1 - 85 / 100
    assert [vals[k] for k in old[:4]] == [30, 5, 10, 55] and vals["Recall"] == 30 / 40 and vals["Precision"] == 30 / 35
    assert ContinuousModel._metric_values(["FPR"], None, (0, 0, 3, 0)) == [1]      # no negative cell: TNR counts as 0


def test_refusals():
    from pybmf_amd.models import Asso
    case = load_case("a")
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match="reconstruction"):
            Asso(tau=0.4, k=2).fit(csr_matrix(case["X"].astype(np.float64)), **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="basis_dim"):
            Asso(tau=0.4, k=2).fit(csr_matrix(case["X"].astype(np.float64)), **dict(FIT_KW, basis_dim=0))
        with pytest.raises(NotImplementedError, match="Boolean"):
            Asso(tau=0.4, k=2).fit(case["X"].astype(np.float64) * 3, **FIT_KW)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {
    "bmf_asso_basis": 8, "bmf_asso_score_work": 2, "bmf_asso_score": 14, "bmf_asso_pick": 12, "bmf_asso_column": 13, "bmf_asso_apply": 6,
}


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
        assert len(args) == n_args and res is (L._i64 if name.endswith("_work") else C.c_int)
    assert L.lib.bmf_version() == 501


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    assert lib.bmf_asso_score_work(0, 4) == -1 and lib.bmf_asso_score_work(4, 0) == -1
    assert lib.bmf_asso_score_work(65, 10) == 2 * 10 * 16
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert lib.bmf_asso_basis(None, 4, 16, 0.5, p, 16, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_asso_basis(p, 0, 16, 0.5, p, 16, p, None) == -1
    assert lib.bmf_asso_basis(p, 4, 12, 0.5, p, 16, p, None) == -1 and b"multiple of 16" in lib.bmf_last_error()
    assert lib.bmf_asso_basis(p, 600, 16, 0.5, p, 16, p, None) == -1          # ldb * 32 < n
    assert lib.bmf_asso_basis(p, 4, 16, float("nan"), p, 16, p, None) == -1
    assert lib.bmf_asso_score(p, p, p, 16, 4, 4, p, 1, p, None, 0.5, 0.5, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_asso_score(p, p, p, 24, 4, 4, p, 1, p, p, 0.5, 0.5, p, None) == -1 and b"multiple of 16" in lib.bmf_last_error()
    assert lib.bmf_asso_score(p, p, p, 16, 4, 4, p, 0, p, p, 0.5, 0.5, p, None) == -1
    assert lib.bmf_asso_score(p, p, p, 16, 4, 4, p, 1, p, p, float("nan"), 0.5, p, None) == -1
    assert lib.bmf_asso_score(p, p, p, 16, 4, 4, p, 1, p, p, 0.5, 0.5, C.c_void_p(p.value + 4), None) == -1
    assert lib.bmf_asso_pick(p, 4, p, 1, 0.0, 0.5, 0.5, p, p, None, p, None) == -1
    assert lib.bmf_asso_pick(p, 4, p, 0, 0.0, 0.5, 0.5, p, p, p, p, None) == -1
    assert lib.bmf_asso_column(p, p, p, 16, 0, p, p, 0.5, 0.5, p, p, p, None) == -1
    assert lib.bmf_asso_column(p, p, None, 16, 4, p, p, 0.5, 0.5, p, p, p, None) == -1
    assert lib.bmf_asso_apply(p, 16, 4, p, None, None) == -1
    assert lib.bmf_asso_apply(p, 0, 4, p, p, None) == -1
