"""Panda without a GPU: the model's host loop (models/Panda.py) on a NumPy stand-in that offers the calls of
pybmf_amd.panda.PatternEngine, against what the reference produced (tests/golden/g28_panda.*, written by
tests/golden/make_golden_panda.py).

The stand-in works on packed uint32 words in the engine's layout (both orientations, m_pad and n_pad multiples of 512); its four
step functions (couples_scores, core_scan, ext_scan, rows_pass) are what the kernels of csrc/panda.hip are compared with on the
device (tests/test_panda_gpu.py).  (i) The real class on it must reproduce every recorded fit -- recorded from the reference with a
stable argsort, the tie rule this build defines: the integers of every log row equal, `cost` equal (== when all three weights are
exact in the sense of boolean_family.exact_weights, 1e-12 relative otherwise), the metric columns to 1e-12 (ratios of equal integers),
U, V and the counts cell for cell, and for cases b, c, d the (T, I, E, cost_now) after every find_core and extend_core.  Where the
reference ends in the TypeError of its own early_stop (cases d, f, h, j) the rows and factors up to there are what is compared: the
stop itself is meant to leave them.  (ii) At sort_items calls recorded from the reference as shipped (NumPy's default argsort), the
defined order and the shipped order agree once the scores are mapped through them: they differ only inside tie groups.
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

from boolean_family import exact_weights
from test_grecond_cpu import pack_rows, popcount, unpack
from test_mebf_cpu import check_cost, row_popcounts, unpack_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
CASES = ["a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k"]
STEP_CASES = ["b", "c", "d"]


def order_of(scores):
    """The defined order: score descending, among equal scores the later position first."""
    return np.flip(np.argsort(np.asarray(scores), kind="stable"))


# ---- the four device steps on packed words ------------------------------------------------------------------------------------
def couples_scores(rs_t, n, rowcount):
    """score[c] = the sum of rowcount over the set bits of bit row c of rs_t, minus |rs_t[c]| (bmf_panda_couples)."""
    out = np.zeros(n, dtype=np.int64)
    for c in range(n):
        rows = np.nonzero(unpack(rs_t[c], len(rowcount)))[0]
        out[c] = int(np.asarray(rowcount, dtype=np.int64)[rows].sum()) - popcount(rs_t[c])
    return out


def core_d_cost(w_model, w_fn, w0, h0, h1):
    w0, h0, h1 = np.float64(w0), np.float64(h0), np.asarray(h1, dtype=np.float64)
    w1 = w0 + 1
    return np.float64(w_model) * ((w1 + h1) - (w0 + h0)) - np.float64(w_fn) * ((w1 * h1) - (w0 * h0))


def core_scan(rs_t, T, cands, mode, w_model, w_fn, w0, h0):
    """(h1 per candidate, winner position or -1, pick position): bmf_panda_core_scan.  mode 0: the first candidate in list order
    with d_cost <= 0.  mode 1: the pick is the highest h1, among equals the last position; it wins iff its d_cost <= 0."""
    h1 = row_popcounts(rs_t[np.asarray(cands, dtype=np.int64)] & T)
    ok = core_d_cost(w_model, w_fn, w0, h0, h1) <= 0
    if mode == 0:
        hit = np.nonzero(ok)[0]
        win = int(hit[0]) if hit.size else -1
        return h1, win, win
    pick = int(order_of(h1)[0])
    return h1, (pick if ok[pick] else -1), pick


def ext_scan(rs_t, pd_t, T, cands, n_t, w_model, w_fp, w_fn, cost_old):
    """(a, b per candidate, winner position or -1): bmf_panda_ext_scan; the first candidate with cost_new <= cost_old."""
    cands = np.asarray(cands, dtype=np.int64)
    a, b = row_popcounts(rs_t[cands] & T), row_popcounts(pd_t[cands] & T)
    partial_fn = -a.astype(np.float64)
    partial_fp = np.float64(n_t) - b.astype(np.float64) + partial_fn
    cost_new = np.float64(cost_old) + np.float64(w_model) * 1 + np.float64(w_fp) * partial_fp + np.float64(w_fn) * partial_fn
    hit = np.nonzero(cost_new <= np.float64(cost_old))[0]
    return a, b, (int(hit[0]) if hit.size else -1)


def rows_pass(rs, pd, m, I, n_i, T, w_model, w_fp, w_fn):
    """(T with the rows that join, their number, sum of d_fn, sum of d_fp): bmf_panda_rows for the item set I of n_i items."""
    p, q = row_popcounts(rs[:m] & I), row_popcounts(pd[:m] & I)
    d_fn = -p
    d_fp = n_i - q + d_fn
    d = np.float64(w_model) * 1 + (np.float64(w_fn) * d_fn.astype(np.float64) + np.float64(w_fp) * d_fp.astype(np.float64))
    join = (d <= 0) & ~unpack(T, m)
    return T | pack_rows(join[None, :], T.size)[0], int(join.sum()), int(d_fn[join].sum()), int(d_fp[join].sum())


class NumpyPatternEngine:
    """pybmf_amd.panda.PatternEngine in NumPy, same layout, same interface.  Index 0 = transposed bit matrices, 1 = row-major."""

    def __init__(self, X, extra=None):
        X = np.asarray(X) != 0
        self.m, self.n = X.shape
        self.W, self.nvw = -(-max(self.m, 1) // 512) * 16, -(-self.n // 512) * 16
        self.x = [pack_rows(X.T, self.W), pack_rows(X, self.nvw)]
        self.sum_x = int(X.sum())
        self.truth = {"train": self.x[0]}
        for name, G in (extra or {}).items():
            self.truth[name] = pack_rows((np.asarray(G) != 0).T, self.W)
        self.rs, self.pd = [self.x[0].copy(), self.x[1].copy()], [np.zeros_like(self.x[0]), np.zeros_like(self.x[1])]
        self.T, self.I = np.zeros(self.W, dtype=np.uint32), np.zeros(self.nvw, dtype=np.uint32)
        self.cand, self.factors, self.reads = np.zeros(0, dtype=np.int32), [], 0

    def scores(self, method):
        self.reads += 1
        if method == "frequency":
            return row_popcounts(self.rs[0][: self.n])
        return couples_scores(self.rs[0], self.n, row_popcounts(self.rs[1][: self.m]))

    def start_core(self, col):
        self.T = self.rs[0][col].copy()
        return popcount(self.T)

    def set_candidates(self, E):
        self.cand = np.asarray(E, dtype=np.int32).copy()

    def core_scan(self, pos, count, mode, w_model, w_fn, w0, h0, want_scores=False):
        h1, win, _ = core_scan(self.rs[0], self.T, self.cand[pos:pos + count], mode, w_model, w_fn, w0, h0)
        self.reads += 1
        if win >= 0:
            self.T = self.T & self.rs[0][self.cand[pos + win]]
        return win, (int(h1[win]) if win >= 0 else 0), (h1.astype(np.int64) if want_scores else None)

    def set_items(self, I):
        self.I = pack_rows(np.isin(np.arange(self.n), I)[None, :], self.nvw)[0]

    def ext_scan(self, pos, count, n_t, n_i, w_model, w_fp, w_fn, cost_old):
        a, b, win = ext_scan(self.rs[0], self.pd[0], self.T, self.cand[pos:pos + count], n_t, w_model, w_fp, w_fn, cost_old)
        self.reads += 1
        if win < 0:
            return dict(i=-1, a=0, b=0, added=0, sum_d_fn=0, sum_d_fp=0)
        col = int(self.cand[pos + win])
        self.I[col >> 5] |= np.uint32(1 << (col & 31))
        self.T, added, s_fn, s_fp = rows_pass(self.rs[1], self.pd[1], self.m, self.I, n_i, self.T, w_model, w_fp, w_fn)
        return dict(i=win, a=int(a[win]), b=int(b[win]), added=added, sum_d_fn=s_fn, sum_d_fp=s_fp)

    def core_rows(self):
        return self.T.copy()

    def apply_core(self):
        u, v = self.T.copy(), self.I.copy()
        cols, rows = np.nonzero(unpack(v, self.n))[0], np.nonzero(unpack(u, self.m))[0]
        self.rs[0][cols] &= ~u
        self.pd[0][cols] |= u
        self.rs[1][rows] &= ~v
        self.pd[1][rows] |= v
        self.factors.append((u, v))
        return u, v

    def factor_cells(self):
        return sum(popcount(u) + popcount(v) for u, v in self.factors)

    def residual_sum(self):
        return popcount(self.rs[0])

    def error_counts(self):
        return popcount(self.pd[0] & ~self.x[0]), popcount(self.x[0] & ~self.pd[0])

    def counts(self, name="train"):
        G, pd = self.truth[name], self.pd[0]
        tp, n_pd, n_gt = popcount(pd & G), popcount(pd), popcount(G)
        return tp, n_pd - tp, n_gt - tp, self.m * self.n - n_pd - (n_gt - tp)

    def factor_arrays(self):
        fs = self.factors
        U = np.array([unpack(u, self.m) for u, _ in fs], dtype=np.uint8).reshape(len(fs), self.m).T
        V = np.array([unpack(v, self.n) for _, v in fs], dtype=np.uint8).reshape(len(fs), self.n).T
        return U, V

    def prediction(self):
        return csr_matrix(unpack_matrix(self.pd[1], self.m, self.n).astype(int))

    def bit_matrices(self):
        return self.rs[0], self.pd[0], self.rs[1], self.pd[1]


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_meta():
    return json.load(open(os.path.join(GOLDEN, "g28_panda.json")))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, "g28_panda.npz"))
    c = dict(load_meta()["cases"][name])
    for key in ("X", "U", "V", "X_val", "X_test", "steps_T", "steps_I", "steps_E"):
        if f"{name}_{key}" in z.files:
            c[key] = z[f"{name}_{key}"]
    return c


def load_points(name):
    z = np.load(os.path.join(GOLDEN, "g28_panda.npz"))
    c = dict(load_meta()["shipped"][name])
    for i, p in enumerate(c["points"]):
        for key in ("X_rs", "T", "before", "after"):
            p[key] = z[f"s{name}_p{i}_{key}"]
    return c


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyPatternEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, engine_factory=None, block=None, record=False):
    """The real class on case's matrices; engine_factory(model) replaces the device engine.  record: model.steps keeps
    (stage, T, I, E, cost_now) after every find_core / extend_core."""
    from pybmf_amd.models import Panda

    class Model(Panda):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

        def _snap(self, stage):
            if record:
                self.steps.append((stage, unpack(self._engine.core_rows(), self.m), sorted(self.I), list(self.E), float(self.cost_now)))

        def find_core(self):
            super().find_core()
            self._snap("core")

        def extend_core(self):
            super().extend_core()
            self._snap("ext")

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(**{key: case[key] for key in ("k", "tol", "w_model", "w_fp", "w_fn", "init_method", "exact_decomp")})
        model.steps = []
        model.fit(sp("X"), sp("X_val"), sp("X_test"), **dict(FIT_KW, block=block))
    return model


def log_rows(model):
    """[[cost, |T|, |I|, metrics ...]] of logs['updates'] (time stamp dropped, the shape cell flattened)."""
    if "updates" not in model.logs:
        return []
    return [[r[1], r[2][0], r[2][1]] + [float(x) for x in r[3:]] for r in model.logs["updates"].values.tolist()]


def all_exact(case):
    """All three weights are 0, 0.5 or 1, the values of boolean_family.exact_weights: their products with counts and the sums are exact."""
    assert exact_weights(0.5, 0.5) and exact_weights(1.0, 1.0) and exact_weights(0.0, 1.0)
    return all(float(case[w]) in (0.0, 0.5, 1.0) for w in ("w_model", "w_fp", "w_fn"))


def check_fit(model, case):
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want)
    exact = all_exact(case)
    if want:
        assert case["log"]["columns"][:3] == ["cost", "n_u", "n_v"]
    for g, w in zip(got, want):
        check_cost(float(g[0]), w[0], exact)
        assert all(isinstance(x, (int, np.integer)) for x in g[1:3]) and [int(x) for x in g[1:3]] == w[1:3]
        assert len(g) == len(w) and np.abs(np.array(g[3:]) - np.array(w[3:])).max() <= 1e-12
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    f = case["U"].shape[1]
    if case["raised"]:       # the fixture keeps the factors up to the stop; the stop here truncates to them
        assert U.shape[1] == f == len(want)
    assert U.shape == (case["shape"][0], f) and V.shape == (case["shape"][1], f)
    assert U.tolist() == (case["U"] != 0).tolist() and V.tolist() == (case["V"] != 0).tolist()
    eng = model._engine
    assert list(eng.counts("train")) == case["counts"]
    X_pd, X = np.asarray(model.X_pd.todense()), case["X"]
    assert [int((X_pd & X).sum()), int((X_pd & (1 - X)).sum())] == case["counts"][:2]
    assert eng.residual_sum() == case["counts"][2]


def check_steps(model, case):
    want = case["steps"]
    assert len(model.steps) >= len(want) > 0       # (the run here goes on past the reference's TypeError to its own stop: one more factor's steps)
    exact = all_exact(case)
    for i, (got, w) in enumerate(zip(model.steps, want)):
        stage, T, I, E, cost = got
        assert stage == w["stage"], i
        assert T.tolist() == (case["steps_T"][i] != 0).tolist(), (i, stage)
        assert I == np.nonzero(case["steps_I"][i])[0].tolist(), (i, stage)
        assert E == [int(e) for e in case["steps_E"][i] if e >= 0], (i, stage)
        check_cost(cost, w["cost"], exact)


def check_state(eng, X):
    """Both orientations are transposes of each other, the residual is X & ~X_pd, nothing is set in the padding."""
    m, n = X.shape
    rs_t, pd_t, rs, pd = eng.bit_matrices()
    R, P = unpack_matrix(rs, m, n), unpack_matrix(pd, m, n)
    assert (unpack_matrix(rs_t, n, m) == R.T).all() and (unpack_matrix(pd_t, n, m) == P.T).all()
    assert (R == ((X != 0) & ~P)).all()
    for M, want in ((rs, R), (rs_t, R), (pd, P), (pd_t, P)):
        assert popcount(M) == int(want.sum())
    assert eng.residual_sum() == int(R.sum())
    return R, P


def description_length(X, U, V, w_model, w_fp, w_fn):
    """w_model (|U| + |V|) + w_fp FP + w_fn FN of the Boolean product, recounted densely."""
    Xb = np.asarray(X) != 0
    P = (np.asarray(U).astype(np.int64) @ np.asarray(V).astype(np.int64).T) > 0
    return w_model * np.float64(int(np.asarray(U).sum()) + int(np.asarray(V).sum())) + w_fp * np.float64(int((P & ~Xb).sum())) \
        + w_fn * np.float64(int((Xb & ~P).sum()))


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    model = fit_case(case, numpy_engine, record=name in STEP_CASES)
    check_fit(model, case)
    check_state(model._engine, case["X"])
    rows = case["log"]["rows"]
    if name in STEP_CASES:
        check_steps(model, case)
    if name in ("a", "b", "c", "k"):     # early_stop sees n_factors before it is incremented: k = 5 yields 6
        assert len(rows) == case["k"] + 1 == model.U.shape[1] and not case["raised"]
    if name == "e":
        assert case["exact_decomp"] and len(rows) == case["k"] + 1 and case["counts"][1] == 0        # cores only: no false positive
    if name in ("d", "f", "h", "j"):
        assert case["raised"] == "TypeError"
    if name == "d":
        assert len(rows) == 40
    if name == "f":
        assert len(rows) == 17 and sum(r[1] == 1 for r in rows) >= 5
    if name == "g":                      # error <= tol = 0 at the last factor: dropped from U, V, still in X_pd and the log
        assert len(rows) == 4 and model.U.shape[1] == 3 and model._engine.residual_sum() == 0
    if name == "j":
        assert rows == [] and model.U.shape[1] == 0
    if name == "k":
        assert [c.split("/")[0] for c in case["log"]["columns"][3:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4


@pytest.mark.parametrize("name", ["b", "c", "g", "i"])
def test_block_size_changes_nothing(name):
    case = load_case(name)
    for block in (1, 7):
        model = fit_case(case, numpy_engine, block=block)
        check_fit(model, case)


@pytest.mark.parametrize("name", ["a", "c", "i"])
def test_logged_cost_is_the_description_length_of_the_factors_so_far(name):
    case = load_case(name)
    model = fit_case(case, numpy_engine)
    U, V = model._engine.factor_arrays()
    for f, row in enumerate(log_rows(model)):
        want = description_length(case["X"], U[:, :f + 1], V[:, :f + 1], case["w_model"], case["w_fp"], case["w_fn"])
        check_cost(float(row[0]), float(want), all_exact(case))


@pytest.mark.parametrize("name", ["a", "c"])
def test_shipped_order_differs_only_inside_tie_groups(name):
    case = load_points(name)
    assert len(case["points"]) == 3
    for p in case["points"]:
        R = p["X_rs"] != 0
        eng = NumpyPatternEngine(R)                # (its residual is the recorded one: nothing is applied)
        if p["method"] == "correlation":
            T = pack_rows((p["T"] != 0)[None, :], eng.W)[0]
            scores = row_popcounts(eng.rs[0][: eng.n] & T)
            assert scores.tolist() == R[p["T"] != 0].sum(axis=0).tolist()
        else:
            scores = eng.scores(p["method"])
            if p["method"] == "couples-frequency":
                Ri = R.astype(np.int64)
                assert scores.tolist() == ((Ri.sum(axis=1) @ Ri) - Ri.sum(axis=0)).tolist()
        before, after = p["before"].astype(np.int64), p["after"].astype(np.int64)
        defined = before[order_of(scores[before])]
        assert sorted(after.tolist()) == sorted(before.tolist())
        assert scores[defined].tolist() == scores[after].tolist()
        assert all(a >= b for a, b in zip(scores[defined], scores[defined][1:]))


def test_tie_rule_on_a_hand_made_list():
    #                     pos: 0  1  2  3  4  5
    E, s = np.array([7, 2, 9, 4, 0, 5]), np.array([3, 5, 3, 5, 1, 3])
    once = E[order_of(s)]
    assert once.tolist() == [4, 2, 5, 9, 7, 0]            # 5s: the later position first; then the 3s the same way; then the 1
    twice = once[order_of(s[order_of(s)])]
    assert twice.tolist() == [2, 4, 7, 9, 5, 0]           # the same scores again: every tie group reversed
    # the correlation pick: the highest score, among equals the last position
    X = np.zeros((6, 4), dtype=np.uint8)
    X[:4, 0], X[:3, 1], X[1:4, 2], X[:2, 3] = 1, 1, 1, 1
    eng = NumpyPatternEngine(X)
    T = eng.rs[0][0]
    h1, win, pick = core_scan(eng.rs[0], T, [1, 2, 3], 1, 1, 1, 1, 4)
    assert h1.tolist() == [3, 3, 2] and pick == 1 and win == 1      # d_cost = (2 + 3 - 5) - (6 - 4) = -2
    h1, win, pick = core_scan(eng.rs[0], T, [2, 1, 3], 0, 1, 1, 1, 4)
    assert win == 0 == pick


def test_decisions_at_the_kinks():
    # core: w_model = w_fn = 1, w0 = 1, h0 = 2: h1 = 1 gives d_cost == 0 (accept), h1 = 0 gives 1 (reject)
    assert core_d_cost(1, 1, 1, 2, 1) == 0 and core_d_cost(1, 1, 1, 2, 0) == 1
    # extension column: weights 1, |T| = 3, b = 0: a = 2 gives cost_new == cost_old (accept), a = 1 gives + 2
    X = np.zeros((5, 3), dtype=np.uint8)
    X[:3, 0], X[:2, 1], X[:1, 2] = 1, 1, 1
    eng = NumpyPatternEngine(X)
    T = eng.rs[0][0]
    a, b, win = ext_scan(eng.rs[0], eng.pd[0], T, [2, 1], 3, 1, 1, 1, 10.0)
    assert a.tolist() == [1, 2] and b.tolist() == [0, 0] and win == 1
    # row rule: weights 1, |I| = 3, no prediction bits: two residual bits give d == 0 (joins), one gives 2
    R = np.zeros((4, 3), dtype=np.uint8)
    R[0], R[1, :2], R[2, :1] = 1, 1, 1
    eng = NumpyPatternEngine(R)
    I = pack_rows(np.ones((1, 3), dtype=bool), eng.nvw)[0]
    T0 = pack_rows(np.array([[1, 0, 0, 0]], dtype=bool), eng.W)[0]
    T1, added, s_fn, s_fp = rows_pass(eng.rs[1], eng.pd[1], 4, I, 3, T0, 1, 1, 1)
    assert unpack(T1, 4).tolist() == [True, True, False, False] and (added, s_fn, s_fp) == (1, -2, 1)


def test_refusals():
    from pybmf_amd.models import Panda
    case = load_case("a")
    X = csr_matrix(case["X"].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(AssertionError):
            Panda(k=2, init_method="random")
        with pytest.raises(NotImplementedError, match="reconstruction"):
            Panda(k=2).fit(X, **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            Panda(k=2).fit(case["X"].astype(np.float64) * 3, **FIT_KW)
        model = Panda(k=2, w_model=3, init_method="correlation", exact_decomp=True)
    assert model.w_model == 0 and model.init_method == "frequency"


def test_stops_with_a_message_leave_the_factors_found_so_far():
    for name in ("d", "f", "h", "j"):
        case = load_case(name)
        model = fit_case(case, numpy_engine)
        assert model.U.shape[1] == model.V.shape[1] == len(case["log"]["rows"])


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {"bmf_panda_couples": 7, "bmf_panda_core_scan": 14, "bmf_panda_close": 7, "bmf_panda_ext_scan": 16,
                    "bmf_panda_rows_work": 1, "bmf_panda_rows": 17}


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


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    assert lib.bmf_panda_rows_work(0) == -1 and lib.bmf_panda_rows_work(10) == 120
    assert lib.bmf_panda_couples(None, 4, 16, p, 8, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_panda_couples(p, 0, 16, p, 8, p, None) == -1
    assert lib.bmf_panda_couples(p, 4, 16, p, 513, p, None) == -1 and b"32 * ld" in lib.bmf_last_error()
    assert lib.bmf_panda_core_scan(p, 4, 16, p, p, 0, 0, 1.0, 1.0, 1, 2, None, p, None) == -1
    assert lib.bmf_panda_core_scan(p, 4, 16, p, p, 2, 2, 1.0, 1.0, 1, 2, p, p, None) == -1 and b"mode" in lib.bmf_last_error()
    assert lib.bmf_panda_core_scan(p, 4, 18, p, p, 2, 0, 1.0, 1.0, 1, 2, p, p, None) == -1 and b"multiple of 4" in lib.bmf_last_error()
    assert lib.bmf_panda_core_scan(p, 4, 16, odd, p, 2, 0, 1.0, 1.0, 1, 2, p, p, None) == -1 and b"aligned" in lib.bmf_last_error()
    assert lib.bmf_panda_core_scan(p, 4, 16, p, p, 2, 0, 1.0, 1.0, 0, 2, p, p, None) == -1 and b"w0" in lib.bmf_last_error()
    assert lib.bmf_panda_close(p, 4, 16, 4, p, p, None) == -1 and b"column" in lib.bmf_last_error()
    assert lib.bmf_panda_close(p, 4, 16, -1, None, p, None) == -1
    assert lib.bmf_panda_ext_scan(p, None, 4, 16, p, p, 2, 3, 1.0, 1.0, 1.0, 5.0, p, p, p, None) == -1
    assert lib.bmf_panda_ext_scan(p, p, 4, 16, p, p, 0, 3, 1.0, 1.0, 1.0, 5.0, p, p, p, None) == -1
    assert lib.bmf_panda_ext_scan(p, p, 4, 16, p, p, 2, -1, 1.0, 1.0, 1.0, 5.0, p, p, p, None) == -1
    assert lib.bmf_panda_rows(p, p, 8, 16, 4, 4, p, p, 3, p, 16, 1.0, 1.0, 1.0, p, p, None) == -1 and b"column" in lib.bmf_last_error()
    assert lib.bmf_panda_rows(p, p, 600, 16, 4, 1, p, p, 3, p, 16, 1.0, 1.0, 1.0, p, p, None) == -1 and b"32 * ldt" in lib.bmf_last_error()
    assert lib.bmf_panda_rows(p, p, 8, 16, 600, 1, p, p, 3, p, 16, 1.0, 1.0, 1.0, p, p, None) == -1
    assert lib.bmf_panda_rows(p, p, 8, 16, 4, 1, p, p, 3, p, 16, 1.0, 1.0, 1.0, None, p, None) == -1
