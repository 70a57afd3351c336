"""MEBF without a GPU: the model's host loop (models/MEBF.py) on a NumPy stand-in that offers the calls of
pybmf_amd.mebf.MedianEngine (growth / weak / apply / truncate / rebuild / counts / ...), against what the reference produced
(tests/golden/g27_mebf.*, written by tests/golden/make_golden_mebf.py).

The stand-in works on packed uint32 words in the engine's layout (both orientations, m_pad and n_pad multiples of 512).  (i) The
real class on it must reproduce every recorded fit -- recorded from the reference with a stable argsort, the tie rule this build
defines: the integers of every log row equal, `cost` equal (== for weights whose products with counts are exact, 1e-12 relative
otherwise), the metric columns to 1e-12 (ratios of equal integers), U, V and the counts cell for cell.  Where the reference ends in
the TypeError of its own early_stop (cases d, e, g, g2) the rows and factors up to there are what is compared: the stop itself is
meant to leave them.  (ii) At calls recorded from the reference as shipped, the grow step at the reference's own `mid` gives its
(a, b), and the defined rule's pick has the score of that `mid`: both lie in one tie group.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
CASES = ["a", "b", "c", "d", "e", "f", "g", "g2", "h"]
POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def row_popcounts(M):
    return POP8[np.ascontiguousarray(M, dtype=np.uint32).view(np.uint8)].reshape(M.shape[0], -1).sum(axis=1)


def order(scores):
    """The defined order: score descending, among equal scores the higher index first."""
    return np.flip(np.argsort(np.asarray(scores), kind="stable"))


def select_median(scores):
    """(mid, P): the index at rank P // 2 of the P positive scores in the defined order; mid = -1 when P = 0."""
    idx = [int(i) for i in order(scores) if scores[i] > 0]
    return (idx[len(idx) // 2] if idx else -1), len(idx)


def grow(rs, x, pd, N, a, t):
    """What bmf_mebf_grow returns for the vector a: (b as a bool vector over the N bit rows, |a|, |b|, dTP, dFP)."""
    c = row_popcounts(rs[:N] & a)
    na = popcount(a)
    b = c.astype(np.float64) > t * np.float64(na)
    free_a = a & ~pd[:N][b]
    return b, na, int(b.sum()), popcount(free_a & x[:N][b]), popcount(free_a & ~x[:N][b])


class NumpyMedianEngine:
    """pybmf_amd.mebf.MedianEngine in NumPy, same layout, same interface.  Index 0 = transposed (axis 0), 1 = row-major (axis 1)."""

    class State:
        def __init__(self, x):
            self.rs, self.pd, self.factors = [x[0].copy(), x[1].copy()], [np.zeros_like(x[0]), np.zeros_like(x[1])], []

    def __init__(self, X, extra=None):
        X = np.asarray(X) != 0
        self.m, self.n = X.shape
        self.W, self.nvw = -(-max(self.m, 1) // 512) * 16, -(-self.n // 512) * 16
        self.x = [pack_rows(X.T, self.W), pack_rows(X, self.nvw)]
        self.N, self.sum_x = [self.n, self.m], int(X.sum())
        self.truth = {"train": self.x[0]}
        for name, G in (extra or {}).items():
            self.truth[name] = pack_rows((np.asarray(G) != 0).T, self.W)
        self._live, self._kept, self._stale = self.State(self.x), None, False
        self.reads = 0

    def _base(self):
        return self._kept if self._stale else self._live

    def _candidate(self, axis, i0, i1, a, t):
        b, na, nb, dtp, dfp = grow(self._live.rs[axis], self.x[axis], self._base().pd[axis], self.N[axis], a, t)
        bw = pack_rows(b[None, :], self.nvw if axis == 0 else self.W)[0]
        u, v = (a, bw) if axis == 0 else (bw, a)
        return dict(axis=axis, mid=i0, P=i1, na=na, nb=nb, dTP=dtp, dFP=dfp, u=u.copy(), v=v.copy())

    def growth(self, t):
        out = []
        for axis in (0, 1):
            rs = self._live.rs[axis]
            mid, P = select_median(row_popcounts(rs[: self.N[axis]]))
            out.append(self._candidate(axis, mid, P, rs[mid].copy() if mid >= 0 else np.zeros(rs.shape[1], dtype=np.uint32), t))
        self.reads += 1
        return out

    def weak(self, t):
        rs = self._live.rs[0]
        idx = order(row_popcounts(rs[: self.n]))
        first, second = int(idx[0]), int(idx[1])       # IndexError with one column, as the reference
        self.reads += 1
        return self._candidate(0, first, second, rs[first] & rs[second], t)

    @staticmethod
    def _apply(st, m, n, u, v):
        u, v = np.array(u, dtype=np.uint32), np.array(v, dtype=np.uint32)
        cols, rows = np.nonzero(unpack(v, n))[0], np.nonzero(unpack(u, m))[0]
        st.rs[0][cols] &= ~u
        st.pd[0][cols] |= u
        st.rs[1][rows] &= ~v
        st.pd[1][rows] |= v
        st.factors.append((u, v))

    def apply(self, u, v, cand=None):
        if self._stale:
            self._live, self._kept, self._stale = self._kept, self._live, False
        self._apply(self._live, self.m, self.n, u, v)

    def rebuild(self, factors):
        self._stale, self._live = False, self.State(self.x)
        for u, v in factors:
            self._apply(self._live, self.m, self.n, u, v)

    def truncate(self, kept):
        self._kept, self._stale = self.State(self.x), True
        for u, v in kept:
            self._apply(self._kept, self.m, self.n, u, v)

    def residual_sum(self):
        return popcount(self._live.rs[0])

    def _fp_fn(self, st):
        return popcount(st.pd[0] & ~self.x[0]), popcount(self.x[0] & ~st.pd[0])

    def error_counts(self):
        return self._fp_fn(self._live)

    def base_counts(self):
        return self._fp_fn(self._base())

    def counts(self, name="train"):
        G, pd = self.truth[name], self._live.pd[0]
        tp, n_pd, n_gt = popcount(pd & G), popcount(pd), popcount(G)
        return tp, n_pd - tp, n_gt - tp, self.m * self.n - n_pd - (n_gt - tp)

    def factor_arrays(self):
        fs = self._live.factors
        U = np.array([unpack(u, self.m) for u, _ in fs], dtype=np.uint8).reshape(len(fs), self.m).T
        V = np.array([unpack(v, self.n) for _, v in fs], dtype=np.uint8).reshape(len(fs), self.n).T
        return U, V

    def prediction(self):
        rows = np.unpackbits(self._live.pd[1][: self.m].view(np.uint8), axis=1, bitorder="little")[:, : self.n]
        return csr_matrix(rows.astype(int))

    def bit_matrices(self, kept=False):
        st = self._kept if kept else self._live
        return st.rs[0], st.pd[0], st.rs[1], st.pd[1]


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_meta():
    return json.load(open(os.path.join(GOLDEN, "g27_mebf.json")))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, "g27_mebf.npz"))
    c = dict(load_meta()["cases"][name])
    for key in ("X", "U", "V", "X_val", "X_test"):
        if f"{name}_{key}" in z.files:
            c[key] = z[f"{name}_{key}"]
    return c


def load_points(name):
    z = np.load(os.path.join(GOLDEN, "g27_mebf.npz"))
    meta = load_meta()
    c = dict(meta["shipped"][name], X=z[f"{name}_X"])
    for i, p in enumerate(c["points"]):
        for key in ("X_rs", "a", "b"):
            p[key] = z[f"s{name}_p{i}_{key}"]
    return c


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyMedianEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, engine_factory=None):
    """The real class on case's matrices; engine_factory(model) replaces the device engine."""
    from pybmf_amd.models import MEBF

    class Model(MEBF):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(k=case["k"], tol=case["tol"], t=case["t"], w_fp=case["w_fp"], w_fn=case["w_fn"])
        model.fit(sp("X"), sp("X_val"), sp("X_test"), **FIT_KW)
    return model


def log_rows(model):
    """[[cost, |u|, |v|, rs, metrics ...]] of logs['updates'] (time stamp dropped, the shape cell flattened)."""
    if "updates" not in model.logs:
        return []
    return [[r[1], r[2][0], r[2][1], r[3]] + [float(x) for x in r[4:]] for r in model.logs["updates"].values.tolist()]


def check_cost(got, want, exact):
    if exact:
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def check_fit(model, case):
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want)
    exact = exact_weights(case["w_fp"], case["w_fn"])
    if want:
        assert case["log"]["columns"][:4] == ["cost", "n_u", "n_v", "rs"]
    for g, w in zip(got, want):
        check_cost(float(g[0]), w[0], exact)
        assert all(isinstance(x, (int, np.integer)) for x in g[1:4]) and [int(x) for x in g[1:4]] == w[1:4]
        assert len(g) == len(w) and np.abs(np.array(g[4:]) - np.array(w[4:])).max() <= 1e-12
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    f = case["U"].shape[1]
    if case["raised"]:       # the fixture keeps the factors up to the stop; the stop here truncates to them
        assert U.shape[1] <= f and not (case["U"][:, U.shape[1]:].any() and case["V"][:, U.shape[1]:].any())
        f = U.shape[1]
    assert U.shape == (case["shape"][0], f) and V.shape == (case["shape"][1], f)
    assert U.tolist() == (case["U"][:, :f] != 0).tolist() and V.tolist() == (case["V"][:, :f] != 0).tolist()
    eng = model._engine
    assert list(eng.counts("train")) == case["counts"]
    X_pd, X = np.asarray(model.X_pd.todense()), case["X"]
    assert [int((X_pd & X).sum()), int((X_pd & (1 - X)).sum())] == case["counts"][:2]
    assert eng.residual_sum() == case["counts"][2]
    rs_t, pd_t, rs, pd = eng.bit_matrices()
    assert unpack_matrix(pd, *X.shape).tolist() == (X_pd != 0).tolist()


def unpack_matrix(words, rows, cols):
    return np.unpackbits(np.ascontiguousarray(words[:rows], dtype=np.uint32).view(np.uint8), axis=1, bitorder="little")[:, :cols].astype(bool)


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


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    model = fit_case(case, numpy_engine)
    check_fit(model, case)
    check_state(model._engine, case["X"])
    rows = case["log"]["rows"]
    if name == "a":
        assert len(rows) == case["k"] == model.U.shape[1] and not case["truncations"]
    if name == "b":      # error <= tol = 0 at the last factor: dropped from U, V, still in X_pd and the log
        assert model._engine.residual_sum() == 0 and model.U.shape[1] == len(rows) - 1 and case["truncations"] == [len(rows) - 1]
    if name in ("d", "e", "g", "g2"):
        assert case["raised"] == "TypeError"
    if name == "e":
        assert rows == [] and model.U.shape[1] == 0
    if name == "g2":     # three truncations, the fit going on in between: an empty column stays where a factor was dropped
        assert case["truncations"] == [1, 2, 3] and len(rows) == 4
        assert not np.asarray(model.U.todense())[:, 1:].any() and np.asarray(model.U.todense())[:, 0].any()
    if name == "h":
        assert [c.split("/")[0] for c in case["log"]["columns"][4:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4


def test_weak_signal_is_reached_and_the_fit_goes_on():
    case = load_case("c")
    calls = []

    def factory(model):
        eng = numpy_engine(model)
        weak = eng.weak
        eng.weak = lambda t: (calls.append(len(eng._live.factors)), weak(t))[1]
        return eng
    model = fit_case(case, factory)
    assert calls and calls[0] < len(case["log"]["rows"]) - 1
    check_fit(model, case)


@pytest.mark.parametrize("name", ["a", "c"])
def test_grow_step_at_the_reference_s_own_mid(name):
    case = load_points(name)
    assert len(case["points"]) == 3
    for p in case["points"]:
        eng = NumpyMedianEngine(case["X"])
        axis, R = p["axis"], p["X_rs"] != 0
        st = eng._live
        st.rs = [pack_rows(R.T, eng.W), pack_rows(R, eng.nvw)]
        st.pd = [eng.x[0] & ~st.rs[0], eng.x[1] & ~st.rs[1]]
        scores = R.sum(axis=axis)
        mid, P = select_median(scores)
        assert p["mid"] >= 0 and scores[mid] == scores[p["mid"]] and P == int((scores > 0).sum())
        a = st.rs[axis][p["mid"]]
        b, na, nb, _, _ = grow(st.rs[axis], eng.x[axis], st.pd[axis], eng.N[axis], a, case["t"])
        assert unpack(a, R.shape[axis]).tolist() == (p["a"] != 0).tolist() and b.tolist() == (p["b"] != 0).tolist()
        assert (na, nb) == (int(p["a"].sum()), int(p["b"].sum()))
        c = eng.growth(case["t"])[axis]
        assert (c["mid"], c["P"]) == (mid, P)


def test_tie_rule_on_a_hand_made_score_vector():
    #                0  1  2  3  4  5  6  7  8  9
    s = np.array([3, 5, 0, 3, 5, 1, 3, 0, 1, 5])
    assert order(s).tolist() == [9, 4, 1, 6, 3, 0, 8, 5, 7, 2]          # three tie groups (5, 3, 1) and the zeros
    assert select_median(s) == (3, 8)                                   # P = 8 (even): rank 4
    s[5] = 0
    assert select_median(s) == (6, 7)                                   # P = 7 (odd): rank 3
    assert select_median(np.zeros(5, dtype=int)) == (-1, 0)
    assert select_median(np.array([0, 2, 0])) == (1, 1)
    assert select_median(np.array([4, 4])) == (0, 2)                    # P = 2: rank 1 = the lower index of a tie
    assert select_median(np.array([4, 7])) == (0, 2)


def test_refusals():
    from pybmf_amd.models import MEBF
    case = load_case("a")
    X = csr_matrix(case["X"].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(TypeError, match="NoneType"):
            MEBF(k=2).fit(X, **FIT_KW)
        with pytest.raises(NotImplementedError, match="reconstruction"):
            MEBF(k=2, t=0.5).fit(X, **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            MEBF(k=2, t=0.5).fit(case["X"].astype(np.float64) * 3, **FIT_KW)
    # the weak signal takes the two fullest columns: with one column the reference's idx[1] raises
    eng = NumpyMedianEngine(np.ones((6, 1), dtype=np.uint8))
    with pytest.raises(IndexError):
        eng.weak(0.5)


def test_stops_with_a_message_leave_the_factors_found_so_far():
    for name in ("d", "e", "g"):
        case = load_case(name)
        model = fit_case(case, numpy_engine)
        assert model.U.shape[1] == model.V.shape[1] <= len(case["log"]["rows"])


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {"bmf_mebf_scores": 6, "bmf_mebf_select": 5, "bmf_mebf_weak_a": 5, "bmf_mebf_grow_work": 1, "bmf_mebf_grow": 13,
                    "bmf_mebf_apply": 10}


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
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert lib.bmf_mebf_grow_work(0) == -1 and lib.bmf_mebf_grow_work(10) == 120
    assert lib.bmf_mebf_scores(None, 4, 16, p, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_mebf_scores(p, 0, 16, p, p, None) == -1
    assert lib.bmf_mebf_select(p, 0, 0, p, None) == -1
    assert lib.bmf_mebf_select(p, 1, 1, p, None) == -1 and b"2 scores" in lib.bmf_last_error()
    assert lib.bmf_mebf_weak_a(p, 16, None, p, None) == -1
    assert lib.bmf_mebf_grow(p, p, p, 4, 18, p, 1, 0.5, p, p, 1, p, None) == -1 and b"multiple of 4" in lib.bmf_last_error()
    assert lib.bmf_mebf_grow(p, p, p, 40, 16, p, 1, 0.5, p, p, 1, p, None) == -1 and b"ceil" in lib.bmf_last_error()
    assert lib.bmf_mebf_grow(p, p, p, 4, 16, C.c_void_p(p.value + 4), 1, 0.5, p, p, 1, p, None) == -1 and b"aligned" in lib.bmf_last_error()
    assert lib.bmf_mebf_apply(p, p, 4, 16, None, p, p, p, p, None) == -1
