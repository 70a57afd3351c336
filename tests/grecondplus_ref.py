"""GreConD+ in NumPy: the stand-in for pybmf_amd.grecondplus.ExpansionEngine that tests/test_grecondplus_cpu.py holds to the reference's
recorded results (tests/golden/g29_grecondplus.*) and tests/test_grecondplus_gpu.py holds the kernels to.

The dense functions work on 0 / 1 matrices straight from the definitions (expansion(), remove_covered(), remove_overlapped() of
PyBMF/models/GreConDPlus.py); NumpyExpansionEngine wraps them in the engine's interface on packed uint32 words (the layout of
tests/test_grecond_cpu.NumpyConceptEngine, which supplies the concept search).

The score of a line: d = ((-w_fp) c + w_fn b) - ((-w_fp) 0 + w_fn a) in fp64, evaluated in exactly that order by NumPy's element-wise
loops (no FMA); the counts come from fp64 matrix-vector products of 0 / 1 matrices, exact far beyond any size used here.
"""
import contextlib
import io
import json
import os

import numpy as np
from scipy.sparse import csr_matrix

from test_grecond_cpu import FIT_KW, NumpyConceptEngine, pack_rows, popcount, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- dense definitions --------------------------------------------------------------------------------------------------------
def line_counts(X, RS, s):
    """(a, b, c) per row of X: a = |rs_i|, b = |x_i & (rs_i | s)|, c = |s & ~x_i|, by the definition, on bool matrices."""
    X, RS, s = np.asarray(X, dtype=bool), np.asarray(RS, dtype=bool), np.asarray(s, dtype=bool)
    return (RS.sum(axis=1).astype(np.int64), (X & (RS | s[None, :])).sum(axis=1).astype(np.int64),
            (s[None, :] & ~X).sum(axis=1).astype(np.int64))


def line_scores(a, b, c, inside, w_fp, w_fn):
    """d per line, fp64: the reference's s_new - s_old with FP_old = 0; 0.0 for a line inside its own set."""
    a, b, c = (np.asarray(t, dtype=np.float64) for t in (a, b, c))
    w_fp, w_fn = np.float64(w_fp), np.float64(w_fn)
    s_new = (-w_fp) * c + w_fn * b
    s_old = (-w_fp) * np.zeros_like(a) + w_fn * a
    d = s_new - s_old
    d[np.asarray(inside, dtype=bool)] = 0.0
    return d


def decide(r_score, c_score):
    """1: the row joins, 0: the column joins, -1: stop (equal positive scores included)."""
    if r_score > c_score and r_score > 0:
        return 1
    if c_score > r_score and c_score > 0:
        return 0
    return -1


def expansion_ref(X, RS, u, v, w_fp, w_fn, max_steps=None, with_counters=False):
    """expansion(X_gt=X, X_old=RS, u, v, w_fp, w_fn) -> (u_exp, v_exp, trace[, counters]); trace: (axis, index, r_score, c_score) per
    evaluated step, the stop (axis -1, index -1) included; counters: ((a, b, c) rows, (a, b, c) columns) as they stood at each step.
    RS must lie inside X (it is a residual)."""
    X, RS = np.asarray(X, dtype=bool), np.asarray(RS, dtype=bool)
    assert not (RS & ~X).any()
    u, v = np.asarray(u, dtype=bool).copy(), np.asarray(v, dtype=bool).copy()
    u_exp, v_exp = np.zeros_like(u), np.zeros_like(v)
    P, N = (X & ~RS).astype(np.float64), (~X).astype(np.float64)       # ones covered already, zeros
    a_r, a_c = RS.sum(axis=1).astype(np.float64), RS.sum(axis=0).astype(np.float64)
    trace, counters = [], []
    while max_steps is None or len(trace) < max_steps:
        vf, uf = v.astype(np.float64), u.astype(np.float64)
        b_r, c_r = a_r + P @ vf, N @ vf
        b_c, c_c = a_c + uf @ P, uf @ N
        d_r, d_c = line_scores(a_r, b_r, c_r, u, w_fp, w_fn), line_scores(a_c, b_c, c_c, v, w_fp, w_fn)
        r_index, c_index = int(np.argmax(d_r)), int(np.argmax(d_c))
        r_score, c_score = float(d_r[r_index]), float(d_c[c_index])
        axis = decide(r_score, c_score)
        if with_counters:
            counters.append((np.array([a_r, b_r, c_r]).astype(np.int64), np.array([a_c, b_c, c_c]).astype(np.int64)))
        trace.append((axis, r_index if axis == 1 else (c_index if axis == 0 else -1), r_score, c_score))
        if axis == 1:
            u[r_index] = u_exp[r_index] = True
        elif axis == 0:
            v[c_index] = v_exp[c_index] = True
        else:
            break
    return (u_exp, v_exp, trace, counters) if with_counters else (u_exp, v_exp, trace)


def remove_covered_ref(U, V, Ue, Ve, k):
    """The factors i != k with u_i inside u_k and v_i inside v_k leave all four matrices."""
    U, V = np.asarray(U) != 0, np.asarray(V) != 0
    keep = [i for i in range(U.shape[1]) if i == k or not (not (U[:, i] & ~U[:, k]).any() and not (V[:, i] & ~V[:, k]).any())]
    return tuple(np.asarray(A)[:, keep].astype(np.uint8) for A in (U, V, Ue, Ve))


def remove_overlapped_ref(X, U, V, Ue, Ve):
    """remove_overlapped() line by line: coverage = U @ V.T is counted once; per factor the rows and columns are taken BEFORE the row
    loop, so the column loop reads and decrements the rows just removed."""
    X = (np.asarray(X) != 0).astype(np.int64)
    U, V, Ue, Ve = (np.asarray(A).astype(np.int64).copy() for A in (U, V, Ue, Ve))
    cov = (U.astype(np.float64) @ V.T.astype(np.float64)).astype(np.int64)        # (BLAS; exact on counts)
    for k in range(U.shape[1]):
        i_idx, j_idx = np.nonzero(U[:, k])[0], np.nonzero(V[:, k])[0]
        for i in np.nonzero(Ue[:, k] == 1)[0]:          # (ascending, as the loop over all rows meets them)
            if (cov[i, j_idx] * X[i, j_idx]).min() >= 2:
                U[i, k] = Ue[i, k] = 0
                cov[i, j_idx] -= 1
        for j in np.nonzero(Ve[:, k] == 1)[0]:
            if (cov[i_idx, j] * X[i_idx, j]).min() >= 2:
                V[j, k] = Ve[j, k] = 0
                cov[i_idx, j] -= 1
    return tuple(A.astype(np.uint8) for A in (U, V, Ue, Ve))


def overlap_prefilter_ref(X, U, V, Ue, Ve):
    """The number of (factor, extension line) pairs whose line of X holds the factor's other set: no removal without one."""
    X, U, V = np.asarray(X) != 0, np.asarray(U) != 0, np.asarray(V) != 0
    n = 0
    for k in range(U.shape[1]):
        n += sum(1 for i in np.nonzero(np.asarray(Ue)[:, k])[0] if not (V[:, k] & ~X[i]).any())
        n += sum(1 for j in np.nonzero(np.asarray(Ve)[:, k])[0] if not (U[:, k] & ~X[:, j]).any())
    return n


# ---- the engine's interface ---------------------------------------------------------------------------------------------------
class NumpyExpansionEngine(NumpyConceptEngine):
    """pybmf_amd.grecondplus.ExpansionEngine in NumPy: packed words in and out."""

    def __init__(self, X, extra=None):
        super().__init__(X, extra)
        self.X = np.asarray(X) != 0
        self.trace, self.pruned = [], (0, 0, 0)

    def dense(self, rows_t):
        """A transposed packed bit matrix (n bit rows) as an m x n bool matrix."""
        return np.unpackbits(rows_t[: self.n].view(np.uint8), axis=1, bitorder="little")[:, : self.m].T.astype(bool)

    def unpack_factors(self, U, V):
        U, V = np.asarray(U, dtype=np.uint32).reshape(-1, self.W), np.asarray(V, dtype=np.uint32).reshape(-1, self.nvw)
        f = U.shape[0]
        return (np.array([unpack(U[i], self.m) for i in range(f)], dtype=np.uint8).reshape(f, self.m).T,
                np.array([unpack(V[i], self.n) for i in range(f)], dtype=np.uint8).reshape(f, self.n).T)

    def expand(self, u, v, w_fp, w_fn, steps=None):
        u_exp, v_exp, self.trace = expansion_ref(self.X, self.dense(self.rs_t), unpack(u, self.m), unpack(v, self.n), w_fp, w_fn)
        return pack_rows(u_exp[None, :], self.W)[0], pack_rows(v_exp[None, :], self.nvw)[0], len(self.trace)

    def prune_overlapped(self, U, V, U_exp, V_exp):
        Ud, Vd = self.unpack_factors(U, V)
        Ued, Ved = self.unpack_factors(U_exp, V_exp)
        passed = overlap_prefilter_ref(self.X, Ud, Vd, Ued, Ved)
        out = remove_overlapped_ref(self.X, Ud, Vd, Ued, Ved)
        self.pruned = (passed, int(Ued.sum() - out[2].sum()), int(Ved.sum() - out[3].sum()))
        assert passed or self.pruned[1:] == (0, 0)
        return (pack_rows(out[0].T, self.W), pack_rows(out[1].T, self.nvw), pack_rows(out[2].T, self.W), pack_rows(out[3].T, self.nvw))

    def rebuild(self, U, V):
        Ud, Vd = self.unpack_factors(U, V)
        pd = (Ud.astype(np.float64) @ Vd.astype(np.float64).T) > 0
        self.pd_t = pack_rows(pd.T, self.W)
        self.rs_t = self.Xt & ~self.pd_t
        U, V = np.asarray(U, dtype=np.uint32).reshape(-1, self.W), np.asarray(V, dtype=np.uint32).reshape(-1, self.nvw)
        self._factors = [(U[i].copy(), V[i].copy()) for i in range(U.shape[0])]

    def apply(self, u, v):
        raise NotImplementedError("GreConD+ sets its residual with rebuild()")


# ---- fixtures and fits --------------------------------------------------------------------------------------------------------
CASES = ["a", "b", "c", "d", "e", "f", "g"]
OVERLAPPED = ["row", "column", "stale", "twice", "single", "nothing", "hole"]
COVERED = ["inside", "all_but_one", "none", "rows_only"]
_loaded = {}


def golden():
    if not _loaded:
        _loaded["meta"] = json.load(open(os.path.join(GOLDEN, "g29_grecondplus.json")))
        z = np.load(os.path.join(GOLDEN, "g29_grecondplus.npz"))
        _loaded["arrays"] = {k: z[k] for k in z.files}
    return _loaded["meta"], _loaded["arrays"]


def load_case(name):
    meta, z = golden()
    c = dict(meta["cases"][name])
    for key in ("X", "U", "V", "U_exp", "V_exp", "X_val", "X_test", "trace"):
        if f"{name}_{key}" in z:
            c[key] = z[f"{name}_{key}"]
    return c


def load_overlapped(name):
    meta, z = golden()
    return dict(meta["overlapped"][name], **{key: z[f"o_{name}_{key}"] for key in ("X", "U0", "V0", "Ue0", "Ve0", "U1", "V1", "Ue1", "Ve1")})


def load_covered(name):
    meta, z = golden()
    return dict(meta["covered"][name], **{key: z[f"c_{name}_{key}"] for key in ("U0", "V0", "Ue0", "Ve0", "U1", "V1", "Ue1", "Ve1")})


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyExpansionEngine(np.asarray(model.X_train.todense()), extra)


def fit_model(X, params, engine_factory=None, X_val=None, X_test=None, steps=None, block=None):
    """The real class; engine_factory(model) replaces the device engine.  The traces of all expansions are kept in model.traces."""
    from pybmf_amd.models import GreConDPlus

    class Model(GreConDPlus):
        def _make_engine(self):
            eng = engine_factory(self) if engine_factory is not None else super()._make_engine()
            self.traces = []
            expand = eng.expand

            def logged(*a, **kw):
                out = expand(*a, **kw)
                self.traces.append(list(eng.trace))
                return out
            eng.expand = logged
            return eng

    def sp(A):
        return None if A is None else csr_matrix(np.asarray(A).astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(**params)
        model.fit(sp(X), sp(X_val), sp(X_test), **dict(FIT_KW, steps=steps, block=block))
    return model


def fit_case(case, engine_factory=None, steps=None, block=None):
    params = {key: case[key] for key in ("k", "tol", "w_fp", "w_fn")}
    return fit_model(case["X"], params, engine_factory, case.get("X_val"), case.get("X_test"), steps, block)


def log_rows(model):
    """[[k, score, |u|, |v|, metrics ...]] of logs['updates'] (time stamp dropped, the shape cell flattened)."""
    if "updates" not in model.logs:
        return []
    return [[r[1], r[2], r[3][0], r[3][1]] + [float(x) for x in r[4:]] for r in model.logs["updates"].values.tolist()]


def trace_array(traces):
    """The traces of a fit as the fixture keeps them: one row (call, axis, index, r_score, c_score) per step."""
    rows = [[i, s[0], s[1], s[2], s[3]] for i, steps in enumerate(traces) for s in steps]
    return np.array(rows, dtype=np.float64).reshape(len(rows), 5)


def dense(A):
    return (np.asarray(A.todense()) != 0).astype(np.uint8)


def check_fit(model, case):
    """Everything the fixture recorded, exactly; the ratio columns of the log to 1e-12 as in tests/test_grecond_cpu.py."""
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want)
    n_head = 4
    if want:
        assert case["log"]["columns"][:n_head] == ["k", "score", "n_u", "n_v"]
        for g, w in zip(got, want):
            assert all(isinstance(x, (int, np.integer)) for x in g[:n_head]), g[:n_head]
            assert [int(x) for x in g[:n_head]] == w[:n_head]
        G, Wt = np.array([r[n_head:] for r in got]), np.array([r[n_head:] for r in want])
        assert G.shape == Wt.shape and np.abs(G - Wt).max() <= 1e-12
    for name in ("U", "V", "U_exp", "V_exp"):
        A = dense(getattr(model, name))
        assert A.shape == case[name].shape, (name, A.shape, case[name].shape)
        assert A.tolist() == (case[name] != 0).astype(np.uint8).tolist(), name
    assert list(model._engine.counts("train")) == case["counts"]
    X_pd, X = np.asarray(model.X_pd.todense()).astype(np.int64), case["X"].astype(np.int64)
    assert [int((X_pd & X).sum()), int((X_pd & (1 - X)).sum())] == case["counts"][:2]
    # the trace of every expansion: axis, index and both scores as raw fp64 bits
    got_t, want_t = trace_array(model.traces), case["trace"]
    assert got_t.shape == want_t.shape and got_t.tobytes() == want_t.tobytes()
    assert len(model.traces) == case["n_calls"] == len(want) and model.n_steps == [len(t) for t in model.traces]
    if case["raised"] is None:
        # the prediction is the product of the factors that survive
        U, V = dense(model.U).astype(np.int64), dense(model.V).astype(np.int64)
        assert ((U @ V.T > 0).astype(np.int64) == X_pd).all()
