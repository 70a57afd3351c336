"""FastStep without a GPU: the model's host loop (models/FastStep.py) on a NumPy fp64 evaluator that offers the engine's calls
(set_factor / evaluate / commit), against the trajectories the reference produced (tests/golden/g22_faststep.*, written by
tests/golden/make_golden_faststep.py).

The evaluator is first held to the reference's own F / dF at the stored points (rtol 1e-12: same formula, same precision, only the
summation order differs); the class on that evaluator must then reproduce every log row: the same (round, k, iter) sequence and row
count -- which pins the projection, the one-past-the-limit stopping rules and the per-step logging -- the F columns to 1e-9
relative, and equal integer counts.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)


class NumpyEvaluator:
    """The arithmetic of FastStep.F / dF (PyBMF/models/FastStep.py:147-211) and of X_pd = (S > tau) in NumPy fp64, behind the
    interface of pybmf_amd.faststep.FastStepEngine.  S - tau is formed like on the device, (sum over the other columns - tau) + u v^T,
    the softplus in its stable form."""

    def __init__(self, X, k, tau, U, V, mask=None):
        self.X = np.asarray(X) != 0
        self.m, self.n = self.X.shape
        self.k, self.tau = int(k), float(tau)
        self.W = None if mask is None else (np.asarray(mask) != 0)
        self.U, self.V = np.array(U, dtype=np.float64), np.array(V, dtype=np.float64)
        self.sum_x = int(self.X.sum())
        self.B = None

    def set_factor(self, k):
        keep = [c for c in range(self.k) if c != k]
        self.B = self.U[:, keep] @ self.V[:, keep].T - self.tau

    def evaluate(self, u, v, want_grad=True, want_counts=False):
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        s = self.B + np.outer(u, v)
        a = np.where(self.X, -s, s)
        e = np.exp(-np.abs(a))
        sp = np.maximum(a, 0.0) + np.log1p(e)
        if self.W is not None:
            sp = np.where(self.W, sp, np.log(2.0))
        F = float(sp.sum())
        du = dv = tp = fp = None
        if want_grad:
            sig = np.where(a >= 0, 1.0, e) / (1.0 + e)
            g = np.where(self.X, -sig, sig)
            if self.W is not None:
                g = np.where(self.W, g, 0.0)
            du, dv = g @ v, g.T @ u
        if want_counts:
            pd = s > 0
            tp, fp = int((pd & self.X).sum()), int((pd & ~self.X).sum())
        return F, du, dv, tp, fp

    def commit(self, k, u, v):
        self.U[:, k], self.V[:, k] = u, v

    def prediction(self):
        return csr_matrix((self.U @ self.V.T > self.tau).astype(int))

    def factors(self):
        return self.U.copy(), self.V.copy()


def load_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g22_faststep.json")))
    z = np.load(os.path.join(GOLDEN, "g22_faststep.npz"))
    c = dict(meta["cases"][name])
    for key in ("X", "pattern", "U0", "V0", "U", "V"):
        c[key] = z[f"{name}_{key}"]
    for i, p in enumerate(c["points"]):
        for key in ("U", "V", "params", "dF"):
            p[key] = z[f"{name}_p{i}_{key}"]
    c.update(k=meta["k"], max_round=meta["max_round"], max_iter=meta["max_iter"])
    return c


def train_matrix(case):
    """X_train as the fixture script handed it to the reference: csr of the ones; for W = 'mask' the ones plus the stored zeros."""
    if case["W"] == "full":
        return csr_matrix(case["X"].astype(np.float64))
    rows, cols = np.nonzero(case["pattern"])
    return csr_matrix((case["X"][rows, cols].astype(np.float64), (rows, cols)), shape=case["X"].shape)


def make_model(case, engine_factory=None):
    """A FastStep that starts from the fixture's factors (after to_interval); engine_factory(model) replaces the device engine --
    then the bits of X never go to a GPU either."""
    from pybmf_amd.models import FastStep

    class Model(FastStep):
        def _start_factors(self):
            self.U, self.V = case["U0"].copy(), case["V0"].copy()

        if engine_factory is not None:
            def _to_device(self):
                self._boolean, self._all_cells, self._sharded, self._rows, self._bits = True, False, False, (0, self.m), None
                self._x_mean = float(self.X_train.sum()) / (float(self.m) * float(self.n))

            def _make_engine(self):
                return engine_factory(self)

    with contextlib.redirect_stdout(io.StringIO()):
        return Model(k=case["k"], W=case["W"], tau=case["tau"], max_round=case["max_round"], max_iter=case["max_iter"], seed=5)


def fit_quietly(model, X):
    with contextlib.redirect_stdout(io.StringIO()):
        model.fit(X, **FIT_KW)
    return model


def log_rows(model):
    """[(round, k, iter, original_F, projected_F, Recall, Precision, Accuracy, F1)] of logs['updates'] (the time stamp dropped)."""
    return [[float(v) for v in r[1:]] for r in model.logs["updates"].values.tolist()]


def numpy_engine(case):
    def factory(model):
        mask = None if model._mask_pattern is None else np.asarray(model._mask_pattern.todense())
        return NumpyEvaluator(case["X"], model.k, model.tau, model.U, model.V, mask=mask)
    return factory


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_numpy_evaluator_matches_the_reference_at_the_stored_points(name):
    case = load_case(name)
    for p in case["points"]:
        ev = NumpyEvaluator(case["X"], case["k"], case["tau"], p["U"], p["V"], mask=None if case["W"] == "full" else case["pattern"])
        ev.set_factor(p["k"])
        m = case["X"].shape[0]
        F, du, dv, _, _ = ev.evaluate(p["params"][:m], p["params"][m:], True, False)
        assert abs(F - p["F"]) <= 1e-12 * abs(p["F"])
        got = np.concatenate([du, dv])
        assert np.abs(got - p["dF"]).max() <= 1e-12 * np.abs(p["dF"]).max()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_host_loop_reproduces_the_reference_rows(name):
    case = load_case(name)
    model = fit_quietly(make_model(case, numpy_engine(case)), train_matrix(case))
    got, want = log_rows(model), case["log"]["rows"]
    assert [c[-1] for c in case["log"]["columns"][:5]] == ["round", "k", "iter", "original_F", "projected_F"]
    assert len(got) == len(want)
    assert [r[:3] for r in got] == [r[:3] for r in want]
    # the loops run one count past their limits
    assert max(r[0] for r in got) == case["max_round"] + 1 and max(r[2] for r in got) == case["max_iter"] + 1
    G, Wt = np.array(got), np.array(want)
    assert np.abs(G[:, 3:5] / Wt[:, 3:5] - 1).max() <= 1e-9
    assert np.abs(G[:, 5:] - Wt[:, 5:]).max() <= 1e-12          # scores: ratios of equal integer counts
    tp, fp = model._counts
    fn = int(case["X"].sum()) - tp
    assert [tp, fp, fn, case["X"].size - tp - fp - fn] == case["counts"]
    assert np.abs(model.U - case["U"]).max() <= 1e-9 * np.abs(case["U"]).max()
    assert np.abs(model.V - case["V"]).max() <= 1e-9 * np.abs(case["V"]).max()
    X_pd = np.asarray(model.X_pd.todense())
    assert (int((X_pd & case["X"]).sum()), int((X_pd & (1 - case["X"])).sum())) == (tp, fp)


def test_refusals():
    from pybmf_amd.models import FastStep
    case = load_case("a")
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match="W='full' or W='mask'"):
            FastStep(k=2, W=np.ones(case["X"].shape))
        model = make_model(case, numpy_engine(case))
        with pytest.raises(NotImplementedError, match="X_val / X_test"):
            model.fit(train_matrix(case), X_val=train_matrix(case), **FIT_KW)
        with pytest.raises(NotImplementedError, match="reconstruction"):
            model.fit(train_matrix(case), **dict(FIT_KW, task="prediction"))
