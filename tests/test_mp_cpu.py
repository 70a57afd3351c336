"""MessagePassing without a GPU: the NumPy restatement (tests/mp_ref.py) on the fixtures, the model class on a NumPy stand-in engine, the
refusals, and the argument checks of the C entry points."""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import mp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_KW = dict(show_logs=False, show_result=False, save_model=False, verbose=False)
ENTRY_POINTS = {"bmf_mp_work": 3, "bmf_mp_start": 11, "bmf_mp_reduce": 15, "bmf_mp_step": 21}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_splitmix64_is_the_published_generator():
    """The first three outputs of splitmix64 seeded with 1234567 (the reference vector of the public-domain C code): the generator
    adds the constant to its state before every output, so output t = splitmix64(seed + (t - 1) gamma) in this module's form."""
    gamma = 0x9E3779B97F4A7C15
    got = [int(R.splitmix64(np.array([(1234567 + t * gamma) & R.MASK64], dtype=np.uint64))[0]) for t in range(3)]
    assert got == [6457827717110365317, 3203168211198807973, 9817491932198370423]


def test_start_values():
    Ph, Ps = R.start_hats(5, 7, 3, seed=0, init_scale=1e-2)
    assert Ph.shape == Ps.shape == (5, 7, 3) and np.abs(Ph).max() <= 1e-2 and np.abs(Ps).max() <= 1e-2
    assert len(np.unique(np.concatenate([Ph.ravel(), Ps.ravel()]))) == 2 * 5 * 7 * 3           # one counter per value
    base = int(R.splitmix64(np.array([0], dtype=np.uint64))[0])
    for which, i, j, f, H in ((0, 0, 0, 0, Ph), (0, 4, 6, 2, Ph), (1, 0, 0, 0, Ps), (1, 3, 5, 1, Ps)):
        idx = ((which * 5 + i) * 7 + j) * 3 + f
        h = int(R.splitmix64(np.array([(base + idx) & R.MASK64], dtype=np.uint64))[0])
        assert H[i, j, f] == 1e-2 * (2.0 * ((h >> 11) / 2.0 ** 53) - 1.0)
    pat = np.random.RandomState(0).rand(5, 7) < 0.5
    Pm, _ = R.start_hats(5, 7, 3, seed=0, init_scale=1e-2, pattern=pat)
    assert np.array_equal(Pm[pat], Ph[pat]) and not Pm[~pat].any()
    assert not np.array_equal(R.start_hats(5, 7, 3, 1, 1e-2)[0], Ph)


def test_cell_pass_by_hand_at_one_cell():
    """k = 2, one cell, worked by hand: Phi = (1, -2), Psi = (0.5, 3); G = (0.5, -2); T = 0.5; M = (-2, 0.5);
    G^ = (min(2, 0 + co), min(0, 0.5 + co)); co = log(0.99 / 0.01) for X = 1."""
    cx, cy, co1, co0 = R.constants(0.5, 0.5, 0.99, 0.99)
    assert cx == cy == 0.0 and co1 == -co0 == np.log(0.99 / (1 - 0.99))
    Xi, Ups = np.array([[1.0, -2.0]]), np.array([[0.5, 3.0]])
    Z = np.zeros((1, 1, 2))
    A, B = R.cell_pass(np.ones((1, 1)), None, Xi, Ups, Z, Z, co1, co0, lr=1.0)
    gh = np.array([min(2.0, co1), 0.0])
    assert np.array_equal(A[0, 0], np.maximum(gh + Ups[0], 0) - np.maximum(Ups[0], 0))
    assert np.array_equal(B[0, 0], np.maximum(gh + Xi[0], 0) - np.maximum(Xi[0], 0))
    A1, _ = R.cell_pass(np.ones((1, 1)), None, Xi[:, :1], Ups[:, :1], Z[:, :, :1], Z[:, :, :1], co1, co0, lr=1.0)
    assert A1[0, 0, 0] == max(min(np.inf, co1) + 0.5, 0) - 0.5                                     # k = 1: M = -inf, T - max(G, 0) = 0


def test_equal_top_values_count_twice():
    Xi, Ups = np.array([[1.0, 1.0, -3.0]]), np.array([[2.0, 2.0, 2.0]])
    Z = np.zeros((1, 1, 3))
    A, _ = R.cell_pass(np.zeros((1, 1)), None, Xi, Ups, Z, Z, 4.0, -4.0, lr=1.0)
    # G = (1, 1, -3): M = (1, 1, 1), so max(-M, 0) = 0 and every G^ is min(0, .) <= 0
    assert A[0, 0, 0] == A[0, 0, 1] and (A <= 0).all()


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixture_conditions_and_recovery(name):
    X, clean, pattern, res = R.fixture(name)
    R.check_fixture(res)
    err = (R.boolean_product(res["U"], res["V"]) ^ clean).mean()
    small = min(np.abs(res["Xi"]).min(), np.abs(res["Ups"]).min())
    print(f"{name}: n_iter={res['n_iter']} smallest |marginal|={small:.3g} last d={res['diffs'][-2:]} error against clean X={err:.4%}")
    assert err <= 0.002                                         # the planted product comes back (noise 2 - 5 %, 30 % hidden)
    rev = R.fixture(name, "reversed")[3]
    assert rev["n_iter"] == res["n_iter"] and np.array_equal(rev["U"], res["U"]) and np.array_equal(rev["V"], res["V"])


def test_non_convergent_case_leaves_by_max_iter():
    m, n, k, noise, s, _ = R.NON_CONVERGENT
    X = R.planted(m, n, k, noise, s)[0]
    res = R.fit(X, k, None, tol=R.TOL, max_iter=120, seed=R.SEED, **R.CONSTS)
    assert not res["converged"] and res["n_iter"] == 120 and min(res["diffs"]) >= R.TOL
    model = fit_stand_in(X, None, k=k, W="full", max_iter=120, task="reconstruction")
    assert model.converged is False and model.n_iter == 120 and len(model.logs["updates"]) == 120
    assert np.array_equal(model.U, res["U"]) and np.array_equal(model.V, res["V"])


# ---- the model class on a NumPy stand-in engine ------------------------------------------------------------------------------------------
def stand_in_class():
    from pybmf_amd.models import MessagePassing

    class Model(MessagePassing):
        """The device never enters: X stays on the host, the engine is the restatement's, the scores are NumPy counts under the rule of
        ContinuousModel._make_scorers (prediction: the non-zero stored entries of a set; reconstruction: its whole matrix)."""

        def _to_device(self):
            self._boolean, self._all_cells, self._sharded, self._rows, self._bits = True, False, False, (0, self.m), None
            self._check_boolean(self.X_train)

        def _make_scorers(self):
            self._scorers = {}

        def _make_engine(self):
            pattern = None if self._mask_pattern is None else np.asarray(self._mask_pattern.todense()) != 0
            return R.RefEngine(np.asarray(self.X_train.todense()) != 0, self.k, pattern, prior_u=self.prior_u, prior_v=self.prior_v,
                               channel_pos=self.channel_pos, channel_neg=self.channel_neg, lr=self.lr, init_scale=self.init_scale)

        def _score(self, name, metrics):
            gt = np.asarray(getattr(self, "X_" + name).todense()) != 0
            where = gt if self.task == "prediction" else None
            counts = R.confusion(gt, R.boolean_product(self.U > 0.5, self.V > 0.5), where)
            return self._metric_values(metrics, None, counts)
    return Model


def fit_stand_in(X, pattern, k, W, X_val=None, X_test=None, task="reconstruction", max_iter=R.MAX_ITER, seed=R.SEED, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        model = stand_in_class()(k=k, W=W, tol=R.TOL, max_iter=max_iter, seed=seed, **R.CONSTS, **kw)
        model.fit(R.train_csr(X, pattern), X_val, X_test, task=task, **FIT_KW)
    return model


def boolean_row(model):
    return [float(v) for v in model.logs["boolean"].values.tolist()[0][1:]]


@pytest.mark.parametrize("name", ["a60x50k3_masked", "b33x130k4_full"])
@pytest.mark.parametrize("task", ["reconstruction", "prediction"])
def test_model_on_the_stand_in_engine(name, task):
    X, clean, pattern, res = R.fixture(name)
    rs = np.random.RandomState(9)
    hidden = ~pattern if pattern is not None else rs.rand(*X.shape) < 0.2
    val, test = hidden & (rs.rand(*X.shape) < 0.5), hidden & ~(rs.rand(*X.shape) < 0.5)
    X_val, X_test = R.train_csr(X, val), R.train_csr(X, test)                  # stored cells, zeros included
    model = fit_stand_in(X, pattern, k=res["U"].shape[1], W="mask" if pattern is not None else "full", X_val=X_val, X_test=X_test, task=task)
    assert model.n_iter == res["n_iter"] and model.converged is True
    assert model.U.dtype == np.float64 and set(np.unique(model.U)) <= {0.0, 1.0}
    assert np.array_equal(model.U, res["U"]) and np.array_equal(model.V, res["V"])
    assert np.array_equal(model.marginal_U, res["Xi"]) and np.array_equal(model.marginal_V, res["Ups"])
    up = model.logs["updates"]
    assert [c[-1] for c in up.columns] == ["time", "iter", "diff"]
    assert [int(v) for v in up.iloc[:, 1]] == list(range(1, res["n_iter"] + 1)) and [float(v) for v in up.iloc[:, 2]] == res["diffs"]
    pd = R.boolean_product(res["U"], res["V"])
    want = []
    for gt in (X if pattern is None else X & pattern, X & val, X & test):      # what a csr of the set holds as non-zeros
        want += R.scores(R.confusion(gt, pd, gt if task == "prediction" else None))
    assert len(model.logs["boolean"]) == 1 and boolean_row(model) == want
    assert [c[0] for c in model.logs["boolean"].columns[1:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4


def test_a_weight_matrix_counts_as_a_pattern_and_seed_none_draws_from_the_rng():
    X, clean, pattern, res = R.fixture("a60x50k3_masked")
    W = pattern * np.random.RandomState(2).uniform(0.5, 3.0, size=X.shape)      # the weights are not used, only the non-zeros
    model = fit_stand_in(X, None, k=3, W=W)
    assert model.n_iter == res["n_iter"] and np.array_equal(model.marginal_U, res["Xi"])
    ones = fit_stand_in(X, None, k=3, W=np.ones(X.shape))                        # all-ones: the full pattern
    assert ones._mask_pattern is None
    with contextlib.redirect_stdout(io.StringIO()):
        model = stand_in_class()(k=3, W="mask", tol=R.TOL, **R.CONSTS)            # seed=None
        model.rng = np.random.RandomState(77)
        model.fit(R.train_csr(X, pattern), task="reconstruction", **FIT_KW)
    drawn = int(np.random.RandomState(77).randint(0, 2 ** 31 - 1))
    want = R.fit(X, 3, pattern, tol=R.TOL, max_iter=R.MAX_ITER, seed=drawn, **R.CONSTS)
    assert model.n_iter == want["n_iter"] and np.array_equal(model.marginal_V, want["Ups"])


def test_signature_and_refusals(monkeypatch):
    import inspect

    import pybmf_amd.engine as E
    from pybmf_amd import models
    from pybmf_amd.models.MessagePassing import MessagePassing
    assert models.MessagePassing is MessagePassing and "MessagePassing" in models.__all__
    sig = inspect.signature(MessagePassing.__init__)
    assert list(sig.parameters)[1:] == ["k", "W", "prior_u", "prior_v", "channel_pos", "channel_neg", "tol", "max_iter", "lr", "seed", "init_scale"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == ["mask", 0.5, 0.5, 0.99, 0.99, 1e-4, 500, 0.2, None, 1e-2]

    def no_upload(*a, **k):
        raise AssertionError("the data went to the device before the refusal")
    for name in ("BitMatrix", "SparseObs", "RealMatrix"):
        monkeypatch.setattr(E, name, no_upload)
    X = (np.random.RandomState(1).rand(10, 8) < 0.4).astype(np.uint8)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match="k=65.*k <= 64"):
            MessagePassing(k=65)
        with pytest.raises(NotImplementedError, match="k=0"):
            MessagePassing(k=0)
        for bad in (dict(prior_u=0.0), dict(prior_v=1.0), dict(channel_pos=1.0), dict(channel_neg=0.0), dict(prior_u=-0.2), dict(channel_pos=1.5)):
            with pytest.raises(ValueError, match=r"inside \(0, 1\)"):
                MessagePassing(k=2, **bad)
        with pytest.raises(ValueError, match="lr=0"):
            MessagePassing(k=2, lr=0)
        with pytest.raises(NotImplementedError, match=r"Boolean \(0/1\)"):
            MessagePassing(k=2, W="full").fit(X.astype(np.float64) * 0.5, task="reconstruction", **FIT_KW)
        with pytest.raises(ValueError, match="shape of X_train"):
            stand_in_class()(k=2, W=np.ones((3, 3))).fit(csr_matrix(X), task="reconstruction", **FIT_KW)
        import torch.distributed as dist
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        with pytest.raises(NotImplementedError, match="one GPU"):
            MessagePassing(k=2, W="full").fit(X, task="reconstruction", **FIT_KW)


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from pybmf_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmf_hip.h")).read(), flags=re.S)
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in ENTRY_POINTS.items():
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in bmf_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(raw, name), f"{name} is missing from libbmf_hip.so"
        res, args = L.SIGNATURES[name]
        assert len(args) == n_args and res is (L._i64 if name.endswith("_work") else C.c_int)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in ENTRY_POINTS)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    p = C.c_void_p(4096)

    def start(**o):
        a = dict(W=p, ldx=16, m=100, n=80, k=5, ldn=128, Phi=p, Psi=p)
        a.update(o)
        return lib.bmf_mp_start(a["W"], a["ldx"], a["m"], a["n"], a["k"], a["ldn"], 7, 1e-2, a["Phi"], a["Psi"], None)

    def reduce(**o):
        a = dict(Phi=p, Psi=p, m=100, n=80, k=5, ldn=128, work=p, Xi=p, Ups=p, d=p, ub=p, vb=p)
        a.update(o)
        return lib.bmf_mp_reduce(a["Phi"], a["Psi"], a["m"], a["n"], a["k"], a["ldn"], 0.0, 0.0, a["work"], a["Xi"], a["Ups"], a["d"], a["ub"], a["vb"], None)

    def step(**o):
        a = dict(X=p, W=p, ldx=16, m=100, n=80, k=5, ldn=128, lr=0.2, Phi=p, Psi=p, work=p, Xi=p, Ups=p, d=p, ub=p, vb=p)
        a.update(o)
        return lib.bmf_mp_step(a["X"], a["W"], a["ldx"], a["m"], a["n"], a["k"], a["ldn"], 4.6, -4.6, a["lr"], 0.0, 0.0, a["Phi"], a["Psi"], a["work"],
                               a["Xi"], a["Ups"], a["d"], a["ub"], a["vb"], None)

    for fn, tag, ptrs in ((start, b"bmf_mp_start", ("Phi", "Psi")), (reduce, b"bmf_mp_reduce", ("Phi", "Psi", "work", "Xi", "Ups", "d")),
                          (step, b"bmf_mp_step", ("X", "Phi", "Psi", "work", "Xi", "Ups", "d"))):
        for name in ptrs:
            assert fn(**{name: None}) == -1 and tag + b": null pointer" in lib.bmf_last_error(), (tag, name)
        for over, text in ((dict(k=0), b"k=0 outside 1..64"), (dict(k=65), b"k=65 outside 1..64"), (dict(k=-2), b"outside 1..64"),
                           (dict(m=0), b"m=0, n=80 must be >= 1"), (dict(n=0, ldn=0), b"m=100, n=0 must be >= 1"), (dict(m=-4), b"must be >= 1"),
                           (dict(ldn=80), b"ldn=80 is not n=80 rounded up to 64"), (dict(ldn=192), b"ldn=192 is not n=80 rounded up to 64"),
                           (dict(ldn=64), b"is not n=80 rounded up")):
            assert fn(**over) == -1, (tag, over)
            assert tag in lib.bmf_last_error() and text in lib.bmf_last_error(), (tag, over, lib.bmf_last_error())
    assert start(ldx=3) == -1 and b"ldx=3 words do not cover ldn=128" in lib.bmf_last_error()
    assert step(ldx=3) == -1 and b"ldx=3 words do not cover ldn=128" in lib.bmf_last_error()
    assert step(lr=float("nan")) == -1 and b"NaN" in lib.bmf_last_error()
    for fn in (reduce, step):
        assert fn(ub=None) == -1 and b"come together" in lib.bmf_last_error()
        assert fn(vb=None) == -1 and b"come together" in lib.bmf_last_error()
    # the workspace: the row partials of every 64-column tile, the column partials of every 32-row segment, one maximum per finish block
    assert lib.bmf_mp_work(1, 1, 1) == 1 * 1 * 1 + 1 * 1 * 64 + 1 + 1
    assert lib.bmf_mp_work(100, 80, 5) == 2 * 100 * 5 + 4 * 5 * 128 + 2 + 3
    assert lib.bmf_mp_work(33, 130, 64) == 3 * 33 * 64 + 2 * 64 * 192 + (33 * 64 + 255) // 256 + 64 * 192 // 256
    for bad in ((0, 80, 5), (100, 0, 5), (100, 80, 0), (100, 80, 65), (-1, 80, 5)):
        assert lib.bmf_mp_work(*bad) == -1, bad
