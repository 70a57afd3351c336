"""MessagePassing fits on the GPU against the NumPy restatement (tests/mp_ref.py) on its fixtures: the engine and the model class give
the oracle's n_iter, U, V and confusion counts on train / val / test under both tasks; the final marginals stay within 64 x the
largest difference between the oracle run with forward sums and the oracle run with reversed sums (both computed here, on the CPU;
the factor absorbs the device's third summation order); two fits from one seed are byte-identical."""
import contextlib
import io

import numpy as np
import pytest

import mp_ref as R

pytestmark = pytest.mark.gpu

FIT_KW = dict(show_logs=False, show_result=False, save_model=False, verbose=False)


def gate_of(name):
    fwd, rev = R.fixture(name)[3], R.fixture(name, "reversed")[3]
    assert rev["n_iter"] == fwd["n_iter"]
    return 64 * max(np.abs(fwd["Xi"] - rev["Xi"]).max(), np.abs(fwd["Ups"] - rev["Ups"]).max())


def engine_fit(X, k, pattern, seed=R.SEED):
    eng = R.make_engine(X, k, pattern, lr=R.CONSTS["lr"])
    res = R.fit(X, k, tol=R.TOL, max_iter=R.MAX_ITER, seed=seed, engine=eng)
    res["decisions"] = eng.decisions()
    return res


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_engine_fit_matches_the_oracle(name):
    X, clean, pattern, ref = R.fixture(name)
    R.check_fixture(ref)
    k = ref["U"].shape[1]
    got = engine_fit(X, k, pattern)
    gate = gate_of(name)
    diff = max(np.abs(got["Xi"] - ref["Xi"]).max(), np.abs(got["Ups"] - ref["Ups"]).max())
    print(f"{name}: n_iter {got['n_iter']} (oracle {ref['n_iter']}), |marginals - oracle| max {diff:.3e}, gate {gate:.3e}")
    assert got["n_iter"] == ref["n_iter"] and got["converged"]
    assert np.array_equal(got["U"], ref["U"]) and np.array_equal(got["V"], ref["V"])
    assert np.array_equal(got["decisions"][0], ref["U"]) and np.array_equal(got["decisions"][1], ref["V"])
    assert diff <= gate
    again = engine_fit(X, k, pattern)
    assert got["Xi"].tobytes() == again["Xi"].tobytes() and got["Ups"].tobytes() == again["Ups"].tobytes() and got["diffs"] == again["diffs"]


@pytest.mark.parametrize("task", ["reconstruction", "prediction"])
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_model_fit_matches_the_oracle(name, task):
    from pybmf_amd.models import MessagePassing
    X, clean, pattern, ref = R.fixture(name)
    k = ref["U"].shape[1]
    rs = np.random.RandomState(9)
    hidden = ~pattern if pattern is not None else rs.rand(*X.shape) < 0.2
    val, test = hidden & (rs.rand(*X.shape) < 0.5), hidden & ~(rs.rand(*X.shape) < 0.5)
    with contextlib.redirect_stdout(io.StringIO()):
        model = MessagePassing(k=k, W="mask" if pattern is not None else "full", tol=R.TOL, max_iter=R.MAX_ITER, seed=R.SEED, **R.CONSTS)
        model.fit(R.train_csr(X, pattern), R.train_csr(X, val), R.train_csr(X, test), task=task, **FIT_KW)
        model.evaluate(df_name="counts", metrics=["TP", "FP", "FN", "TN"])
    assert model.n_iter == ref["n_iter"] and model.converged is True
    assert np.array_equal(model.U, ref["U"]) and np.array_equal(model.V, ref["V"]) and model.U.dtype == np.float64
    gate = gate_of(name)
    assert max(np.abs(model.marginal_U - ref["Xi"]).max(), np.abs(model.marginal_V - ref["Ups"]).max()) <= gate
    up = model.logs["updates"]
    assert [int(v) for v in up.iloc[:, 1]] == list(range(1, ref["n_iter"] + 1))
    assert float(up.iloc[-1, 2]) < R.TOL <= min(float(v) for v in up.iloc[:-1, 2])
    # the counts: the whole matrices under 'reconstruction', the non-zero stored entries of each set under 'prediction' (the rule of
    # ContinuousModel._make_scorers for every continuous model)
    pd = R.boolean_product(ref["U"], ref["V"])
    want = []
    for gt in (X if pattern is None else X & pattern, X & val, X & test):
        want += list(R.confusion(gt, pd, gt if task == "prediction" else None))
    got = [int(v) for v in model.logs["counts"].values.tolist()[0][1:]]
    assert got == want
    row = [float(v) for v in model.logs["boolean"].values.tolist()[0][1:]]
    assert len(model.logs["boolean"]) == 1 and len(row) == 12
    for s in range(3):
        assert row[4 * s: 4 * s + 4] == pytest.approx(R.scores(want[4 * s: 4 * s + 4]), rel=1e-12, abs=0)
    assert np.array_equal(np.asarray(model.X_pd.todense()) != 0, pd)
