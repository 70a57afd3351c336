"""BinaryMFThresholdExColumnwise.fit on the device against the NumPy restatement's fit (tests/thresh_cols_ref.py).  The fixtures are
checked on the CPU (test_thresh_cols_cpu.py) to keep every Armijo / curvature comparison and every thresholded entry off its tie by a
margin far above the kernels' 1e-11, so both fits take the same path: same n_iter, same evaluation counts, the same integer counts."""
import contextlib
import io
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import thresh_cols_ref as R  # noqa: E402

FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def fit(X, U, V, us, vs, lam, verbose=False, X_val=None, X_test=None, max_iter=R.MAX_ITER):
    """(model, captured output)"""
    from pybmf_amd.models.BinaryMFThresholdExColumnwise import BinaryMFThresholdExColumnwise
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model = BinaryMFThresholdExColumnwise(k=U.shape[1], U=U.copy(), V=V.copy(), W="full", us=us, vs=vs, lamda=lam, max_iter=max_iter, seed=1)
        model.fit(csr_matrix(X), None if X_val is None else csr_matrix(X_val), None if X_test is None else csr_matrix(X_test), verbose=verbose, **FIT_KW)
    return model, buf.getvalue()


def check_against(model, ref, U, V, sets=("train",)):
    log = model.logs["updates"]
    k = U.shape[1]
    assert model.n_iter == ref["n_iter"] and len(log) == ref["n_iter"] + 1
    assert [c for c in log.columns] == [("", "", "time"), ("", "", "iter"), ("", "", "F")] + [(s, 0, mt) for s in sets for mt in R.METRICS]
    assert list(log[("", "", "iter")]) == list(range(ref["n_iter"] + 1))
    np.testing.assert_allclose(np.array(log[("", "", "F")], dtype=np.float64), ref["F"], rtol=1e-9)
    x, want = np.concatenate([model.us, model.vs]), ref["x"][-1]
    assert model.us.dtype == np.float64 and model.us.shape == (k,) and model.vs.shape == (k,)
    assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max()
    for s in sets:
        got = [[log[(s, 0, mt)][t] for mt in R.METRICS] for t in range(len(log))]
        assert got == ref["scores"][s], s          # equal integer counts behind them: the same host formula on both sides
    assert (model.U == U).all() and (model.V == V).all()
    assert np.array_equal(np.asarray(model.X_pd.todense()) != 0, R.product(U, V, want[:k], want[k:]))


@pytest.mark.parametrize("k,lam", R.FIXTURES)
def test_fit_equals_restatement(gpu, k, lam):
    X, U, V, us, vs, ref = R.fixture(k, lam)
    model, _ = fit(X, U, V, tuple(us), list(vs), lam)
    check_against(model, ref, U, V)


@pytest.mark.parametrize("k,lam", [(5, 10), (64, 5)])
def test_verbose_output(gpu, k, lam):
    """The recorded layout: the scalar model's four lines, then `threshold update :` with the old and the new x on two lines and
    `threshold update direction :` with alpha * pk on one; 2 k numbers per list; the evaluation counts of the restatement's searches."""
    X, U, V, us, vs, ref = R.fixture(k, lam)
    model, text = fit(X, U, V, us, vs, lam, verbose=True)
    lines = [ln for ln in text.splitlines() if ln.startswith("[I]   Wolfe") or ln.startswith("[I]     ") or ln.startswith("[I]       ")]
    assert len(lines) == 9 * ref["n_iter"]
    num2, num4 = r"-?\d+\.\d{2}", r"-?\d+\.\d{4}"
    for it in range(ref["n_iter"]):
        b = lines[9 * it: 9 * it + 9]
        fc, gc = ref["evals"][it]
        assert b[0] == "[I]   Wolfe line search iter         : {}".format(it + 1)
        assert b[1] == "[I]     num of function evals        : {}".format(fc)
        assert b[2] == "[I]     num of gradient evals        : {}".format(gc)
        assert re.fullmatch(r"\[I\]     function value update        : \d+\.\d{3} -> \d+\.\d{3}", b[3]), b[3]
        assert b[4] == "[I]     threshold update             :"
        assert re.fullmatch(r"\[I\]       \[(%s, ){%d}%s\]" % (num2, 2 * k - 1, num2), b[5]), b[5]
        assert re.fullmatch(r"\[I\]     ->\[(%s, ){%d}%s\]" % (num2, 2 * k - 1, num2), b[6]), b[6]
        assert b[7] == "[I]     threshold update direction   :"
        assert re.fullmatch(r"\[I\]       \[(%s, ){%d}%s\]" % (num4, 2 * k - 1, num4), b[8]), b[8]
        assert b[5][10:] == "[" + ", ".join("{:.2f}".format(v) for v in ref["x"][it]) + "]"      # the old x is the previous row's
    check_against(model, ref, U, V)


@pytest.mark.parametrize("k", [5, 33])
def test_pipeline_from_simple_threshold(gpu, k):
    """SimpleThreshold(columnwise, randomize) -> this model on its us, vs TUPLES: row 0 is scored at the best trial's thresholds, F
    starts at the restatement's value there and never increases."""
    from pybmf_amd.models.SimpleThreshold import SimpleThreshold
    X, U, V, _, _, _ = R.fixture(k, 10)
    with contextlib.redirect_stdout(io.StringIO()):
        st = SimpleThreshold(U=U.copy(), V=V.copy(), by_metric="F1", columnwise=True, randomize=True, n_trials=50, seed=2024)
        st.fit(X.copy(), verbose=False, **FIT_KW)
    assert isinstance(st.us, tuple) and len(st.us) == k
    model, _ = fit(X, U, V, st.us, st.vs, 10, max_iter=3)
    log = model.logs["updates"]
    tp, fp = (int(v) for v in st.counts_[st.best_iter - 1])
    fn = int(X.sum()) - tp
    assert [log[("train", 0, mt)][0] for mt in R.METRICS] == R.scores(tp, fp, fn, X.size - tp - fp - fn)
    x0 = np.concatenate([np.asarray(st.us), np.asarray(st.vs)])
    Fs = np.array(log[("", "", "F")], dtype=np.float64)
    assert Fs[0] == pytest.approx(R.F(X.astype(np.float64), U, V, x0, 10), rel=1e-9)
    assert len(Fs) >= 2 and (np.diff(Fs) <= 0).all()


def test_val_and_test_sets(gpu):
    k, lam = 17, 10
    X, U, V, us, vs, _ = R.fixture(k, lam)
    rs = np.random.RandomState(3)
    Xv, Xt = (X ^ (rs.rand(*X.shape) < 0.1)).astype(np.uint8), (X & (rs.rand(*X.shape) < 0.5)).astype(np.uint8)
    ref = R.fit(X, U, V, us, vs, lam, max_iter=R.MAX_ITER, extra={"val": Xv, "test": Xt})
    model, _ = fit(X, U, V, us, vs, lam, X_val=Xv, X_test=Xt)
    check_against(model, ref, U, V, sets=("train", "val", "test"))


def test_a_list_of_ones_over_the_budget_is_refused(gpu, monkeypatch):
    """Where the scalar model falls back to the tile product, this one refuses: it has no such route."""
    X, U, V, us, vs, _ = R.fixture(5, 10)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (4096, 1 << 30))
    with pytest.raises(NotImplementedError, match="does not fit the memory budget"):
        fit(X, U, V, us, vs, 10)
