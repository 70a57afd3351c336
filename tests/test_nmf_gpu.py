"""NMFSklearn on the GPU against the fixture g32_nmf (the reference's NMFSklearn, i.e. scikit-learn's coordinate-descent NMF).

The gate for U, V, the initial factors and reconstruction_err_ is 1e-4 of the largest entry: the project's gate for parity with an fp64
reference through 24-bit operands (the Gram runs on the fp32 matrix cores, X V on the factor's three int8 digit planes).  For the
NNDSVD initialisers the operand rounding 2^-23 times the 1 / 0.05 amplification of the asserted singular gaps is 2e-6, 50 times inside
the gate.  n_iter_ must be equal and X_pd bit-identical: the fixture was made so that neither hangs on a rounding
(tests/golden/make_golden_nmf.py).
"""
import contextlib
import io
import warnings

import numpy as np
import pytest
from scipy.sparse import csr_matrix, issparse

from test_nmf_cpu import CASES, FIT_KW, NNDSVD_CASES, close, fit_quietly, load_case, make_model

pytestmark = pytest.mark.gpu

GATE = 1e-4
_fits = {}


def fitted(name):
    """The case through the class on the device, fitted once and shared."""
    if name not in _fits:
        c = load_case(name)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            model = fit_quietly(make_model(c), c["X"])
        _fits[name] = (model, [w for w in caught if issubclass(w.category, RuntimeWarning)])
    return _fits[name]


@pytest.mark.parametrize("name", CASES)
def test_class_reproduces_the_fixture(name):
    c = load_case(name)
    model, warned = fitted(name)
    U, V = np.asarray(model.U.todense()), np.asarray(model.V.todense())
    scale = lambda A: max(np.abs(A).max(), 1e-300)  # noqa: E731
    print(f"case {name}: n_iter {model.n_iter_} (fixture {c['n_iter']}), max |dU| / max|U| = {np.abs(U - c['U']).max() / scale(c['U']):.3g}, "
          f"|dV| = {np.abs(V - c['V']).max() / scale(c['V']):.3g}, |dU0| = {np.abs(model.U_init - c['W0']).max() / scale(c['W0']):.3g}, "
          f"|dV0| = {np.abs(model.V_init - c['H0'].T).max() / scale(c['H0']):.3g}, err {model.model.reconstruction_err_:.9g} "
          f"(fixture {c['reconstruction_err']:.9g})")
    assert model.n_iter_ == c["n_iter"] == model.model.n_iter_
    assert issparse(model.U) and issparse(model.V) and model.logs == {}
    assert close(U, c["U"], GATE) and close(V, c["V"], GATE)
    assert abs(model.model.reconstruction_err_ - c["reconstruction_err"]) <= GATE * max(c["reconstruction_err"], 1e-300) or name == "j"
    if name == "j":
        assert model.model.reconstruction_err_ == 0.0 and not U.any() and not V.any()
    assert np.array_equal(np.asarray(model.X_pd.todense()).astype(np.uint8), c["X_pd"])
    assert model.model.n_components_ == c["k"] and np.array_equal(model.model.components_, V.T)
    assert bool([w for w in warned if "maximum number of iterations" in str(w.message)]) == (name == "i")
    if name in NNDSVD_CASES:
        assert close(model.U_init, c["W0"], GATE) and close(model.V_init, c["H0"].T, GATE)
        for got, want in ((model.U_init, c["W0"]), (model.V_init, c["H0"].T)):
            flipped = (got == 0) != (want == 0)
            if name == "g":   # (the one case with entries at the truncation threshold 1e-6: a flipped one is that small on both sides)
                assert np.abs(got[flipped]).max(initial=0) <= 2e-6 and np.abs(want[flipped]).max(initial=0) <= 2e-6
            else:
                assert not flipped.any()
    else:
        assert close(model.U_init, c["W0"], 1e-12) and close(model.V_init, c["H0"].T, 1e-12)   # host draws / given matrices


def test_custom_start_from_the_fixture_init_reproduces_the_nndsvd_fit():
    """The sweeps alone: from the fixture's own initial factors the fit must land where the 'nndsvd' fit lands."""
    c = load_case("a")
    model = fit_quietly(make_model(c, init_method="custom", U=c["W0"].copy(), V=c["H0"].T.copy()), c["X"])
    U, V = np.asarray(model.U.todense()), np.asarray(model.V.todense())
    assert model.n_iter_ == c["n_iter"]
    assert close(U, c["U"], GATE) and close(V, c["V"], GATE)
    assert np.array_equal(np.asarray(model.X_pd.todense()).astype(np.uint8), c["X_pd"])
    same, _ = fitted("a")
    assert close(U, np.asarray(same.U.todense()), GATE) and close(V, np.asarray(same.V.todense()), GATE)


def test_engine_products_and_rec_error_against_numpy():
    """bits_product on a thin matrix of both signs wider than one 64-column block, both orientations, and rec_error of given factors."""
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.nmf import NMFEngine, bits_product
    c = load_case("g")
    X = c["X"].astype(np.float64)
    bits = BitMatrix(c["X"], "cuda:0")
    rng = np.random.RandomState(3)
    for transposed, rows in ((False, X.shape[1]), (True, X.shape[0])):
        T = rng.standard_normal((rows, 75)) * np.logspace(-3, 3, 75)
        want = (X.T if transposed else X) @ T
        got = bits_product(bits, T, transposed)
        # a 24-bit operand per column and an fp32 result: 2^-23 of the column's largest entry times the ones in a row of X
        bound = 2.0 ** -22 * np.abs(T).max(axis=0) * (X.T if transposed else X).sum(axis=1).max() + 2.0 ** -23 * np.abs(want).max(axis=0)
        assert (np.abs(got - want).max(axis=0) <= bound).all()
    eng = NMFEngine(bits, c["k"])
    eng.load_factors(c["U"], c["V"])
    want = ((X - c["U"] @ c["V"].T) ** 2).sum()
    assert abs(eng.rec_error() - want) <= 1e-5 * X.sum()


def test_nmf_start_feeds_the_thresholding_model():
    """The flow of the reference's notebooks: NMFSklearn's factors as the 'custom' start of BinaryMFThreshold."""
    from pybmf_amd.models import BinaryMFThreshold
    c = load_case("a")
    nmf, _ = fitted("a")
    with contextlib.redirect_stdout(io.StringIO()):
        model = BinaryMFThreshold(k=c["k"], U=nmf.U, V=nmf.V, W="full", u=0.5, v=0.5, lamda=10, min_diff=1e-3, max_iter=5, init_method="custom")
        model.fit(csr_matrix(c["X"].astype(np.float64)), **FIT_KW)
    assert "updates" in model.logs and len(model.logs["updates"]) >= 1
