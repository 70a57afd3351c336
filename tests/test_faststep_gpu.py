"""FastStep on the device: the evaluation pass (csrc/faststep.hip through pybmf_amd.faststep.FastStepEngine) against the NumPy fp64
evaluator of tests/test_faststep_cpu.py, and FastStep.fit() against the reference's trajectories (tests/golden/g22_faststep.*).

The gates on F / dF are not chosen in advance: they are 10 x the worst relative error measured over these very cases on an MI355X
(profiles/faststep_parity.txt holds the measured values).  Both sides are fp64 with the same formula, so the error is summation order
(and the last bits of exp / log1p).  Every test prints its figures before it asserts.

Error measures: F relative; the gradient norm-wise, max |d - d_ref| / max |d_ref| over [du | dv] (single entries of a sum of mixed
signs cancel, the line search uses the vector through dot products); U, V norm-wise likewise.
"""
import numpy as np
import pytest

from test_faststep_cpu import FIT_KW, NumpyEvaluator, fit_quietly, load_case, log_rows, make_model, train_matrix

pytestmark = pytest.mark.gpu

# 10 x the worst values measured on an MI355X (profiles/faststep_parity.txt): kernel F and dF 1.14e-13 (one cell at a = -700, where
# a last-bit difference of S moves exp(a) by 1e-13; every other case <= 4.9e-16), fit F columns 5.33e-15, fit U / V 1.37e-14
GATE_KERNEL_F = 1.2e-12
GATE_KERNEL_DF = 1.2e-12
GATE_FIT_F = 5.4e-14
GATE_FIT_UV = 1.4e-13


def device_engine(X, k, tau, U, V, mask=None):
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.faststep import FastStepEngine
    bits = BitMatrix(np.ascontiguousarray(X, dtype=np.uint8), "cuda:0")
    mbits = None if mask is None else BitMatrix(np.ascontiguousarray(mask, dtype=np.uint8), "cuda:0")
    return FastStepEngine(bits, k, tau, U, V, mask=mbits)


def compare(X, mask, k, tau, U, V, col, u, v, label):
    """Device against NumPy at one point; returns (rel F, rel dF)."""
    ref = NumpyEvaluator(X, k, tau, U, V, mask=mask)
    ref.set_factor(col)
    F0, du0, dv0, tp0, fp0 = ref.evaluate(u, v, True, True)
    eng = device_engine(X, k, tau, U, V, mask)
    eng.set_factor(col)
    F1, du1, dv1, tp1, fp1 = eng.evaluate(u, v, True, True)
    F2, du2, dv2, tp2, fp2 = eng.evaluate(u, v, True, True)
    F3 = eng.evaluate(u, v, False, False)[0]
    g0, g1 = np.concatenate([du0, dv0]), np.concatenate([du1, dv1])
    eF = abs(F1 - F0) / abs(F0)
    eG = float(np.abs(g1 - g0).max() / max(np.abs(g0).max(), np.finfo(np.float64).tiny))
    print(f"faststep parity {label}: F {F0:.6e} rel {eF:.2e}  dF max {np.abs(g0).max():.3e} rel {eG:.2e}  TP/FP {tp1}/{fp1} (NumPy {tp0}/{fp0})")
    assert (tp1, fp1) == (tp0, fp0)
    # two calls on the same input: the same bits (no atomics, fixed-order sums); F alone takes the same per-cell path
    assert F1.hex() == F2.hex() == F3.hex() and (tp1, fp1) == (tp2, fp2)
    assert du1.tobytes() == du2.tobytes() and dv1.tobytes() == dv2.tobytes()
    return eF, eG


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_kernel_at_the_stored_points(name):
    case = load_case(name)
    m = case["X"].shape[0]
    mask = None if case["W"] == "full" else case["pattern"]
    for i, p in enumerate(case["points"]):
        eF, eG = compare(case["X"], mask, case["k"], case["tau"], p["U"], p["V"], p["k"], p["params"][:m], p["params"][m:], f"{name}/p{i}")
        # ... and against the reference's own numbers
        eng = device_engine(case["X"], case["k"], case["tau"], p["U"], p["V"], mask)
        eng.set_factor(p["k"])
        F, du, dv, _, _ = eng.evaluate(p["params"][:m], p["params"][m:], True, False)
        rF = abs(F - p["F"]) / abs(p["F"])
        rG = np.abs(np.concatenate([du, dv]) - p["dF"]).max() / np.abs(p["dF"]).max()
        print(f"faststep parity {name}/p{i} vs reference: F rel {rF:.2e}  dF rel {rG:.2e}")
        assert max(eF, rF) <= GATE_KERNEL_F and max(eG, rG) <= GATE_KERNEL_DF


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k", [1, 4, 64])
@pytest.mark.parametrize("shape", [(1, 1), (127, 33), (130, 257)])
def test_kernel_at_ragged_shapes(shape, k, masked):
    """Tiles cut by both edges; factor entries at the 1e-5 floor; S - tau from -20 to 700, so both branches of the softplus and of
    the sigmoid run far out."""
    m, n = shape
    rng = np.random.RandomState(1000 * m + 10 * k + int(masked))
    tau = 20.0
    U, V = rng.rand(m, k), rng.rand(n, k)
    U[rng.rand(m, k) < 0.1] = 0.0
    V[rng.rand(n, k) < 0.1] = 0.0
    U[-1, -1] = V[-1, -1] = 0.0
    U[0, 0] = V[0, 0] = 1.0
    c = np.sqrt((700.0 + tau) / (U @ V.T).max())
    U, V = np.maximum(U * c, 1e-5), np.maximum(V * c, 1e-5)
    S = U @ V.T
    assert (U == 1e-5).any() or m * k == 1
    assert (V == 1e-5).any() or n * k == 1
    assert 690.0 <= (S - tau).max() <= 710.0
    X = (rng.rand(m, n) < 0.5).astype(np.uint8)
    mask = (rng.rand(m, n) < 0.6).astype(np.uint8) if masked else None
    col = k // 2
    u, v = U[:, col] * rng.uniform(0.5, 1.0, m), V[:, col] * rng.uniform(0.5, 1.0, n)
    eF, eG = compare(X, mask, k, tau, U, V, col, u, v, f"{m}x{n} k={k} mask={int(masked)}")
    assert eF <= GATE_KERNEL_F and eG <= GATE_KERNEL_DF


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fit_follows_the_reference(name):
    case = load_case(name)
    model = fit_quietly(make_model(case), train_matrix(case))
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want)
    assert [r[:3] for r in got] == [r[:3] for r in want]
    G, Wt = np.array(got), np.array(want)
    eF = float(np.abs(G[:, 3:5] / Wt[:, 3:5] - 1).max())
    eU = float(np.abs(model.U - case["U"]).max() / np.abs(case["U"]).max())
    eV = float(np.abs(model.V - case["V"]).max() / np.abs(case["V"]).max())
    tp, fp = model._counts
    fn = int(case["X"].sum()) - tp
    counts = [tp, fp, fn, case["X"].size - tp - fp - fn]
    print(f"faststep fit {name}: {len(got)} rows, F columns rel {eF:.2e}, U rel {eU:.2e}, V rel {eV:.2e}, counts {counts} (reference {case['counts']})")
    assert counts == case["counts"]
    assert np.abs(G[:, 5:] - Wt[:, 5:]).max() <= 1e-12     # scores: ratios of equal integer counts, row by row
    assert eF <= GATE_FIT_F and max(eU, eV) <= GATE_FIT_UV
    Ud, Vd = model._engine.factors()
    assert np.array_equal(Ud, model.U) and np.array_equal(Vd, model.V)
    X_pd = np.asarray(model.X_pd.todense())
    assert (int((X_pd & case["X"]).sum()), int((X_pd & (1 - case["X"])).sum())) == (tp, fp)


def test_larger_fit_keeps_its_invariants():
    """6040 x 3706, k = 8, 1.0 M ones, two rounds of four steps per factor: the F of the last row is what a fresh evaluation at the
    final factors returns, and the counts are those of the real product (device_ops.product_csr) thresholded at tau."""
    import contextlib
    import io
    from pybmf_amd.device_ops import product_csr
    from pybmf_amd.models import FastStep
    m, n, k = 6040, 3706, 8
    rng = np.random.RandomState(7)
    X = np.zeros(m * n, dtype=np.uint8)
    X[rng.choice(m * n, size=1_000_000, replace=False)] = 1
    X = X.reshape(m, n)
    with contextlib.redirect_stdout(io.StringIO()):
        model = FastStep(k=k, max_round=1, max_iter=3, seed=3)
        model.fit(X, **FIT_KW)
    rows = log_rows(model)
    assert rows[-1][:2] == [2.0, float(k - 1)] and len(rows) <= 2 * k * 4
    eng = model._engine
    eng.set_factor(k - 1)
    F, _, _, tp, fp = eng.evaluate(model.U[:, k - 1], model.V[:, k - 1], False, True)
    assert F == rows[-1][3] == rows[-1][4]
    assert (tp, fp) == model._counts
    S = product_csr(model.U, model.V, boolean=False, device="cuda:0")
    pd = np.asarray(S.todense()) > model.tau
    want = (int((pd & (X == 1)).sum()), int((pd & (X == 0)).sum()))
    print(f"faststep larger fit: F {F:.6e}, TP/FP {tp}/{fp}, thresholded real product {want[0]}/{want[1]}")
    assert (tp, fp) == want
