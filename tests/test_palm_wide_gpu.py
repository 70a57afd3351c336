"""ELBMF and PRIMP at a rank 64 < k <= 128 on the GPU (pybmf_amd/palm_wide.py, csrc/palm_wide.hip) against the reference's own numbers
(golden g34: tests/golden/make_golden_palm_wide.py) and against the oracle on another shape.  The gates are those of
tests/test_palm_gpu.py: single steps 1e-5, loops 1e-4 on factors and logged scalars, Boolean counts exact (the fixture keeps every
entry at least 1e-3 from the 0.5 threshold at every iteration)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402

FIT = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
LOOP = dict(reg_l1=0.01, reg_l2=0.02, reg_growth=1.05)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        yield


def relf(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / max(np.linalg.norm(np.asarray(b, dtype=np.float64)), 1e-300))


def planted(k):
    return np.kron(np.eye(k), np.ones((3, 1))), np.kron(np.eye(k), np.ones((2, 1)))


def load_g34(golden_dir):
    """(z, steps, meta, {k: (X, U0, V0)}); the start rebuilt from its stored grid indices as the generator builds it."""
    z = np.load(os.path.join(golden_dir, "g34_palm_wide.npz"))
    steps = np.load(os.path.join(golden_dir, "g34_palm_wide_steps.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g34_palm_wide.json")))
    data = {}
    for k in meta["ks"]:
        m, n, _ = meta[f"k{k}"]["shape"]
        PU, PV = planted(k)
        U0 = 0.7 * PU + 0.2 * z[f"k{k}_U0_grid"].astype(np.float64) / 256.0
        V0 = 0.7 * PV + 0.2 * z[f"k{k}_V0_grid"].astype(np.float64) / 256.0
        data[k] = (np.unpackbits(z[f"k{k}_X"], axis=1)[:, :n].astype(np.uint8), U0, V0)
    return z, steps, meta, data


@pytest.fixture(scope="module")
def g34(golden_dir):
    return load_g34(golden_dir)


def fit_elbmf(X, U0, V0, k, beta, max_iter, min_diff, W="full", **kw):
    from pybmf_amd.models import ELBMF
    with quiet():
        mdl = ELBMF(k=k, U=U0.copy(), V=V0.copy(), W=W, init_method="custom", beta=beta, max_iter=max_iter, min_diff=min_diff, tol=0.0, **LOOP)
        mdl.fit(X, **dict(FIT, **kw))
    return mdl


def check_loop(mdl, g, U, V):
    from pybmf_amd.palm_wide import WidePalmEngine
    assert isinstance(mdl._eng, WidePalmEngine)
    want = np.array(g["updates"]["rows"], dtype=np.float64)
    got = np.array([[float(v) for v in r[1:]] for r in mdl.logs["updates"].values.tolist()])
    assert [tuple(str(x) for x in c) for c in mdl.logs["updates"].columns][1:] == [tuple(c) for c in g["updates"]["columns"]]
    assert got.shape == want.shape                                                   # (stops at the recorded iteration)
    np.testing.assert_allclose(got[:, :7], want[:, :7], rtol=1e-4)
    np.testing.assert_allclose(got[:, 7:], want[:, 7:], rtol=1e-12, atol=1e-15)      # scores from exact integer counts
    assert relf(mdl.U, U) < 1e-4 and relf(mdl.V, V) < 1e-4, (relf(mdl.U, U), relf(mdl.V, V))
    assert list(mdl.counts[-1]) == g["counts"]


def test_elbmf_single_steps_against_g34(g34):
    from pybmf_amd.models.ELBMF import update_U
    z, steps, meta, data = g34
    X, U0, V0 = data[72]
    U_prev = U0 + 0.05 * z["k72_U_prev_grid"].astype(np.float64) / 64.0
    for i, p in enumerate(meta["steps"]):
        Un, Ul = update_U(X, U0, V0, None, p["reg_l1"], p["reg_l2"], p["beta"], U_prev)
        assert relf(Un, steps[f"k72_step{i}_U"]) < 1e-5, (i, relf(Un, steps[f"k72_step{i}_U"]))
        assert np.array_equal(Ul, U0)
        Vn, _ = update_U(np.ascontiguousarray(X.T), V0, steps[f"k72_step{i}_U"].astype(np.float64), None, p["reg_l1"], p["reg_l2"], p["beta"], V0)
        assert relf(Vn, steps[f"k72_step{i}_V"]) < 1e-5, (i, relf(Vn, steps[f"k72_step{i}_V"]))


@pytest.mark.parametrize("tag", ["palm", "ipalm"])
@pytest.mark.parametrize("k", [65, 72, 128])
def test_elbmf_class_matches_reference_loop(g34, k, tag):
    """The class loop against the reference's log and final factors at the gates of tests/test_palm_gpu.py.

    What this holds the engine to at k = 65, beta = 0: the reference's prox has no dead zone at 0 -- an exact-zero entry with argument
    x = -eta grad goes to 0 for x >= 0 and to (x + kai) / (1 + lam) ~ kai = 2e-3 for x < 0 -- and on near-Boolean factors a few such
    arguments per iteration are of size 1e-8.  One cell on the other side is 1.4e-4 of ||U||_F here, above the gate by itself.  With
    X V from the 24-bit digit planes alone (off by up to 6e-8 per entry of a column that reaches 1) the cell of iteration 12 went the
    other way (U at 1.04e-4); with the remainder planes (WidePalmEngine.refresh) all six cases stay within 2e-7 at every iteration."""
    z, _, meta, data = g34
    g = meta[f"k{k}"][tag]
    mdl = fit_elbmf(*data[k], k, g["beta"], g["max_iter"], g["min_diff"])
    check_loop(mdl, g, z[f"k{k}_{tag}_U"], z[f"k{k}_{tag}_V"])
    assert mdl.X_pd.sum() == g["counts"][0] + g["counts"][1]


def test_elbmf_stops_at_the_recorded_iteration(g34):
    z, _, meta, data = g34
    g = meta["k72"]["stop"]
    assert g["n_iter"] < g["max_iter"]
    mdl = fit_elbmf(*data[72], 72, g["beta"], g["max_iter"], g["min_diff"])
    assert mdl.n_iter == g["n_iter"]
    check_loop(mdl, g, z["k72_stop_U"], z["k72_stop_V"])


def test_elbmf_under_a_mask_and_weights_against_g34(g34):
    from scipy.sparse import csr_matrix
    from pybmf_amd.models.ELBMF import update_U
    z, steps, meta, data = g34
    X, U0, V0 = data[72]
    m, n = X.shape
    W01 = np.unpackbits(z["k72_W01"], axis=1)[:, :n].astype(np.float64)
    Ws = {"W01": W01, "Wr": z["k72_Wr_levels"].astype(np.float64) / 2.0}
    U_prev = U0 + 0.05 * z["k72_U_prev_grid"].astype(np.float64) / 64.0
    for i, p in enumerate(meta["masked_steps"]):
        W = Ws[p["W"]]
        Un, Ul = update_U(X, U0, V0, W, p["reg_l1"], p["reg_l2"], p["beta"], U_prev)
        Vn, _ = update_U(np.ascontiguousarray(X.T), V0, U0, np.ascontiguousarray(W.T), p["reg_l1"], p["reg_l2"], p["beta"], V0)
        ru, rv = relf(Un, steps[f"k72_mstep{i}_U"]), relf(Vn, steps[f"k72_mstep{i}_V"])
        assert ru < 1e-5 and rv < 1e-5, (i, ru, rv)
        assert np.array_equal(Ul, U0)
    r, c = np.nonzero(W01)
    Xs = csr_matrix((X[r, c].astype(np.float64), (r, c)), shape=X.shape)
    for tag in ("mpalm", "mipalm"):
        g = meta["k72"][tag]
        mdl = fit_elbmf(Xs, U0, V0, 72, g["beta"], g["max_iter"], g["min_diff"], W="mask")
        check_loop(mdl, g, z[f"k72_{tag}_U"], z[f"k72_{tag}_V"])


def _fixture_rand(monkeypatch, z):
    """torch.rand replaced by the reference's own draws for primp(seed=3), as in tests/test_palm_gpu.py."""
    draws = [torch.from_numpy(z["k72_primp_seed3_U0"].copy()), torch.from_numpy(z["k72_primp_seed3_Vt0"].copy())]

    def fake_rand(*shape, dtype=None, **kw):
        t = draws.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(dtype) if dtype is not None else t
    monkeypatch.setattr(torch, "rand", fake_rand)


def test_primp_against_g34(g34, monkeypatch):
    import importlib
    P = importlib.import_module("pybmf_amd.models.PRIMP")
    from pybmf_amd.models import PRIMP
    z, steps, meta, data = g34
    X, U0, V0 = data[72]
    m, n = X.shape
    Vt0 = np.ascontiguousarray(V0.T)
    U_prev = U0 + 0.05 * z["k72_U_prev_grid"].astype(np.float64) / 64.0
    for i, p in enumerate(meta["primp_steps"]):
        Un = P.elbmf_step_ipalm(X, U0, Vt0, U_prev, p["l1reg"], p["l2reg"], p["tau"], p["beta"])
        assert relf(Un, steps[f"k72_pstep{i}_U"]) < 1e-5, (i, relf(Un, steps[f"k72_pstep{i}_U"]))
    for tag in ("primp64", "primp64_b0"):
        g = meta[tag]
        seen = []
        U, Vt = P.elbmf_ipalm(X, U0, Vt0, 0.01, 0.0, lambda t: 1.02 ** t, g["maxiter"], 1e-8, g["beta"],
                              lambda t, Uc, Vc, fn: seen.append((t, Uc.shape, Vc.shape, float(fn))))
        assert Vt.shape == z[f"k72_{tag}_Vt"].shape
        assert relf(U, z[f"k72_{tag}_U"]) < 1e-4 and relf(Vt, z[f"k72_{tag}_Vt"]) < 1e-4, (tag, relf(U, z[f"k72_{tag}_U"]))
        assert seen[-1][3] == pytest.approx(g["fn_final"], rel=1e-4) and seen[0][1:3] == (U.shape, Vt.shape)
        # rounding: identical wherever the reference's factor is more than 1e-4 from the 0.5 threshold
        Ur, Vtr = np.unpackbits(z[f"k72_{tag}_Ur"], axis=1)[:, :72].astype(bool), np.unpackbits(z[f"k72_{tag}_Vtr"], axis=1)[:, :n].astype(bool)
        far_u, far_v = np.abs(z[f"k72_{tag}_U"].astype(np.float64) - 0.5) > 1e-4, np.abs(z[f"k72_{tag}_Vt"].astype(np.float64) - 0.5) > 1e-4
        assert np.array_equal((U > 0.5)[far_u], Ur[far_u]) and np.array_equal((Vt > 0.5)[far_v], Vtr[far_v])
    # tensors in -> tensors out, dtype kept
    Ut, Vtt = P.elbmf_ipalm(torch.from_numpy(X.astype(np.float32)), torch.from_numpy(U0).float(), torch.from_numpy(Vt0).float(), 0.01, 0, lambda t: 1.02 ** t,
                            3, 1e-8, 1e-4, None)
    assert isinstance(Ut, torch.Tensor) and Ut.dtype == torch.float32 and tuple(Vtt.shape) == (72, n)
    # primp(seed=3) and the class: the reference's own draws -> the same rounded factors (up to cells at the threshold)
    want_u = np.unpackbits(z["k72_primp_seed3_Ur"], axis=1)[:, :72]
    want_v = np.unpackbits(z["k72_primp_seed3_Vtr"], axis=1)[:, :n]
    _fixture_rand(monkeypatch, z)
    Ur, Vtr = P.primp(torch.from_numpy(X.astype(np.float32)), 72, l1reg=0.01, maxiter=25, beta=1e-4, seed=3)
    assert isinstance(Ur, torch.Tensor) and tuple(Vtr.shape) == (72, n)
    assert (Ur.numpy().astype(np.uint8) == want_u).mean() > 0.999 and (Vtr.numpy().astype(np.uint8) == want_v).mean() > 0.999
    _fixture_rand(monkeypatch, z)
    with quiet():
        mdl = PRIMP(k=72, reg=0.01, reg_growth=1.02, max_iter=25, min_diff=1e-8, beta=1e-4, seed=3)
        mdl.fit(X, **FIT)
    assert (mdl.U.astype(np.uint8) == want_u).mean() > 0.999 and (mdl.V.T.astype(np.uint8) == want_v).mean() > 0.999
    assert set(np.unique(mdl.U)) <= {0.0, 1.0} and len(mdl.logs["boolean"]) == 1


def test_elbmf_k100_against_the_oracle():
    """k = 100 on a 300 x 200 planted matrix, 8 iterations, beta > 0: factors, error, gaps and counts against the oracle at 1e-4."""
    from pybmf_amd import _lib as L
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.palm_wide import WidePalmEngine
    rs = np.random.RandomState(34)
    k = 100
    PU, PV = planted(k)
    X = PU @ PV.T
    X = np.where(rs.rand(*X.shape) < 0.01, 1 - X, X).astype(np.uint8)
    assert X.shape == (300, 200)
    # a start that keeps every entry away from the 0.5 threshold at every iteration, found on the host alone (as the g34 generator does)
    for seed in range(100):
        r2 = np.random.RandomState(1000 + seed)
        U0, V0 = 0.7 * PU + 0.2 * r2.rand(*PU.shape), 0.7 * PV + 0.2 * r2.rand(*PV.shape)
        near, U, V, Ul, Vl = np.inf, U0, V0, U0, V0
        for t in range(8):
            l1, l2 = 0.02, 0.05 * 1.1 ** t
            (Un, Ul), (Vn, Vl) = orc.elbmf_update(X.astype(float), U, V, None, l1, l2, 0.15, Ul, True), orc.elbmf_update(X.T.astype(float), V, U, None, l1, l2, 0.15, Vl, True)
            U, V = Un, Vn
            near = min(near, np.abs(U - 0.5).min(), np.abs(V - 0.5).min())
        if near >= 1e-3:
            break
    else:
        raise AssertionError("no start keeps its distance from the threshold")
    res = orc.elbmf_fit(X, U0, V0, None, reg_l1=0.02, reg_l2=0.05, reg_growth=1.1, beta=0.15, max_iter=6, min_diff=0.0, reassoc=True)
    assert len(res["updates"]) == 8
    eng = WidePalmEngine(BitMatrix(X, "cuda:0"), k, L.PALM_ELBMF, beta=0.15)
    eng.load_factors(U0, V0)
    for t, want in enumerate(res["updates"]):
        l1, l2 = 0.02, 0.05 * 1.1 ** t
        eng.step("U", l1, l2, l1, l2)
        eng.step("V", l1, l2, l1, l2)
        eng.refresh("U")
        eng.refresh("V")
        err, gu, gv, cnt = eng.scalars()
        assert err == pytest.approx(want[6], rel=1e-4) and gu == pytest.approx(want[4], rel=1e-4) and gv == pytest.approx(want[5], rel=1e-4), t
        assert cnt == tuple(res["counts"][t]), t
    U, V = eng.factors()
    assert relf(U, res["U"]) < 1e-4 and relf(V, res["V"]) < 1e-4
    assert not eng.can_pipeline()


@pytest.mark.parametrize("task", ["reconstruction", "prediction"])
def test_elbmf_val_and_test_sets_at_k72(g34, task):
    """X_val / X_test under both tasks: the extra columns of the last iteration equal the scores recomputed by _score from the factors
    the fit returns (which are those of that iteration), and every row has them."""
    from scipy.sparse import csr_matrix
    z, _, meta, data = g34
    X, U0, V0 = data[72]
    rs = np.random.RandomState(72)
    split = rs.rand(*X.shape)
    parts = [csr_matrix(np.where(sel, X, 0).astype(np.float64)) for sel in (split < 0.7, (split >= 0.7) & (split < 0.85), split >= 0.85)]
    mdl = fit_elbmf(parts[0], U0, V0, 72, 0.0, 6, 1e-8, X_val=parts[1], X_test=parts[2], task=task)
    names = ["ERR", "Accuracy", "Recall", "Precision", "F1"]
    cols = [tuple(str(x) for x in c) for c in mdl.logs["updates"].columns]
    rows = mdl.logs["updates"].values.tolist()
    assert len(rows) == mdl.n_iter
    for nm in ("val", "test"):
        idx = [cols.index((nm, "0", mt)) for mt in names]
        assert all(np.isfinite([float(r[i]) for i in idx]).all() for r in rows)
        np.testing.assert_allclose([float(rows[-1][i]) for i in idx], [float(v) for v in mdl._score(nm, names)], rtol=1e-12, atol=1e-15)
    if task == "prediction":
        idx = [cols.index(("train", "0", mt)) for mt in names]
        np.testing.assert_allclose([float(rows[-1][i]) for i in idx], [float(v) for v in mdl._score("train", names)], rtol=1e-12, atol=1e-15)


def test_k64_still_runs_on_the_narrow_engine(g34):
    """Rank 64 is untouched: PalmEngine is chosen, and the factors after 5 iterations are bit-identical to driving that engine directly."""
    from pybmf_amd import _lib as L
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.palm import PalmEngine
    from pybmf_amd.palm_wide import WidePalmEngine, palm_engine
    _, _, _, data = g34
    X, U0, V0 = data[65]
    U0, V0 = np.ascontiguousarray(U0[:, :64]), np.ascontiguousarray(V0[:, :64])
    mdl = fit_elbmf(X, U0, V0, 64, 0.0, 3, 0.0)
    assert type(mdl._eng) is PalmEngine and not isinstance(mdl._eng, WidePalmEngine)
    assert type(palm_engine(BitMatrix(X, "cuda:0"), 64, L.PALM_ELBMF)) is PalmEngine
    eng = PalmEngine(BitMatrix(X, "cuda:0"), 64, L.PALM_ELBMF, beta=0.0)
    eng.load_factors(U0, V0)
    for t in range(mdl.n_iter):
        eng.iterate(t, LOOP["reg_l1"], LOOP["reg_l2"] * LOOP["reg_growth"] ** t, LOOP["reg_l1"], LOOP["reg_l2"] * LOOP["reg_growth"] ** t)
    U, V = eng.factors()
    assert mdl.n_iter == 5 and np.array_equal(mdl.U, U) and np.array_equal(mdl.V, V)


def test_refusals(g34):
    from pybmf_amd.models import ELBMF, PRIMP
    from pybmf_amd.models.ELBMF import update_U
    import importlib
    P = importlib.import_module("pybmf_amd.models.PRIMP")
    _, _, _, data = g34
    X, U0, V0 = data[72]
    rs = np.random.RandomState(1)
    with quiet():
        with pytest.raises(NotImplementedError, match="k <= 128"):
            ELBMF(k=129, U=rs.rand(X.shape[0], 129), V=rs.rand(X.shape[1], 129), init_method="custom", max_iter=2).fit(X, **FIT)
        with pytest.raises(NotImplementedError, match="k <= 128"):
            PRIMP(k=129, max_iter=2, seed=0).fit(X, **FIT)
        with pytest.raises(NotImplementedError, match="k <= 128"):
            update_U(X, rs.rand(X.shape[0], 130), rs.rand(X.shape[1], 130), None, 0.01, 0.02, 0.0, rs.rand(X.shape[0], 130))
        with pytest.raises(NotImplementedError):
            ELBMF(k=72, U=U0.copy(), V=V0.copy(), init_method="custom", max_iter=2).fit(X.astype(np.float64) * 3, **FIT)
        with pytest.raises(NotImplementedError):
            P.elbmf_step_ipalm(X * 3, U0, np.ascontiguousarray(V0.T), None, 0.01, 0.0, 1.0, 0.0)
