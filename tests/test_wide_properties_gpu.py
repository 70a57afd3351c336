"""Randomised (hypothesis, derandomised) checks of the rank 64 < k <= 128 path (pybmf_amd/wide.py) against the fp64 oracle at ragged
shapes: m, n from 1 to 300 -- below 64 and below k included --, k from 65 (one live column in block 1) to 128, densities from almost
empty to almost full.  The style and the gates of tests/test_properties_gpu.py: factors 1e-4 norm-wise, scalars 1e-4 relative,
Boolean counts exact; draws where a factor entry lies within fp32 rounding of a threshold are skipped."""
import contextlib
import io

import numpy as np
import pytest
from scipy.sparse import csr_matrix

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402

hyp = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, assume, given, settings, strategies as st  # noqa: E402

FIT = dict(show_logs=False, show_result=False, save_model=False)
SETTINGS = dict(deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
SHAPE = dict(m=st.integers(1, 300), n=st.integers(1, 300), k=st.integers(65, 128), dens=st.floats(0.05, 0.9), seed=st.integers(0, 10_000))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def relf(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def frame_values(df):
    return np.array([[float(v) for v in row[1:]] for row in df.values.tolist()])  # drop the 'time' column


def clear_of(F, t=0.5):
    """No entry within fp32 rounding (and the 1e-4 factor gate) of the threshold t."""
    return np.abs(np.asarray(F) - t).min() > 1e-4 * t


def start(rs, X, k):
    """Initial factors with entries on both sides of 0.5, a zero row of U (m > 2) and a zero column of V (the eps paths).  The row
    stays live unless other rows of X hold ones too: when every one of X sits in the eps row, the fp64 oracle walks off the fp32 range
    the contractions work in (at m = 3, n = 1: U ~ 1e15, V ~ 1e-33 after one WNMF update, V^T V underflows)."""
    m, n = X.shape
    U0, V0 = rs.rand(m, k) * 0.7, rs.rand(n, k) * 0.7
    r = rs.randint(m)
    if m > 2 and X.sum() > X[r].sum():
        U0[r, :] = 0.0
    V0[:, rs.randint(k)] = 0.0
    return orc.zeros_to_eps(U0), orc.zeros_to_eps(V0)


def in_fp32_range(*Fs):
    """Every non-zero entry of the oracle's factors at least 1e-18, so that the products the fp32 contractions form of them (Gram
    entries: squares) stay normal fp32 numbers.  MU from an eps entry can drive a factor far below that (7e-42 at m = n = 3 when a
    column's only one sits in the eps row of U), where fp32 flushes what fp64 keeps."""
    return all(np.abs(F[F != 0]).min(initial=1.0) >= 1e-18 for F in Fs)


def trace_floors(X, cols):
    """Absolute floors of the logged scalars, per column name, added to the 1e-4 relative gate (those of test_properties_gpu.py):
    error / rec_error come from the trace form 1/2 (sum X - 2 <U, X V> + <U^T U, V^T V>) on fp32 contractions, ~1e-7 |X|^2, which a
    near-exact fit (WNMF at m = n = 1) reaches; RMSE = sqrt(2 rec / cells) turns it into ~1e-3 rms(X); MAE is a direct sum from the
    fp32 shadows of the factors, ~1e-7 |P| per cell."""
    f = dict(error=2e-6 * X.sum(), rec_error=2e-6 * X.sum(), RMSE=1e-3 * np.sqrt(X.mean()), MAE=1e-6)
    return np.array([f.get(c, 0.0) for c in cols])


def check_rows(rows, want, X, cols, tag):
    rows, want = np.asarray(rows), np.asarray(want)
    assert rows.shape == want.shape, (tag, rows.shape, want.shape)
    assert (np.abs(rows - want) <= 1e-4 * np.abs(want) + trace_floors(X, cols)).all(), (tag, rows, want)


@pytest.mark.parametrize("penalty", [True, False])
def test_wide_engine_updates(penalty):
    """WideMUEngine, 4 updates: factors after each against the re-associated penalty updates / the WNMF update, and the scalars of
    every state (error, rec_error, reg_error, RMSE, MAE, confusion counts)."""
    from pybmf_amd import _lib as L
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.wide import WideMUEngine

    @settings(max_examples=40, **SETTINGS)
    @given(**SHAPE)
    def check(m, n, k, dens, seed):
        rs = np.random.RandomState(seed)
        X = (rs.rand(m, n) < dens).astype(np.float64)
        assume(X.sum() > 0)
        U, V = start(rs, X, k)
        eng = WideMUEngine(BitMatrix(X.astype(np.uint8), "cuda:0"), k, L.MODE_PENALTY if penalty else L.MODE_WNMF, with_mae=True)
        eng.load_factors(U, V)
        eng.prepare()
        reg = 0.5
        for it in range(5):
            if it:
                eng.update(reg)
                if penalty:
                    V = orc.penalty_update_V_reassoc(X, U, V, reg)
                    U = orc.penalty_update_U_reassoc(X, U, V, reg)
                else:
                    U, V = orc.wnmf_update(X, None, U, V)
                assume(in_fp32_range(U, V))
                Ug, Vg = eng.factors()
                assert Ug.shape == (m, k) and Vg.shape == (n, k)
                assert relf(Ug, U) < 1e-4 and relf(Vg, V) < 1e-4, (it, m, n, k, relf(Ug, U), relf(Vg, V))
            assume(clear_of(U) and clear_of(V))
            got = eng.scalars(reg)
            P = U @ V.T
            if penalty:
                err, rec, rg = orc.penalty_errors(X, None, U, V, reg)
            else:
                rec = orc.rec_term(X, P)
                err, rg = rec, 0.0
            rmse, mae = orc.rmse_mae(X, P)
            names = ("error", "rec_error", "reg_error", "RMSE", "MAE")
            for g, w, fl, name in zip(got[:5], (err, rec, rg, rmse, mae), trace_floors(X, names), names):
                assert g == pytest.approx(w, rel=1e-4, abs=max(fl, 1e-9)), (it, m, n, k, name, g, w)
            assert got[5] == tuple(int(c) for c in orc.confusion_counts(X, orc.boolean_product(U, V, 0.5, 0.5))), (it, m, n, k)
            reg *= 1.3
        s_abs, s_sq = eng.residual_sums()
        R = X - U @ V.T
        cells = m * n   # (the MAE floor of trace_floors, per cell)
        assert s_abs == pytest.approx(np.abs(R).sum(), rel=1e-4, abs=1e-6 * cells) and s_sq == pytest.approx((R * R).sum(), rel=1e-4, abs=1e-12 * cells)

    check()


def masks(rs, X, kind):
    """(what the class is given as X and W, the dense W of the oracle) for W = 'full' or 'mask' (a csr with explicit zeros: the stored
    cells are the observed ones)."""
    m, n = X.shape
    if kind == "full":
        return X, "full", None
    obs = rs.rand(m, n) < 0.6
    obs |= X != 0
    r, c = np.nonzero(obs)
    return csr_matrix((X[r, c], (r, c)), shape=(m, n)), "mask", obs.astype(np.float64)


def test_wide_classes_fit():
    """BinaryMFPenalty and WNMF at k > 64 under W = 'full' and 'mask': the log tables, the factors, the Boolean product and
    _score_train against orc.penalty_fit / orc.wnmf_fit.  (A weight matrix at k > 64: tests/test_wide_extras_gpu.py, fixed shape.)"""
    from pybmf_amd.models import BinaryMFPenalty, WNMF

    @settings(max_examples=40, **SETTINGS)
    @given(kind=st.sampled_from(["full", "mask"]), **SHAPE)
    def check(kind, m, n, k, dens, seed):
        rs = np.random.RandomState(seed)
        X = (rs.rand(m, n) < dens).astype(np.float64)
        Xin, Wcls, Wd = masks(rs, X, kind)
        assume((X if Wd is None else Wd * X).sum() > 0)
        U0, V0 = start(rs, X, k)
        ref = orc.penalty_fit(X, k=k, U=U0.copy(), V=V0.copy(), W=Wd, reg=0.5, reg_growth=1.3, init_method="custom", normalize_method=None,
                              max_iter=3, tol=-1.0)
        assume(clear_of(ref["U"]) and clear_of(ref["V"]) and in_fp32_range(ref["U"], ref["V"]))
        with quiet():
            mdl = BinaryMFPenalty(k=k, U=U0.copy(), V=V0.copy(), W=Wcls, reg=0.5, reg_growth=1.3, init_method="custom", normalize_method=None,
                                  max_iter=3, tol=-1.0)
            mdl.fit(Xin.copy(), task="reconstruction", **FIT)
        tag = (kind, m, n, k)
        assert relf(mdl.U, ref["U"]) < 1e-4 and relf(mdl.V, ref["V"]) < 1e-4, (tag, relf(mdl.U, ref["U"]), relf(mdl.V, ref["V"]))
        check_rows(frame_values(mdl.logs["updates"]), ref["updates"], X, ("iter", "error", "rec_error", "reg", "reg_error", "RMSE", "MAE"), tag)
        assert [tuple(c) for c in mdl.counts] == [tuple(c) for c in ref["counts"]], tag
        rmse, mae = orc.rmse_mae(X, ref["U"] @ ref["V"].T)
        got = mdl._score_train(["RMSE", "MAE", "TP", "FP"])
        assert got[0] == pytest.approx(rmse, rel=1e-4, abs=1e-6) and got[1] == pytest.approx(mae, rel=1e-4, abs=1e-6), tag
        assert tuple(got[2:]) == tuple(ref["counts"][-1][:2]), tag

        # tol at the trace-form floor: an exact fit (m = n = 1 after one update) has error 0.0 in fp64 and ~1e-9 on the fp32
        # contractions, so "error <= tol" with the default tol = 0 would stop the two runs at different iterations; both stop there now
        # (running on past an exact fit drives entries below the fp32 range, where the two cannot agree)
        tol = float(trace_floors(X, ("error",))[0])
        refw = orc.wnmf_fit(X.copy(), k, U=U0.copy(), V=V0.copy(), W=Wd, max_iter=3, init_method="custom", tol=tol)
        assume(in_fp32_range(refw["U"], refw["V"]))
        with quiet():
            w = WNMF(k=k, U=U0.copy(), V=V0.copy(), W=Wcls, init_method="custom", max_iter=3, tol=tol)
            w.fit(Xin.copy(), task="reconstruction", **FIT)
        # rows / columns whose observed cells are all zero are where the reference's in-place "0 -> eps" on X_train decides the
        # factors (tests/test_properties_gpu.py::test_masked_updates_with_weights): the others, and the product where it is observed
        Wo = np.ones_like(X) if Wd is None else Wd
        live_r, live_c = (Wo * X).sum(1) > 0, (Wo * X).sum(0) > 0
        assert relf(w.U[live_r], refw["U"][live_r]) < 1e-4 and relf(w.V[live_c], refw["V"][live_c]) < 1e-4, tag
        P, Pr = (w.U @ w.V.T)[Wo != 0], (refw["U"] @ refw["V"].T)[Wo != 0]
        assert np.abs(P - Pr).max() <= 1e-4 * max(1.0, np.abs(Pr).max()), tag
        if live_r.all() and live_c.all():
            check_rows(frame_values(w.logs["updates"]), refw["updates"], X, ("iter", "error", "RMSE", "MAE"), tag)
            rmse, mae = orc.rmse_mae(X, refw["U"] @ refw["V"].T)
            got = w._score_train(["RMSE", "MAE"])
            assert got[0] == pytest.approx(rmse, rel=1e-4, abs=1e-6) and got[1] == pytest.approx(mae, rel=1e-4, abs=1e-6), tag

    check()


def test_wide_classes_prediction():
    """task = 'prediction' with X_val / X_test at k > 64 (W = 'mask' on the training csr): factors against the oracle's fit, and the
    scores of both extra sets against orc.entry_scores on their non-zero cells (ContinuousModel densifies its data sets)."""
    from pybmf_amd.models import BinaryMFPenalty

    @settings(max_examples=30, **SETTINGS)
    @given(**SHAPE)
    def check(m, n, k, dens, seed):
        rs = np.random.RandomState(seed)
        X = (rs.rand(m, n) < dens).astype(np.float64)
        split = rs.randint(3, size=(m, n))
        sets = []
        for part in range(3):
            r, c = np.nonzero(split == part)
            sets.append(csr_matrix((X[r, c], (r, c)), shape=(m, n)))
        train = sets[0]
        obs = (split == 0).astype(np.float64)
        assume((obs * X).sum() > 0 and sets[1].count_nonzero() > 0 and sets[2].count_nonzero() > 0)
        U0, V0 = start(rs, obs * X, k)
        ref = orc.penalty_fit(X, k=k, U=U0.copy(), V=V0.copy(), W=obs, reg=0.5, reg_growth=1.3, init_method="custom", normalize_method=None,
                              max_iter=3, tol=-1.0)
        assume(clear_of(ref["U"]) and clear_of(ref["V"]) and in_fp32_range(ref["U"], ref["V"]))
        with quiet():
            mdl = BinaryMFPenalty(k=k, U=U0.copy(), V=V0.copy(), W="mask", reg=0.5, reg_growth=1.3, init_method="custom", normalize_method=None,
                                  max_iter=3, tol=-1.0)
            mdl.fit(train.copy(), sets[1].copy(), sets[2].copy(), task="prediction", **FIT)
        tag = (m, n, k)
        assert relf(mdl.U, ref["U"]) < 1e-4 and relf(mdl.V, ref["V"]) < 1e-4, (tag, relf(mdl.U, ref["U"]), relf(mdl.V, ref["V"]))
        U32, V32 = mdl.U.astype(np.float32).astype(np.float64), mdl.V.astype(np.float32).astype(np.float64)
        for name, S in (("val", sets[1]), ("test", sets[2])):
            coo = S.tocoo()
            nz = coo.data != 0
            r, c, d = coo.row[nz], coo.col[nz], coo.data[nz]
            rmse, mae = mdl._score(name, ["RMSE", "MAE"])
            want = orc.entry_scores(r, c, d, U32, V32)
            assert rmse == pytest.approx(want[0], rel=1e-4) and mae == pytest.approx(want[1], rel=1e-4), (tag, name)
            assert tuple(mdl._score(name, ["TP", "FP", "FN", "TN"])) == tuple(orc.entry_scores(r, c, d, mdl.U, mdl.V, 0.5, 0.5)), (tag, name)

    check()
