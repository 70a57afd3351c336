"""BinaryMFThresholdExColumnwise without a GPU: the NumPy restatement (tests/thresh_cols_ref.py) against central differences and against
the reference's own recorded numbers of the scalar model (golden g4), the argument checks of the C entry points, the model's surface
(parameter print, threshold arguments, refusals before any upload) and the conditions of the fit fixtures."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import thresh_cols_ref as R

FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False, verbose=False)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 17, 64])
def test_gradient_against_central_differences(k):
    """dF is the true gradient of F (d Us / d us = -dUs cancels the sign of the residual's derivative, so the reference's sign is the
    gradient's): dF[i] = (F(x + h e_i) - F(x - h e_i)) / 2h.  Gate 1e-7 max|dF|: the
    differences of an fp64 F ~ 1e2..1e3 at h = 1e-6 are good to ~1e-9 of the gradient's scale (h^2 truncation ~1e-12, rounding
    eps F / h ~ 1e-8 absolute on gradients of ~1e2)."""
    rs = np.random.RandomState(k)
    m, n = 40, 30
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    scale = rs.uniform(0.5, 3.0, size=k)
    U, V = rs.rand(m, k) * scale, rs.rand(n, k) * scale
    x = np.concatenate([rs.uniform(0.3, 0.7, size=k) * scale, rs.uniform(0.3, 0.7, size=k) * scale])
    lam, h = 10, 1e-6
    got = R.dF(X, U, V, x, lam)
    num = np.empty(2 * k)
    for i in range(2 * k):
        e = np.zeros(2 * k)
        e[i] = h
        num[i] = (R.F(X, U, V, x + e, lam) - R.F(X, U, V, x - e, lam)) / (2 * h)
    err = np.abs(got - num).max() / np.abs(got).max()
    print(f"k={k}: |dF - central difference| / max|dF| = {err:.2e}")
    assert err <= 1e-7


def test_constant_vectors_equal_the_recorded_scalar_model(golden_dir):
    """At every grid point (u, v) of golden g4 and lamda in {10, 100}: F at constant vectors equals the reference's F_grid (rtol 1e-12)
    and the two halves of dF sum to its dF_grid (1e-10 of its scale)."""
    z = np.load(os.path.join(golden_dir, "g4_threshold.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g4_threshold.json")))
    X = np.unpackbits(z["X_bits"], axis=1, bitorder="little")[:, : z["shape"][1]].astype(np.float64)
    U, V = z["U"], z["V"]
    k = U.shape[1]
    for lam in (10, 100):
        Fg, dFg = z[f"F_grid_lam{lam}"], z[f"dF_grid_lam{lam}"]
        scale = np.abs(dFg).max()
        for i, u in enumerate(meta["grid_u"]):
            for j, v in enumerate(meta["grid_v"]):
                x = np.concatenate([np.full(k, u), np.full(k, v)])
                assert R.F(X, U, V, x, lam) == pytest.approx(Fg[i, j], rel=1e-12)
                g = R.dF(X, U, V, x, lam)
                assert abs(g[:k].sum() - dFg[i, j, 0]) <= 1e-10 * scale and abs(g[k:].sum() - dFg[i, j, 1]) <= 1e-10 * scale


# ---- the C entry points refuse bad arguments without a GPU ------------------------------------------------------------------------------
def cols(lib, **over):
    p = C.c_void_p(4096)
    a = dict(seg_row=p, seg_beg=p, seg_len=p, nseg=10, idx=p, m=100, n=80, U64=p, V64=p, ldf=32, k=20, x=p, n_points=4, work=p, out_host=p)
    a.update(over)
    return lib.bmf_thresh_cols64(a["seg_row"], a["seg_beg"], a["seg_len"], a["nseg"], a["idx"], a["m"], a["n"], a["U64"], a["V64"], a["ldf"], a["k"], a["x"],
                                 a["n_points"], 10.0, 50.0, 1, a["work"], a["out_host"], 1.0, None)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    for name in ("seg_row", "seg_beg", "seg_len", "idx", "U64", "V64", "x", "work", "out_host"):
        assert cols(lib, **{name: None}) == -1 and b"bmf_thresh_cols64: null pointer" in lib.bmf_last_error(), name
    for over, text in ((dict(k=0), b"k=0 outside 1..64"), (dict(k=65, ldf=128), b"k=65 outside 1..64"), (dict(k=-3), b"outside 1..64"),
                       (dict(ldf=19), b"ldf=19 < k=20"), (dict(m=0), b"m=0, n=80 must be >= 1"), (dict(n=0), b"m=100, n=0 must be >= 1"),
                       (dict(m=-5), b"must be >= 1"), (dict(nseg=0), b"nseg=0 outside 1..864"), (dict(nseg=865), b"nseg=865 outside 1..864"),
                       (dict(n_points=0), b"n_points=0 outside 1..16 for k=20"), (dict(n_points=17), b"n_points=17 outside 1..16 for k=20"),
                       (dict(k=16, n_points=33), b"n_points=33 outside 1..32 for k=16"), (dict(k=33, ldf=64, n_points=9), b"n_points=9 outside 1..8 for k=33"),
                       (dict(work=C.c_void_p(4104)), b"not 16-byte aligned"), (dict(out_host=C.c_void_p(4104)), b"not 16-byte aligned")):
        assert cols(lib, **over) == -1, over
        assert b"bmf_thresh_cols64" in lib.bmf_last_error() and text in lib.bmf_last_error(), (over, lib.bmf_last_error())
    # the two queries are host arithmetic: positive, monotone, k = 0 and k = 65 refused
    assert [lib.bmf_thresh_cols64_max_points(k) for k in (1, 16, 17, 32, 33, 64)] == [32, 32, 16, 16, 8, 8]
    assert lib.bmf_thresh_cols64_max_points(0) == -1 and lib.bmf_thresh_cols64_max_points(65) == -1
    for k in (1, 16, 17, 32, 33, 64):
        mp = lib.bmf_thresh_cols64_max_points(k)
        sizes = [lib.bmf_thresh_cols64_work(100, 80, k, p_) for p_ in range(1, mp + 1)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert lib.bmf_thresh_cols64_work(200, 80, k, mp) > sizes[-1] and lib.bmf_thresh_cols64_work(100, 160, k, mp) > sizes[-1]
        assert lib.bmf_thresh_cols64_work(100, 80, k, mp + 1) == -1 and lib.bmf_thresh_cols64_work(100, 80, k, 0) == -1
    for bad in ((0, 80, 5, 1), (100, 0, 5, 1), (100, 80, 0, 1), (100, 80, 65, 1)):
        assert lib.bmf_thresh_cols64_work(*bad) == -1, bad


# ---- the model's surface ----------------------------------------------------------------------------------------------------------
def make(k=3, m=10, n=8, **kw):
    from pybmf_amd.models.BinaryMFThresholdExColumnwise import BinaryMFThresholdExColumnwise
    rs = np.random.RandomState(7)
    return BinaryMFThresholdExColumnwise(k=k, U=rs.rand(m, k), V=rs.rand(n, k), **kw)


def test_parameter_print_and_threshold_arguments():
    from pybmf_amd import models
    from pybmf_amd.models.BinaryMFThresholdExColumnwise import BinaryMFThresholdExColumnwise
    assert models.BinaryMFThresholdExColumnwise is BinaryMFThresholdExColumnwise and "BinaryMFThresholdExColumnwise" in models.__all__
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model = make(k=20, m=30, n=50, W="full", us=tuple(0.1 * c for c in range(20)), vs=[0.5] * 20, lamda=5, seed=3)
    names = [line.split(":")[0].replace("[I]", "").strip() for line in buf.getvalue().splitlines()]
    assert names[:13] == ["k", "U", "V", "W", "us", "vs", "lamda", "min_diff", "max_iter", "init_method", "solver", "normalize_method", "seed"]
    lines = buf.getvalue().splitlines()
    assert lines[4] == "[I] us           : (20,)" and lines[5] == "[I] vs           : (20,)" and lines[7] == "[I] min_diff     : 0.001"
    assert model.us.dtype == np.float64 and model.us.shape == (20,) and np.array_equal(model.us, [0.1 * c for c in range(20)])
    assert model.vs.dtype == np.float64 and np.array_equal(model.vs, np.full(20, 0.5))
    with contextlib.redirect_stdout(io.StringIO()):
        model = make(k=3)                                                   # the defaults: scalars, broadcast
        assert np.array_equal(model.us, [0.5] * 3) and np.array_equal(model.vs, [0.5] * 3) and model.W == "mask" and model.lamda == 100
        model = make(k=3, us=0.25, vs=np.array([1, 2, 3]))
        assert np.array_equal(model.us, [0.25] * 3) and np.array_equal(model.vs, [1.0, 2.0, 3.0]) and model.vs.dtype == np.float64
        assert np.array_equal(model.threshold_to_x(), [0.25, 0.25, 0.25, 1, 2, 3])
        model.x_to_threshold(np.arange(6.0))
        assert np.array_equal(model.us, [0, 1, 2]) and np.array_equal(model.vs, [3, 4, 5])
        lo, hi = model.x_bounds()
        assert np.array_equal(lo, np.concatenate([model.U.min(axis=0), model.V.min(axis=0)]) + 1e-6)
        assert np.array_equal(hi, np.concatenate([model.U.max(axis=0), model.V.max(axis=0)]) - 1e-6)
        for bad in (dict(us=(0.1, 0.2)), dict(vs=[0.1] * 4), dict(us=np.zeros((3, 1)))):
            with pytest.raises(ValueError, match="scalar or a sequence of k = 3"):
                make(k=3, **bad)
        with pytest.raises(AssertionError):
            make(k=3, solver="grid-search")


def test_refusals_come_before_any_upload(monkeypatch):
    import pybmf_amd.engine as E

    def no_upload(*a, **k):
        raise AssertionError("the data went to the device before the refusal")
    monkeypatch.setattr(E, "BitMatrix", no_upload)
    monkeypatch.setattr(E, "SparseObs", no_upload)
    monkeypatch.setattr(E, "RealMatrix", no_upload)
    X = (np.random.RandomState(1).rand(10, 8) < 0.4).astype(np.uint8)
    holes = csr_matrix(X)                                     # W = 'mask' on a csr that does not store every cell
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match=r"Boolean \(0/1\)"):
            make(W="full").fit(X.astype(np.float64) * 0.5, **FIT_KW)
        with pytest.raises(NotImplementedError, match=r"Boolean \(0/1\)"):
            make(W="full").fit(X, X_val=csr_matrix(X * 3), **FIT_KW)
        with pytest.raises(NotImplementedError, match="all-ones mask only"):
            make().fit(holes, **FIT_KW)                       # (the default W = 'mask')
        with pytest.raises(NotImplementedError, match="all-ones mask only"):
            make().fit(X, **FIT_KW)                           # (a dense array under 'mask': its non-zeros are the pattern)
        Wm = np.ones((10, 8))
        Wm[2, 3] = 0
        with pytest.raises(NotImplementedError, match="all-ones mask only"):
            make(W=Wm).fit(X, **FIT_KW)
        with pytest.raises(NotImplementedError, match="all-ones mask only"):
            make(W=np.full((10, 8), 2.0)).fit(X, **FIT_KW)
        with pytest.raises(NotImplementedError, match="k=65.*k <= 64"):
            make(k=65, W="full").fit(X, **FIT_KW)
        import torch.distributed as dist
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        with pytest.raises(NotImplementedError, match="one GPU"):
            make(W="full").fit(X, **FIT_KW)


def test_memory_budget_rule():
    """The list of the ones may take 16 bytes per one within a quarter of the free device memory, at most 4 GiB (the rule
    BinaryMFThreshold._setup_trace applies; this model refuses where the scalar one falls back to the tile product)."""
    from pybmf_amd.ones_list import list_fits
    assert list_fits(1000, 64000) and not list_fits(1001, 64000)
    assert list_fits((4 << 30) // 16, 1 << 40) and not list_fits((4 << 30) // 16 + 1, 1 << 40)


# ---- the fit fixtures meet their conditions (from the restatement alone) -------------------------------------------------------------------
@pytest.mark.parametrize("k,lam", R.FIXTURES)
def test_fit_fixture_conditions(k, lam):
    X, U, V, us, vs, ref = R.fixture(k, lam)
    br, bc = R.BLOCKS[k]
    assert X.shape == (k * br, k * bc) and U.shape == (k * br, k) and V.shape == (k * bc, k)
    print(f"k={k} lamda={lam}: n_iter={ref['n_iter']} clamped={ref['clamped']} margins armijo={ref['armijo']:.2e} "
          f"curvature={ref['curvature']:.2e} entry={ref['entry']:.2e}")
    if lam == 10:
        assert ref["n_iter"] >= 3
    else:
        assert ref["clamped"] >= 1
    assert ref["armijo"] >= R.MARGIN and ref["curvature"] >= R.MARGIN and ref["entry"] >= R.MARGIN
    assert len(ref["F"]) == ref["n_iter"] + 1 == len(ref["x"]) and all(b <= a for a, b in zip(ref["F"], ref["F"][1:]))
