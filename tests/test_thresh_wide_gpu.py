"""BinaryMFThreshold at a rank 64 < k <= 128 through the class, against the reference's own runs (golden g33,
tests/golden/make_golden_threshold_wide.py).  Gates, those under which test_models_gpu.py and test_masked_gpu.py hold g4 and g8: the same
number of rows as the reference, (u, v, F) to 1e-6, the log columns equal, the Boolean counts equal."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FIT = dict(show_logs=False, show_result=False, save_model=False)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


@pytest.fixture(scope="module")
def g33(golden_dir):
    z = np.load(os.path.join(golden_dir, "g33_threshold_wide.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g33_threshold_wide.json")))
    return z, meta


def unpack(z, name):
    return np.unpackbits(z[f"{name}_X_bits"], axis=1, bitorder="little")[:, : z[f"{name}_shape"][1]]


def cells(z, prefix, shape):
    M = csr_matrix((z[prefix + "_vals"].astype(np.float64), (z[prefix + "_rows"], z[prefix + "_cols"])), shape=shape)
    assert M.nnz == len(z[prefix + "_rows"])      # explicit zeros stay stored
    return M


def frame(df):
    cols = [tuple(str(x) for x in c) for c in df.columns][1:]      # drop the 'time' column
    return cols, np.array([[float(v) for v in row[1:]] for row in df.values.tolist()])


def check_against_reference(model, ref):
    cols, rows = frame(model.logs["updates"])
    want = np.array(ref["rows"]["rows"])
    assert cols == [tuple(c) for c in ref["rows"]["columns"]]
    nc = min(len(rows), len(want))
    bad = np.nonzero(np.abs(rows[:nc, 1:4] - want[:nc, 1:4]).max(1) > 1e-6 * np.abs(want[:nc, 1:4]).max(1) + 1e-9)[0]
    first = int(bad[0]) if len(bad) else nc
    print("rows", len(rows), "reference", len(want), "worst (u, v, F) relative difference", float(np.abs(rows[:nc, 1:4] / want[:nc, 1:4] - 1).max()))
    assert len(rows) == len(want), (len(rows), len(want), "first differing row", first, rows[max(first - 1, 0):first + 2, :4].tolist(),
                                    want[max(first - 1, 0):first + 2, :4].tolist())
    np.testing.assert_allclose(rows[:, :4], want[:, :4], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(rows[:, 4:], want[:, 4:], rtol=1e-12, atol=1e-15)      # scores at those thresholds: exact counts
    assert model.u == pytest.approx(ref["u"], abs=1e-6) and model.v == pytest.approx(ref["v"], abs=1e-6)
    assert [int(c) for c in model._cover_counts()[:4]] == ref["counts"]
    return rows


def fit_full(z, meta, name, lam):
    from pybmf_amd.models import BinaryMFThreshold
    c = meta[name]
    with quiet():
        model = BinaryMFThreshold(k=c["k"], U=z[f"{name}_U"].copy(), V=z[f"{name}_V"].copy(), W="full", u=c["u0"], v=c["v0"], lamda=lam, min_diff=1e-3,
                                  max_iter=c["max_iter"])
        model.fit(unpack(z, name), task="reconstruction", **FIT)
    return model


@pytest.mark.parametrize("name,lam", [("a", 10), ("a", 100), ("b", 100), ("c", 10)])
def test_full_mask_matches_the_reference(g33, name, lam):
    """Cases a, b, c: W='full', the trace form in batches of up to eight trial points."""
    z, meta = g33
    model = fit_full(z, meta, name, lam)
    assert model._kp == 128 and model._trace is not None and model._trace["max_pairs"] == 8
    assert tuple(model._Ud.shape)[1] == 128 and tuple(model._Vd.shape)[1] == 128
    rows = check_against_reference(model, meta[name][f"lam{lam}"])
    gi = meta["grid"]
    assert model.F([gi[1], gi[2]]) == pytest.approx(z[f"{name}_F_grid_lam{lam}"][1, 2], rel=1e-11)
    if (name, lam) == ("a", 10):      # fitted twice: identical logs
        again = frame(fit_full(z, meta, name, lam).logs["updates"])[1]
        assert np.array_equal(rows, again)


def test_stored_cells_match_the_reference(g33):
    """Case d: the class default W='mask' on a csr with explicit zeros, an empty row and an empty column: the cell-list objective."""
    from pybmf_amd.models import BinaryMFThreshold
    z, meta = g33
    c = meta["d"]
    X = cells(z, "d", tuple(int(s) for s in z["a_shape"]))
    with quiet():
        model = BinaryMFThreshold(k=c["k"], U=z["a_U"].copy(), V=z["a_V"].copy(), u=c["u0"], v=c["v0"], lamda=c["lamda"], min_diff=1e-3, max_iter=c["max_iter"])
        model.fit(X.copy(), task="reconstruction", **FIT)
    assert model._kp == 128 and model._trace is None and model._obs is not None
    check_against_reference(model, c)
    for i, a in enumerate(meta["grid"]):
        for j, b in enumerate(meta["grid"]):
            assert model.F([a, b]) == pytest.approx(z["d_F_grid"][i, j], rel=1e-11)
            assert np.abs(model.dF([a, b]) - z["d_dF_grid"][i, j]).max() <= 1e-9 * (np.abs(z["d_dF_grid"]).max() + 1.0)


def test_prediction_with_val_and_test_matches_the_reference(g33):
    """Case e: X_val / X_test under task='prediction': the block-list scorers beside the wide objective."""
    from pybmf_amd.models import BinaryMFThreshold
    z, meta = g33
    c = meta["e"]
    shape = tuple(int(s) for s in z["a_shape"])
    sets = {nm: cells(z, "e_" + nm, shape) for nm in ("train", "val", "test")}
    with quiet():
        model = BinaryMFThreshold(k=c["k"], U=z["a_U"].copy(), V=z["a_V"].copy(), u=c["u0"], v=c["v0"], lamda=c["lamda"], min_diff=1e-3, max_iter=c["max_iter"])
        model.fit(sets["train"].copy(), sets["val"].copy(), sets["test"].copy(), task="prediction", **FIT)
    assert model._kp == 128 and model._obs is not None
    check_against_reference(model, c)


def test_tile_product_route_is_refused(g33, monkeypatch):
    from pybmf_amd.models import BinaryMFThreshold
    z, meta = g33
    monkeypatch.setenv("BMF_THRESH_TRACE", "0")
    with quiet(), pytest.raises(NotImplementedError, match="k=72.*tile-product"):
        BinaryMFThreshold(k=72, U=z["a_U"].copy(), V=z["a_V"].copy(), W="full", lamda=10, max_iter=3).fit(unpack(z, "a"), task="reconstruction", **FIT)


def test_rank_16_still_takes_the_narrow_entry_points(golden_dir, monkeypatch):
    """g4 at k = 16: the entry points of k <= 64 (the wide ones raise if touched), 32 columns on the device, the reference's rows."""
    from pybmf_amd import _lib as L
    from pybmf_amd.models import BinaryMFThreshold

    def touched(*a, **kw):
        raise AssertionError("a wide entry point was called at k = 16")
    for fn in ("bmf_thresh_trace_wide", "bmf_thresh_trace_wide_work", "bmf_thresh_trace_wide_max_pairs", "bmf_thresh_transform64_wide", "bmf_masked_thresh64_wide"):
        monkeypatch.setattr(L.lib, fn, touched)
    z = np.load(os.path.join(golden_dir, "g4_threshold.npz"))
    ref = json.load(open(os.path.join(golden_dir, "g4_threshold.json")))["lam10"]
    X = np.unpackbits(z["X_bits"], axis=1, bitorder="little")[:, : z["shape"][1]]
    with quiet():
        model = BinaryMFThreshold(k=16, U=z["U"].copy(), V=z["V"].copy(), W="full", u=0.5, v=0.5, lamda=10, min_diff=1e-3, max_iter=100)
        model.fit(X, task="reconstruction", **FIT)
    assert model._kp == 32 and model._trace is not None and model._trace["max_pairs"] == 32
    rows, want = frame(model.logs["updates"])[1], np.array(ref["rows"]["rows"])
    assert len(rows) == len(want)
    np.testing.assert_allclose(rows[:, :4], want[:, :4], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(rows[:, 4:], want[:, 4:], rtol=1e-12, atol=1e-15)
    assert model.u == pytest.approx(ref["u"], abs=1e-6) and model.v == pytest.approx(ref["v"], abs=1e-6)
