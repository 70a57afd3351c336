"""BinaryMFThreshold at a rank 64 < k <= 128, the parts that need no GPU: the fixture g33 (tests/golden/make_golden_threshold_wide.py)
against the CPU oracle, the refusals of the new entry points (csrc/thresh_wide.hip) and of the class, and the bound on the workspace."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import oracle as orc

CASES_FULL = [("a", 10), ("a", 100), ("b", 100), ("c", 10)]


@pytest.fixture(scope="module")
def g33(golden_dir):
    z = np.load(os.path.join(golden_dir, "g33_threshold_wide.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g33_threshold_wide.json")))
    return z, meta


def full_matrix(z, name):
    m, n = z[f"{name}_shape"]
    return np.unpackbits(z[f"{name}_X_bits"], axis=1, bitorder="little")[:, :n].astype(np.float64)


def cell_matrix(z, prefix, shape):
    X, W = np.zeros(shape), np.zeros(shape)
    r, c = z[prefix + "_rows"], z[prefix + "_cols"]
    X[r, c], W[r, c] = z[prefix + "_vals"], 1.0
    return X, W


def check_case(X, W, U, V, meta, ref, Fg, dFg, lam, u0, v0, max_iter):
    grid = meta["grid"]
    for i, a in enumerate(grid):
        for j, b in enumerate(grid):
            assert orc.thresh_F(X, W, U, V, a, b, lam) == pytest.approx(Fg[i, j], rel=1e-12)
            np.testing.assert_allclose(orc.thresh_dF(X, W, U, V, a, b, lam), dFg[i, j], rtol=1e-9, atol=1e-9)
    res = orc.threshold_fit(X, U, V, W, u=u0, v=v0, lamda=lam, min_diff=1e-3, max_iter=max_iter)
    want = np.array(ref["rows"]["rows"])
    mine = np.array([r[:4] for r in res["rows"]])
    assert mine.shape == want[:, :4].shape
    np.testing.assert_allclose(mine, want[:, :4], rtol=1e-9, atol=1e-12)
    assert res["u"] == pytest.approx(ref["u"], rel=1e-9) and res["v"] == pytest.approx(ref["v"], rel=1e-9)
    assert [int(c) for c in res["rows"][-1][4:]] == ref["counts"]
    # the recorded counts are decided: no factor entry within 1e-6 of its final threshold
    assert np.abs(U - ref["u"]).min() > 1e-6 and np.abs(V - ref["v"]).min() > 1e-6
    return res, want


@pytest.mark.parametrize("name,lam", CASES_FULL)
def test_fixture_full_mask_against_the_oracle(g33, name, lam):
    z, meta = g33
    X, U, V = full_matrix(z, name), z[f"{name}_U"], z[f"{name}_V"]
    c = meta[name]
    assert U.shape == (X.shape[0], c["k"]) and V.shape == (X.shape[1], c["k"]) and 64 < c["k"] <= 128
    res, want = check_case(X, None, U, V, meta, c[f"lam{lam}"], z[f"{name}_F_grid_lam{lam}"], z[f"{name}_dF_grid_lam{lam}"], lam, c["u0"], c["v0"],
                           c["max_iter"])
    scores = np.array([orc.boolean_scores(*r[4:]) for r in res["rows"]])      # W='full', reconstruction: whole-matrix scores in the log
    np.testing.assert_allclose(scores, want[:, 4:], rtol=1e-15)


def test_fixture_shapes_are_the_issue_s(g33):
    z, meta = g33
    assert [(tuple(z[f"{n}_shape"]), meta[n]["k"]) for n in "abc"] == [((130, 100), 72), ((150, 140), 128), ((90, 70), 65)]
    assert meta["a"]["lamdas"] == [10, 100] and meta["b"]["lamdas"] == [100] and meta["c"]["lamdas"] == [10]


def test_fixture_stored_cells_against_the_oracle(g33):
    """Case d: W='mask' on a csr with explicit zeros, an empty row and an empty column."""
    z, meta = g33
    shape = tuple(z["a_shape"])
    X, W = cell_matrix(z, "d", shape)
    c = meta["d"]
    assert 0.35 < W.mean() < 0.45 and W[c["empty_row"]].sum() == 0 and W[:, c["empty_col"]].sum() == 0
    assert (z["d_vals"] == 0).any() and (z["d_vals"] == 1).any()
    assert (c["u0"], c["v0"], c["lamda"], c["max_iter"]) == (0.3, 0.3, 10, 40)
    res, want = check_case(X, W, z["a_U"], z["a_V"], meta, c, z["d_F_grid"], z["d_dF_grid"], c["lamda"], c["u0"], c["v0"], c["max_iter"])
    scores = np.array([orc.boolean_scores(*r[4:]) for r in res["rows"]])      # reconstruction: the csr as a whole matrix
    np.testing.assert_allclose(scores, want[:, 4:], rtol=1e-15)


def test_fixture_prediction_against_the_oracle(g33):
    """Case e: X_val / X_test under task='prediction'; the log's scores are those of the stored entries of each set."""
    z, meta = g33
    shape = tuple(z["a_shape"])
    X, W = cell_matrix(z, "e_train", shape)
    c = meta["e"]
    res, want = check_case(X, W, z["a_U"], z["a_V"], meta, c, z["e_F_grid"], z["e_dF_grid"], c["lamda"], c["u0"], c["v0"], c["max_iter"])
    cols = [tuple(x) for x in c["rows"]["columns"]]
    for nm in ("train", "val", "test"):
        keep = z[f"e_{nm}_vals"] != 0       # (the reference's csr arithmetic drops the explicit zeros of the ground truth: test_prediction_gpu.py)
        sc = orc.boolean_scores(*orc.entry_scores(z[f"e_{nm}_rows"][keep], z[f"e_{nm}_cols"][keep], z[f"e_{nm}_vals"][keep], z["a_U"], z["a_V"],
                                                  c["u"], c["v"]))
        got = [want[-1][cols.index((nm, "0", mt))] for mt in ("Recall", "Precision", "Accuracy", "F1")]
        np.testing.assert_allclose(got, sc, rtol=1e-12)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def last_error(lib):
    return lib.bmf_last_error().decode()


def test_work_and_max_pairs_refuse_other_ranks():
    from pybmf_amd import _lib as L
    lib = L.lib
    assert lib.bmf_thresh_trace_wide_max_pairs(65) == lib.bmf_thresh_trace_wide_max_pairs(128) >= 1
    maxp = lib.bmf_thresh_trace_wide_max_pairs(100)
    for k, other in ((64, "bmf_thresh_trace64_max_pairs"), (1, "bmf_thresh_trace64_max_pairs"), (129, "k <= 128"), (0, "65..128")):
        assert lib.bmf_thresh_trace_wide_max_pairs(k) == -1
        assert "bmf_thresh_trace_wide_max_pairs" in last_error(lib) and other in last_error(lib), last_error(lib)
    for k, other in ((64, "bmf_thresh_trace64_work"), (129, "k <= 128")):
        assert lib.bmf_thresh_trace_wide_work(100, 100, k, 1) == -1
        assert "bmf_thresh_trace_wide_work" in last_error(lib) and other in last_error(lib), last_error(lib)
    for bad in ((0, 100, 72, 1), (100, 0, 72, 1), (100, 100, 72, 0), (100, 100, 72, maxp + 1)):
        assert lib.bmf_thresh_trace_wide_work(*bad) == -1 and "bmf_thresh_trace_wide_work" in last_error(lib), bad
    one, two = lib.bmf_thresh_trace_wide_work(130, 100, 72, 1), lib.bmf_thresh_trace_wide_work(130, 100, 72, 2)
    assert 0 < one < two and lib.bmf_thresh_trace_wide_work(130, 100, 128, 1) == one      # 128 columns whatever k


def test_workspace_of_a_long_factor_stays_within_the_budget():
    """100 000 rows: the partial Grams are bounded by the chunk count, not by the rows -- one pair fits the 2 GiB that _setup_trace allows
    (with 4096 / 128 rows per partial the Grams alone would be 3 000 x 4 x 128 KiB)."""
    from pybmf_amd import _lib as L
    n_work = L.lib.bmf_thresh_trace_wide_work(100000, 20000, 128, 1)
    assert 0 < n_work * 8 < (2 << 30)
    factors = 2 * (100001 + 20001) * 128
    assert n_work - factors - 3 * (8 * 100000 + 64) - 2 <= 4 * 32 * 128 * 128      # at most 32 partials per matrix


def test_trace_wide_refusals():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    maxp = lib.bmf_thresh_trace_wide_max_pairs(72)

    def call(seg_row=p, idx=p, U=p, work=p, out=p, uv=p, m=10, n=10, ldf=128, k=72, nseg=1, n_pairs=1):
        return lib.bmf_thresh_trace_wide(seg_row, p, p, nseg, idx, m, n, U, p, ldf, k, uv, n_pairs, 10.0, 1.0, 0, work, out, 1.0, None)

    for kw in (dict(seg_row=None), dict(idx=None), dict(U=None), dict(work=None), dict(out=None), dict(uv=None)):
        assert call(**kw) == -1 and "bmf_thresh_trace_wide: null pointer" in last_error(lib), kw
    assert call(k=64) == -1 and "bmf_thresh_trace64" in last_error(lib) and "k=64" in last_error(lib)
    assert call(k=129) == -1 and "k=129" in last_error(lib) and "k <= 128" in last_error(lib)
    for n_pairs in (0, -1, maxp + 1):
        assert call(n_pairs=n_pairs) == -1 and f"n_pairs={n_pairs} outside 1..{maxp}" in last_error(lib)
    for kw in (dict(m=0), dict(n=0), dict(ldf=71), dict(nseg=0), dict(nseg=8 * 10 + 65)):
        assert call(**kw) == -1 and "bmf_thresh_trace_wide" in last_error(lib), kw


def test_masked_wide_refusals():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.bmf_thresh_transform64_wide(None, 128, 10, 72, 0.5, 10.0, p, None, None) == -1 and "bmf_thresh_transform64_wide: null pointer" in last_error(lib)
    assert lib.bmf_thresh_transform64_wide(p, 128, 10, 72, 0.5, 10.0, None, None, None) == -1 and "null pointer" in last_error(lib)
    assert lib.bmf_thresh_transform64_wide(p, 128, 10, 64, 0.5, 10.0, p, None, None) == -1
    assert "k=64" in last_error(lib) and "bmf_thresh_transform64;" in last_error(lib)
    assert lib.bmf_thresh_transform64_wide(p, 128, 10, 129, 0.5, 10.0, p, None, None) == -1 and "k <= 128" in last_error(lib)
    assert lib.bmf_thresh_transform64_wide(p, 128, 129, 72, 0.5, 10.0, p, None, None) == -1 and "bad shape" in last_error(lib)

    def masked(ptr_=p, Us=p, dUs=p, dVs=p, partial=p, out=p, k=72, nseg=1, blocks=1):
        return lib.bmf_masked_thresh64_wide(ptr_, p, p, None, p, p, nseg, Us, dUs, p, dVs, k, partial, blocks, out, None)

    for kw in (dict(ptr_=None), dict(Us=None), dict(partial=None), dict(out=None)):
        assert masked(**kw) == -1 and "bmf_masked_thresh64_wide: null pointer" in last_error(lib), kw
    assert masked(dUs=None) == -1 and "both derivative factors or neither" in last_error(lib)
    assert masked(k=64) == -1 and "bmf_masked_thresh64_k" in last_error(lib) and "k=64" in last_error(lib)
    assert masked(k=129) == -1 and "k <= 128" in last_error(lib)
    for kw in (dict(nseg=0), dict(blocks=0), dict(blocks=65536)):
        assert masked(**kw) == -1 and "bmf_masked_thresh64_wide" in last_error(lib), kw


# ---- the class ------------------------------------------------------------------------------------------------------------------------
FIT = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)


def test_class_refuses_real_valued_data_above_64():
    from pybmf_amd.models import BinaryMFThreshold
    rs = np.random.RandomState(0)
    X = rs.rand(40, 30)
    mdl = BinaryMFThreshold(k=70, U=rs.rand(40, 70), V=rs.rand(30, 70), W="full", lamda=10, max_iter=2)
    with pytest.raises(NotImplementedError, match="k=70.*Boolean"):
        mdl.fit(X, **FIT)
    with pytest.raises(NotImplementedError, match="k=70.*Boolean"):
        BinaryMFThreshold(k=70, U=rs.rand(40, 70), V=rs.rand(30, 70), lamda=10, max_iter=2).fit(csr_matrix(np.round(X, 1)), **FIT)


def test_class_refuses_a_rank_above_128():
    from pybmf_amd.models import BinaryMFThreshold
    rs = np.random.RandomState(1)
    X = (rs.rand(40, 30) < 0.3).astype(np.uint8)
    mdl = BinaryMFThreshold(k=129, U=rs.rand(40, 129), V=rs.rand(30, 129), W="full", lamda=10, max_iter=2)
    with pytest.raises(NotImplementedError, match=r"^k=129: this build supports k <= 128$"):
        mdl.fit(X, **FIT)
