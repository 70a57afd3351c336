"""The objective kernels of BinaryMFThreshold at a rank 64 < k <= 128 (csrc/thresh_wide.hip) through the C ABI, against the fp64 oracle
(orc.thresh_F / orc.thresh_dF; the cell-list form against tests/masked_ref.py) at random fp64 factors, and on the grids of golden g33.

Gates, those of the k <= 64 forms (test_thresh_trace64_shapes, test_masked_thresh64_cell_by_cell): F rel 1e-11 (abs 1e-9), dF within
1e-9 (max|dF| + 1).  Every sum is fp64 in a fixed order: the trace form was measured at 3e-15 of the literal one at k <= 64, and twice
the terms does not use a margin of three thousand."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import masked_ref as R  # noqa: E402
import oracle as orc  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. the trace form
# ---------------------------------------------------------------------------------------------------------------------------------------
def trace_inputs(X):
    """The ones of X as the segment list bmf_thresh_trace64 / _wide take (<= 128 cells of one row each, longest first)."""
    m = X.shape[0]
    rows, cols = np.nonzero(X)
    counts = np.bincount(rows, minlength=m)
    starts = np.cumsum(counts) - counts
    seg = [(i, starts[i] + a, min(128, counts[i] - a)) for i in range(m) for a in range(0, counts[i], 128)]
    seg.sort(key=lambda t: -t[2])
    return (dev(np.array([t[0] for t in seg], np.int32)), dev(np.array([t[1] for t in seg], np.int64)), dev(np.array([t[2] for t in seg], np.int32)),
            len(seg), dev(cols.astype(np.int32)), float(len(rows)))


class Trace:
    """One matrix and one pair of factors on the device.  The factor arrays carry NaN wherever the kernels must not look: columns >= k
    (the leading dimension is k + 3) and rows >= m / n."""

    def __init__(self, X, U, V):
        from pybmf_amd import _lib as L
        self.L, (self.m, self.n), self.k = L, X.shape, U.shape[1]
        self.ldf = self.k + 3
        self.Ud = torch.full((self.m + 5, self.ldf), float("nan"), dtype=torch.float64, device="cuda")
        self.Vd = torch.full((self.n + 3, self.ldf), float("nan"), dtype=torch.float64, device="cuda")
        self.Ud[:self.m, :self.k], self.Vd[:self.n, :self.k] = dev(U), dev(V)
        self.seg = trace_inputs(X)
        self.maxp = L.lib.bmf_thresh_trace_wide_max_pairs(self.k)
        self.work = torch.zeros(int(L.lib.bmf_thresh_trace_wide_work(self.m, self.n, self.k, self.maxp)), dtype=torch.float64, device="cuda")
        self.out_host = torch.zeros(4 * self.maxp + 1, dtype=torch.float64).pin_memory()
        self.seq = 0.0

    def __call__(self, pts, lam, grad):
        """[(F, dF_u, dF_v)] at pts, in calls of at most max_pairs pairs; checks the stamps of every call."""
        L = self.L
        seg_row, seg_beg, seg_len, nseg, idx, sx = self.seg
        res = []
        for a in range(0, len(pts), self.maxp):
            part = pts[a:a + self.maxp]
            uv = (C.c_double * (2 * len(part)))(*[x for p_ in part for x in p_])
            self.seq += 1.0
            L.check(L.lib.bmf_thresh_trace_wide(L.ptr(seg_row), L.ptr(seg_beg), L.ptr(seg_len), nseg, L.ptr(idx), self.m, self.n, L.ptr(self.Ud),
                                                L.ptr(self.Vd), self.ldf, self.k, uv, len(part), float(lam), sx, int(grad), L.ptr(self.work),
                                                L.ptr(self.out_host), self.seq, stream()), "bmf_thresh_trace_wide")
            torch.cuda.synchronize()
            o = self.out_host.numpy()
            assert o[4 * len(part)] == self.seq               # the sequence word is written last
            assert (o[0:4 * len(part):4] == self.seq).all()   # and every pair carries the call's stamp behind its results
            res += [(0.5 * o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]) for i in range(len(part))]
        return res


@pytest.mark.parametrize("m,n,dens", [(37, 150, 0.95), (130, 100, 0.3), (257, 300, 0.1), (50, 40, 0.0)])
@pytest.mark.parametrize("k", [65, 97, 128])
def test_thresh_trace_wide_shapes(k, m, n, dens):
    """One column, half a block and a full block in the second half; rows of two segments (37 x 150), more than one Gram chunk (257 rows and
    300 rows + the zero row: two chunks each), a matrix with a single one; 1 pair, max_pairs pairs and max_pairs + 1 points (two calls)."""
    rs = np.random.RandomState(1000 * k + m)
    X = (rs.rand(m, n) < dens).astype(np.uint8)
    if dens > 0:
        X[0, :] = 1
        X[3, :] = 0
    else:
        X[1, 2] = 1   # (one cell: the list must not be empty)
    U, V = rs.rand(m, k), rs.rand(n, k)
    T = Trace(X, U, V)
    assert T.maxp >= 2
    pts = [(0.1 + 0.8 * rs.rand(), 0.1 + 0.8 * rs.rand()) for _ in range(T.maxp + 1)]
    Xf = X.astype(np.float64)
    want_F = {lam: [orc.thresh_F(Xf, None, U, V, u, v, lam) for (u, v) in pts] for lam in (10, 100)}
    want_dF = [orc.thresh_dF(Xf, None, U, V, u, v, 10) for (u, v) in pts]
    worst_f = worst_g = 0.0
    for lam, grad in ((10, True), (100, False)):
        for batch in (pts[:1], pts[:T.maxp], pts):
            got = T(batch, lam, grad)
            assert len(got) == len(batch)
            for i, g in enumerate(got):
                worst_f = max(worst_f, abs(g[0] - want_F[lam][i]) / max(abs(want_F[lam][i]), 1e-300))
                assert g[0] == pytest.approx(want_F[lam][i], rel=1e-11, abs=1e-9)
                if grad:
                    scale = np.abs(want_dF[i]).max() + 1.0
                    worst_g = max(worst_g, np.abs(np.array(g[1:]) - want_dF[i]).max() / scale)
                    assert np.abs(np.array(g[1:]) - want_dF[i]).max() <= 1e-9 * scale
                else:
                    assert g[1] == 0.0 and g[2] == 0.0
            if len(batch) == len(pts):
                whole = got
            elif len(batch) == 1:
                alone = got
        assert alone[0] == whole[0]                                                   # the same bits, alone or as one pair of eight
        assert T(pts, lam, grad) == whole                                             # and when repeated
    # F with the gradient riding along equals F without it, bit for bit
    assert [g[0] for g in T(pts, 10, False)] == [g[0] for g in T(pts, 10, True)]
    print(f"trace_wide k={k} {m}x{n} dens={dens}: F rel {worst_f:.3g}, dF / (max|dF| + 1) {worst_g:.3g}")


@functools.lru_cache(maxsize=None)
def g33():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return np.load(os.path.join(here, "g33_threshold_wide.npz")), json.load(open(os.path.join(here, "g33_threshold_wide.json")))


@pytest.mark.parametrize("name,lam", [("a", 10), ("a", 100), ("b", 100), ("c", 10)])
def test_thresh_trace_wide_on_the_reference_grid(name, lam):
    """The reference's own F and dF on the 4 x 4 grid of golden g33 (16 points: two calls), with and without the gradient."""
    z, meta = g33()
    n = z[f"{name}_shape"][1]
    X = np.unpackbits(z[f"{name}_X_bits"], axis=1, bitorder="little")[:, :n]
    T = Trace(X, z[f"{name}_U"], z[f"{name}_V"])
    pts = [(u, v) for u in meta["grid"] for v in meta["grid"]]
    Fg, dFg = z[f"{name}_F_grid_lam{lam}"].ravel(), z[f"{name}_dF_grid_lam{lam}"].reshape(-1, 2)
    got_f, got_g = T(pts, lam, False), T(pts, lam, True)
    np.testing.assert_allclose([g[0] for g in got_f], Fg, rtol=1e-11)
    assert [g[0] for g in got_f] == [g[0] for g in got_g]
    assert np.abs(np.array([g[1:] for g in got_g]) - dFg).max() <= 1e-9 * (np.abs(dFg).max() + 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. observed cells: bmf_thresh_transform64_wide + bmf_masked_thresh64_wide
# ---------------------------------------------------------------------------------------------------------------------------------------
N = 210
# an empty row, rows on each side of the 64-cell segment boundary and of the four-cell step, rows of three and four segments
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 130, 200] + np.random.RandomState(7).randint(1, 100, size=12).tolist()
M = len(LENGTHS)


@functools.lru_cache(maxsize=None)
def cells(weights):
    rows, cols, x, w = R.make_cells(LENGTHS, N, np.random.RandomState(300 + weights), real=False, weights=weights)
    assert (x == 0).any() and (x == 1).any() and np.bincount(rows, minlength=M).tolist() == LENGTHS
    return rows, cols, x, w


@functools.lru_cache(maxsize=None)
def obs(weights):
    from pybmf_amd.engine import SparseObs
    rows, cols, x, w = cells(weights)
    return SparseObs(rows, cols, x, w, (M, N))


def masked_eval(ls, U, V, rows_u, rows_v, u, v, lam, grad, blocks):
    """(sum (w r)^2, g1, g2, untouched word) through the device transform and the cell pass; the factor arrays are rows_pad x 128 with NaN
    in the padding columns and rows."""
    from pybmf_amd import _lib as L
    k = U.shape[1]
    mp, np_ = rows_u + 7, rows_v + 2
    Ud, Vd = torch.full((mp, 128), float("nan"), dtype=torch.float64, device="cuda"), torch.full((np_, 128), float("nan"), dtype=torch.float64, device="cuda")
    Ud[:rows_u, :k], Vd[:rows_v, :k] = dev(U), dev(V)
    Us, dUs = torch.full((mp, 128), -1.0, dtype=torch.float64, device="cuda"), torch.full((mp, 128), -1.0, dtype=torch.float64, device="cuda")
    Vs, dVs = torch.full((np_, 128), -1.0, dtype=torch.float64, device="cuda"), torch.full((np_, 128), -1.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_thresh_transform64_wide(L.ptr(Ud), mp, rows_u, k, u, lam, L.ptr(Us), L.ptr(dUs) if grad else None, stream()))
    L.check(L.lib.bmf_thresh_transform64_wide(L.ptr(Vd), np_, rows_v, k, v, lam, L.ptr(Vs), L.ptr(dVs) if grad else None, stream()))
    for S_, rows in ((Us, rows_u), (Vs, rows_v)) + (((dUs, rows_u), (dVs, rows_v)) if grad else ()):
        h = S_.cpu().numpy()
        assert np.isfinite(h).all() and (h[rows:] == 0).all() and (h[:, k:] == 0).all()       # transformed padding is exact zero
    partial = torch.full((4 * blocks,), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_masked_thresh64_wide(L.ptr(ls["ptr"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), L.ptr(ls["wgt"]), L.ptr(ls["seg_row"]), L.ptr(ls["seg_beg"]),
                                           ls["nseg"], L.ptr(Us), L.ptr(dUs) if grad else None, L.ptr(Vs), L.ptr(dVs) if grad else None, k,
                                           L.ptr(partial), blocks, L.ptr(out), stream()))
    return out.cpu().numpy(), Us.cpu().numpy()[:rows_u, :k], (dUs.cpu().numpy()[:rows_u, :k] if grad else None)


@pytest.mark.parametrize("lamda", [10.0, 100.0])
@pytest.mark.parametrize("weights", [False, True], ids=["mask", "weights"])
@pytest.mark.parametrize("k", [65, 100, 128])
def test_masked_thresh64_wide_cell_by_cell(k, weights, lamda):
    """The cell pass at 128 columns behind the device transform, as BinaryMFThreshold runs it: a cell list with explicit zeros, weights in
    {0.5, 1, 3} (squared in F, once in dF), an empty row, rows of up to four segments; 1 and 3 workgroups make the segment loop stride;
    `out` is written (not added to) and bit-identical when repeated."""
    rows, cols, x, w = cells(weights)
    rs = np.random.RandomState(50 + k)
    U, V = rs.rand(M, k), rs.rand(N, k)
    u, v = 0.45, 0.6
    wf, wg1, wg2 = R.thresh_ref(rows, cols, x, w, U, V, u, v, lamda)
    ls = obs(weights).csr
    nseg = ls["nseg"]
    assert nseg == sum((ln + 63) // 64 for ln in LENGTHS)
    scale = max(abs(wg1), abs(wg2)) + 1.0
    for grad in (False, True):
        for blocks in (1, 3, (nseg + 3) // 4):
            o, S, D = masked_eval(ls, U, V, M, N, u, v, lamda, grad, blocks)
            print(f"masked_wide k={k} lamda={lamda:g} grad={grad} blocks={blocks}: F rel {abs(o[0] - wf) / wf:.3g}, dF {abs(o[1] - wg1):.3g} "
                  f"{abs(o[2] - wg2):.3g} scale {scale:.3g}")
            assert o[3] == -3.0                                           # three words written, the fourth is not the kernel's
            assert 0.5 * o[0] == pytest.approx(0.5 * wf, rel=1e-11, abs=1e-9)
            if grad:
                assert abs(o[1] - wg1) <= 1e-9 * scale and abs(o[2] - wg2) <= 1e-9 * scale
            else:
                assert o[1] == 0.0 and o[2] == 0.0                        # F only: the gradient words are written as zeros
            assert np.array_equal(o, masked_eval(ls, U, V, M, N, u, v, lamda, grad, blocks)[0])
    # the transform itself, to the 1e-14 of the k <= 64 form
    np.testing.assert_allclose(S, orc.stable_sigmoid((U - u) * lamda), rtol=1e-14, atol=0)
    np.testing.assert_allclose(D, orc.thresh_dXdx(U, u, lamda), rtol=1e-14, atol=0)


@pytest.mark.parametrize("case,prefix", [("d", "d"), ("e", "e_train")])
def test_masked_thresh64_wide_on_the_reference_grid(case, prefix):
    """The reference's own F and dF over the stored cells of golden g33 (cases d and e: W='mask', k = 72)."""
    from pybmf_amd.engine import SparseObs
    z, meta = g33()
    m, n = (int(s) for s in z["a_shape"])
    U, V = z["a_U"], z["a_V"]
    ls = SparseObs(z[prefix + "_rows"], z[prefix + "_cols"], z[prefix + "_vals"].astype(np.float64), None, (m, n)).csr
    lam = float(meta[case]["lamda"])
    Fg, dFg = z[f"{case}_F_grid"], z[f"{case}_dF_grid"]
    scale = np.abs(dFg).max() + 1.0
    for i, a in enumerate(meta["grid"]):
        for j, b in enumerate(meta["grid"]):
            o, _, _ = masked_eval(ls, U, V, m, n, a, b, lam, True, 64)
            assert 0.5 * o[0] == pytest.approx(Fg[i, j], rel=1e-11, abs=1e-9)
            assert np.abs(o[1:3] - dFg[i, j]).max() <= 1e-9 * scale
            assert 0.5 * masked_eval(ls, U, V, m, n, a, b, lam, False, 64)[0][0] == pytest.approx(Fg[i, j], rel=1e-11, abs=1e-9)
