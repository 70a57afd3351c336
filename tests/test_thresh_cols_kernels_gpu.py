"""bmf_thresh_cols64 (csrc/thresh_cols.hip) called directly, against the NumPy restatement (tests/thresh_cols_ref.py): 16, 32 and 64
lanes per point, k not a power of two, rows longer than one 128-cell segment, a full row, an all-zero row, a single-cell matrix and
the 1 x 1 case; batches that need several calls; factors with NaN in their padding; guard words around the records."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import thresh_cols_ref as R  # noqa: E402

SHAPES = [(70, 45, 5, 0.3), (300, 333, 20, 0.1), (260, 200, 40, 0.5), (33, 700, 64, 0.9), (129, 31, 33, 0.4), (65, 130, 17, 0.2), (64, 64, 1, 0.5),
          (50, 40, 16, "one cell"), (1, 1, 1, "full")]
N_POINTS = 37
GUARD, SENTINEL = 2, -777.25   # words in front of and behind the records (two: the record block stays 16-byte aligned)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib as L
    return L, torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, d):
    return torch.from_numpy(np.array(a)).to(d)   # (a copy: the cases are read-only)


_cases = {}


def case(m, n, k, dens):
    """(X, U, V, points) of a shape, built once and left unchanged.  The factor columns have different scales; every point has one
    column of U thresholded above all its entries and one column of V below all of them."""
    key = (m, n, k, dens)
    if key not in _cases:
        rs = np.random.RandomState(1000 * m + k)
        if dens == "one cell":
            X = np.zeros((m, n), np.uint8)
            X[1, 2] = 1
        elif dens == "full":
            X = np.ones((m, n), np.uint8)
        else:
            X = (rs.rand(m, n) < dens).astype(np.uint8)
            X[0, :] = 1
            if m > 3:
                X[3, :] = 0
        scale = rs.uniform(0.5, 3.0, size=k)
        U, V = rs.rand(m, k) * scale, rs.rand(n, k) * scale
        pts = []
        for p in range(N_POINTS):
            us, vs = rs.uniform(0.1, 0.9, size=k) * scale, rs.uniform(0.1, 0.9, size=k) * scale
            us[p % k] = U[:, p % k].max() + 1.0
            vs[(p + 1) % k] = V[:, (p + 1) % k].min() - 1.0
            pts.append(np.concatenate([us, vs]))
        pts = np.array(pts)
        for a in (X, U, V, pts):
            a.setflags(write=False)
        _cases[key] = (X, U, V, pts)
    return _cases[key]


_refs = {}


def reference(key, lam):
    """F and dF of the restatement at the points of a shape, computed once."""
    if (key, lam) not in _refs:
        X, U, V, pts = case(*key)
        Xf = X.astype(np.float64)
        _refs[(key, lam)] = (np.array([R.F(Xf, U, V, x, lam) for x in pts]), np.array([R.dF(Xf, U, V, x, lam) for x in pts]))
    return _refs[(key, lam)]


def segments(X, d):
    """The ones of X as the segment list (<= 128 cells of one row each, longest first)."""
    m = X.shape[0]
    rows, cols = np.nonzero(X)
    cnt = np.bincount(rows, minlength=m)
    starts = np.cumsum(cnt) - cnt
    seg = [(i, starts[i] + a, min(128, cnt[i] - a)) for i in range(m) for a in range(0, cnt[i], 128)]
    seg.sort(key=lambda t: -t[2])
    return (dev(np.array([t[0] for t in seg], np.int32), d), dev(np.array([t[1] for t in seg], np.int64), d),
            dev(np.array([t[2] for t in seg], np.int32), d), len(seg), dev(cols.astype(np.int32), d), float(len(rows)))


class Setup:
    """Device state of one shape: factors with ldf > k, extra rows and NaN in all the padding; workspace; guarded records."""

    def __init__(self, L, d, X, U, V):
        self.L, self.d = L, d
        self.m, self.n = X.shape
        self.k = U.shape[1]
        self.ldf = self.k + 3
        self.Ud = torch.full((self.m + 5, self.ldf), float("nan"), dtype=torch.float64, device=d)
        self.Vd = torch.full((self.n + 3, self.ldf), float("nan"), dtype=torch.float64, device=d)
        self.Ud[: self.m, : self.k], self.Vd[: self.n, : self.k] = dev(U, d), dev(V, d)
        self.seg = segments(X, d)
        self.maxp = L.lib.bmf_thresh_cols64_max_points(self.k)
        self.work = torch.zeros(int(L.lib.bmf_thresh_cols64_work(self.m, self.n, self.k, self.maxp)), dtype=torch.float64, device=d)
        self.rec = 2 + 2 * self.k
        self.buf = torch.zeros(2 * GUARD + self.rec * self.maxp + 1, dtype=torch.float64).pin_memory()
        self.x_pin = torch.zeros(self.maxp * 2 * self.k, dtype=torch.float64).pin_memory()
        self.seq = 0.0

    def run(self, pts, lam, grad):
        """Records [point][1 + 2k] = (2 F, dF...) of `pts`, a batch per call; x alternates between device and pinned host memory."""
        L, k, rec = self.L, self.k, self.rec
        res = []
        for call, a in enumerate(range(0, len(pts), self.maxp)):
            part = np.ascontiguousarray(pts[a:a + self.maxp])
            if call % 2:
                self.x_pin.numpy()[: part.size] = part.ravel()
                x = self.x_pin
            else:
                x = dev(part, self.d)
            self.seq += 1.0
            o = self.buf.numpy()
            o[:] = SENTINEL
            sr, sb, sl, nseg, idx, sx = self.seg
            L.check(L.lib.bmf_thresh_cols64(L.ptr(sr), L.ptr(sb), L.ptr(sl), nseg, L.ptr(idx), self.m, self.n, L.ptr(self.Ud), L.ptr(self.Vd), self.ldf, k,
                                            L.ptr(x), len(part), float(lam), sx, int(grad), L.ptr(self.work), C.c_void_p(self.buf.data_ptr() + 8 * GUARD),
                                            self.seq, stream()))
            torch.cuda.synchronize()
            body = o[GUARD: GUARD + rec * len(part) + 1]
            assert (o[:GUARD] == SENTINEL).all() and (o[GUARD + rec * len(part) + 1:] == SENTINEL).all()   # the guards, and the slots of points not asked for
            assert body[rec * len(part)] == self.seq and (body[0:rec * len(part):rec] == self.seq).all()   # every stamp
            recs = body[: rec * len(part)].reshape(len(part), rec)[:, 1:].copy()
            if not grad:
                assert (recs[:, 1:] == SENTINEL).all()   # the gradient words are not written
            res.append(recs)
        return np.concatenate(res)


@pytest.mark.parametrize("m,n,k,dens", SHAPES)
def test_thresh_cols64_shapes(env, m, n, k, dens):
    """F to rel 1e-11 (abs 1e-9), dF within 1e-9 (max|dF| + 1): the project's gates for the scalar form (test_thresh_trace64_shapes).
    lamda = 10 with the gradient, lamda = 100 without; 2 F bit-equal with and without the gradient; a repeated call bit-equal."""
    L, d = env
    X, U, V, pts = case(m, n, k, dens)
    S = Setup(L, d, X, U, V)
    Fw, dFw = reference((m, n, k, dens), 10)
    got = S.run(pts, 10, True)
    dev_f = np.abs(0.5 * got[:, 0] - Fw) / np.maximum(np.abs(Fw) * 1e-11, 1e-9)
    dev_g = np.abs(got[:, 1:] - dFw).max(axis=1) / (1e-9 * (np.abs(dFw).max(axis=1) + 1.0))
    print(f"{m}x{n} k={k}: lamda=10 F at {dev_f.max():.1e} of its gate, dF at {dev_g.max():.1e}")
    for i in range(N_POINTS):
        assert 0.5 * got[i, 0] == pytest.approx(Fw[i], rel=1e-11, abs=1e-9)
        assert np.abs(got[i, 1:] - dFw[i]).max() <= 1e-9 * (np.abs(dFw[i]).max() + 1.0)
    again = S.run(pts, 10, True)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))                  # the same call, the same bits
    plain = S.run(pts, 10, False)
    assert np.array_equal(plain[:, 0].view(np.uint64), got[:, 0].view(np.uint64))      # 2 F does not depend on want_grad
    Fw100, _ = reference((m, n, k, dens), 100)
    got100 = S.run(pts, 100, False)
    for i in range(N_POINTS):
        assert 0.5 * got100[i, 0] == pytest.approx(Fw100[i], rel=1e-11, abs=1e-9)


@pytest.mark.parametrize("m,n,k,dens", [(70, 45, 5, 0.3), (300, 333, 20, 0.1), (33, 700, 64, 0.9)])
def test_constant_vectors_agree_with_the_scalar_kernel(env, m, n, k, dens):
    """With all us equal to u and all vs equal to v the record agrees with bmf_thresh_trace64 at (u, v): F to rel 1e-11, the two halves
    of the gradient, summed, to 1e-9 of the scale."""
    L, d = env
    X, U, V, _ = case(m, n, k, dens)
    S = Setup(L, d, X, U, V)
    rs = np.random.RandomState(5)
    uv = [(0.1 + 2.0 * rs.rand(), 0.1 + 2.0 * rs.rand()) for _ in range(S.maxp)]
    got = S.run(np.array([np.concatenate([np.full(k, u), np.full(k, v)]) for u, v in uv]), 10, True)
    maxp = L.lib.bmf_thresh_trace64_max_pairs(k)
    assert maxp == S.maxp
    work = torch.zeros(int(L.lib.bmf_thresh_trace64_work(m, n, k, maxp)), dtype=torch.float64, device=d)
    out_host = torch.zeros(4 * maxp + 1, dtype=torch.float64).pin_memory()
    flat = (C.c_double * (2 * maxp))(*[x for p_ in uv for x in p_])
    sr, sb, sl, nseg, idx, sx = S.seg
    L.check(L.lib.bmf_thresh_trace64(L.ptr(sr), L.ptr(sb), L.ptr(sl), nseg, L.ptr(idx), m, n, L.ptr(S.Ud), L.ptr(S.Vd), S.ldf, k, flat, maxp, 10.0, sx, 1,
                                     L.ptr(work), L.ptr(out_host), 1.0, stream()))
    torch.cuda.synchronize()
    o = out_host.numpy()
    for i in range(maxp):
        assert got[i, 0] == pytest.approx(o[4 * i + 1], rel=1e-11)
        scale = max(abs(o[4 * i + 2]), abs(o[4 * i + 3])) + 1.0
        assert abs(got[i, 1:1 + k].sum() - o[4 * i + 2]) <= 1e-9 * scale and abs(got[i, 1 + k:].sum() - o[4 * i + 3]) <= 1e-9 * scale
