"""The kernels of csrc/thresh_grid.hip through the C ABI: the threshold panels bit for bit against F > thr, and the grid / pair-list
cover counts against the NumPy restatement (tests/thresh_grid_ref.py) AND against bmf_cover_count / bmf_cover_count_wide run once per
pair on the same panels (the existing path).  Integer kernels: every word and every count must be equal.

The count tests pack their panels on the host, so a fault of the panel kernel cannot hide one of the count kernels; the shapes that
span two column chunks and two row batches come from bmf_grid_cover_plan.  Padding words of X hold ones (no prediction bit lies
there), the counters are pre-loaded (the kernels add), outputs of the panel kernel are pre-filled with a marker and carry guard words."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import thresh_grid_ref as R  # noqa: E402

MARK32, MARK64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib as L
    return L, torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def round_up(x, m):
    return (x + m - 1) // m * m


def row_words(bits, rows_pad):
    """bool (rows, kb <= 64) -> uint64 [rows_pad]"""
    rows, kb = bits.shape
    out = np.zeros(rows_pad, np.uint64)
    out[:rows] = (bits.astype(np.uint64) << np.arange(kb, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)
    return out


def col_words(bits, kp, ldcb):
    """bool (rows, kb <= kp) -> uint32 [kp][ldcb], 32 rows per word"""
    rows, kb = bits.shape
    wide = np.zeros((kp, ldcb * 32), np.uint8)
    wide[:kb, :rows] = bits.T
    return np.packbits(wide, axis=1, bitorder="little").view(np.uint32)


# ---- bmf_thresh_panels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 3 * 128 + 5])
def test_panels(env, rows):
    L, d = env
    rows_pad = round_up(rows, 64)
    ld_min = rows_pad // 32
    ldcb = round_up(ld_min, 4) + 4                                   # wider than the panel: the words past rows_pad / 32 keep the marker
    for k in (1, 5, 32, 33, 64):
        kp = 32 if k <= 32 else 64
        rs = np.random.RandomState(1000 * rows + k)
        F = rs.rand(rows, k) * 2 - 0.5
        F[rs.rand(rows, k) < 0.2] = 0.0                              # exact zeros
        F[0, 0] = 0.0
        host = np.full((rows_pad, kp), np.nan)                       # NaN in the padding rows and columns
        host[:rows, :k] = F
        if rows_pad > rows:
            host[rows:, : max(1, k // 2)] = 1e300                    # and values above every threshold in some padding rows
        Fd = dev(host)
        for T in (1, 3, 40):
            thr = R.grid(F, T, columnwise=True)                      # (T, k); thr[0] is each column's minimum: equality by construction
            assert (F == thr[0][None, :]).any(axis=0).all() and (F == 0.0).any()
            rb = dev(np.full(T * rows_pad + 8, MARK64, np.uint64))
            cb = dev(np.full(T * kp * ldcb + 8, MARK32, np.uint32))
            td = dev(thr)
            L.check(L.lib.bmf_thresh_panels(L.ptr(Fd), rows_pad, rows, k, kp, L.ptr(td), T, L.ptr(rb), L.ptr(cb), ldcb, stream()), "bmf_thresh_panels")
            got_rb = rb.cpu().numpy().view(np.uint64)
            got_cb = cb.cpu().numpy().view(np.uint32)
            assert (got_rb[T * rows_pad:] == MARK64).all() and (got_cb[T * kp * ldcb:] == MARK32).all()      # guard words
            got_cb = got_cb[: T * kp * ldcb].reshape(T, kp, ldcb)
            assert (got_cb[:, :, ld_min:] == MARK32).all()
            for t in range(T):
                bits = F > thr[t][None, :]
                assert np.array_equal(got_rb[t * rows_pad:(t + 1) * rows_pad], row_words(bits, rows_pad)), (k, T, t)
                assert np.array_equal(got_cb[t, :, :ld_min], col_words(bits, kp, ldcb)[:, :ld_min]), (k, T, t)
            # either output alone
            rb2 = dev(np.full(T * rows_pad, MARK64, np.uint64))
            L.check(L.lib.bmf_thresh_panels(L.ptr(Fd), rows_pad, rows, k, kp, L.ptr(td), T, L.ptr(rb2), None, 0, stream()), "bmf_thresh_panels")
            assert np.array_equal(rb2.cpu().numpy().view(np.uint64), got_rb[: T * rows_pad])


# ---- bmf_grid_cover_count / bmf_pairs_cover_count ------------------------------------------------------------------------------------
def plan(L, rows_pad, words, panels):
    cw, rpb, ab = C.c_int(0), C.c_int(0), C.c_int(0)
    L.check(L.lib.bmf_grid_cover_plan(rows_pad, words, panels, C.byref(cw), C.byref(rpb), C.byref(ab)), "bmf_grid_cover_plan")
    return cw.value, rpb.value, ab.value


def shapes(L):
    cw, rpb, _ = plan(L, 64, 4, 1)
    return {"1x1": (1, 1), "70x45": (70, 45), "515x1030": (515, 1030), "two_chunks": (70, 32 * cw + 40), "two_batches": (rpb + 3, 45)}


SHAPE_NAMES = ["1x1", "70x45", "515x1030", "two_chunks", "two_batches"]


def make_case(m, n, k, kind, seed):
    rs = np.random.RandomState(seed)
    Ub, Vb = rs.rand(m, k) < min(0.3, 3.0 / k + 0.05), rs.rand(n, k) < min(0.3, 3.0 / k + 0.05)
    U = Ub * rs.uniform(0.3, 1.0, size=(m, k)) + 0.02 * rs.rand(m, k)
    V = Vb * rs.uniform(0.3, 1.0, size=(n, k)) + 0.02 * rs.rand(n, k)
    if kind == "ones":
        X = np.ones((m, n), bool)
    elif kind == "zeros":
        X = np.zeros((m, n), bool)
    else:
        X = R.product(Ub, Vb) ^ (rs.rand(m, n) < 0.03)
    return X, U, V


class Panels:
    """X and the host-packed panels of thr_u (A, k) / thr_v (B, k) on the device, one or two 64-column blocks."""

    def __init__(self, X, U, V, thr_u, thr_v):
        m, n = X.shape
        k = U.shape[1]
        self.k, self.nb, self.kp = k, (1 if k <= 64 else 2), (32 if k <= 32 else 64)
        self.rows_pad, self.words = round_up(m, 64), round_up((n + 31) // 32, 4)
        self.ldx, self.ldcb = self.words + 4, self.words + 8
        xb = np.ones((self.rows_pad, self.ldx * 32), np.uint8)         # padding bits of X are ones
        xb[:m, :n] = X
        self.X = dev(np.packbits(xb, axis=1, bitorder="little").view(np.uint32))
        self.A, self.B = len(thr_u), len(thr_v)
        self.Ub = [U > t[None, :] for t in thr_u]
        self.Vb = [V > t[None, :] for t in thr_v]
        self.rb, self.cb = [], []
        for b in range(self.nb):
            sl = slice(64 * b, min(k, 64 * b + 64))
            self.rb.append(dev(np.stack([row_words(bits[:, sl], self.rows_pad) for bits in self.Ub])))
            self.cb.append(dev(np.stack([col_words(bits[:, sl], self.kp, self.ldcb) for bits in self.Vb])))
        self.Xh = X

    def head(self, L):
        second = (L.ptr(self.rb[1]), L.ptr(self.cb[1])) if self.nb == 2 else (None, None)
        return (L.ptr(self.X), self.rows_pad, self.ldx, self.words, L.ptr(self.rb[0]), second[0], self.A, L.ptr(self.cb[0]), second[1], self.ldcb,
                self.kp, self.B)

    def expected(self):
        return np.array([[R.counts_of(self.Xh, ub, vb) for vb in self.Vb] for ub in self.Ub], dtype=np.int64)

    def single(self, L, a, b):
        """The existing path: one cover count of the pair (a, b) on the same panels."""
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        if self.nb == 1:
            L.check(L.lib.bmf_cover_count(L.ptr(self.X), self.rows_pad, self.ldx, self.words, L.ptr(self.rb[0][a]), L.ptr(self.cb[0][b]), self.ldcb, self.kp,
                                          L.ptr(cnt), None, stream()), "bmf_cover_count")
        else:
            L.check(L.lib.bmf_cover_count_wide(L.ptr(self.X), self.rows_pad, self.ldx, self.words, L.ptr(self.rb[0][a]), L.ptr(self.rb[1][a]),
                                               L.ptr(self.cb[0][b]), L.ptr(self.cb[1][b]), self.ldcb, L.ptr(cnt), stream()), "bmf_cover_count_wide")
        return cnt


def grid_counts(L, P, preload):
    cnt = dev(preload)
    L.check(L.lib.bmf_grid_cover_count(*P.head(L), L.ptr(cnt), stream()), "bmf_grid_cover_count")
    return cnt.cpu().numpy()


def pair_counts(L, P, pairs, preload):
    cnt, pd = dev(preload), dev(np.asarray(pairs, dtype=np.int32))
    L.check(L.lib.bmf_pairs_cover_count(*P.head(L), L.ptr(pd), len(pairs), L.ptr(cnt), stream()), "bmf_pairs_cover_count")
    return cnt.cpu().numpy()


@pytest.mark.parametrize("k", [5, 64, 72, 128])
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_grid_and_pair_counts(env, shape, k):
    L, d = env
    m, n = shapes(L)[shape]
    rows_pad, words = round_up(m, 64), round_up((n + 31) // 32, 4)
    cw, rpb, _ = plan(L, rows_pad, words, 5)
    if shape == "two_chunks":
        assert words > cw
    if shape == "two_batches":
        assert rows_pad > rpb
    grids = [(1, 1), (3, 5)] + ([(40, 40)] if shape == "70x45" else [])
    for kind in ("ones", "zeros", "planted"):
        X, U, V = make_case(m, n, k, kind, seed=7 * k + len(shape))
        for A, B in grids:
            if (A, B) == (40, 40) and kind != "planted":
                continue
            thr_u, thr_v = R.grid(U, A, columnwise=True), R.grid(V, B, columnwise=True)     # ascending in every column: nested panels
            P = Panels(X, U, V, thr_u, thr_v)
            want = P.expected()
            rs = np.random.RandomState(A * 100 + B)
            pre = rs.randint(1, 1000, size=(A, B, 2)).astype(np.int64)                         # the kernels add to what the counters hold
            got = grid_counts(L, P, pre)
            assert np.array_equal(got - pre, want), (kind, A, B)
            # TP and FP cannot grow with either threshold
            assert (np.diff(want, axis=0) <= 0).all() and (np.diff(want, axis=1) <= 0).all()
            if kind == "ones":
                assert (want[:, :, 1] == 0).all()
            if kind == "zeros":
                assert (want[:, :, 0] == 0).all()
            # the existing path, one launch per pair on the same panels
            singles = torch.stack([P.single(L, a, b) for a in range(A) for b in range(B)]).cpu().numpy().reshape(A, B, 2)
            assert np.array_equal(singles, want), (kind, A, B)
            # the pair list on every pair of the grid, with one pair out of range (it adds nothing)
            pairs = [(a, b) for a in range(A) for b in range(B)] + [(-1, 0), (A, 0), (0, B)]
            pre_p = rs.randint(1, 1000, size=(len(pairs), 2)).astype(np.int64)
            got_p = pair_counts(L, P, pairs, pre_p) - pre_p
            assert np.array_equal(got_p[: A * B].reshape(A, B, 2), want), (kind, A, B)
            assert (got_p[A * B:] == 0).all()


@pytest.mark.parametrize("k", [5, 72])
def test_pair_list_on_shuffled_panels(env, k):
    """Panels in no order (not nested), pairs drawn with repeats: the pair list equals the restatement."""
    L, d = env
    m, n = 130, 300
    X, U, V = make_case(m, n, k, "planted", seed=99 + k)
    rs = np.random.RandomState(5 + k)
    thr_u, thr_v = R.grid(U, 7, columnwise=True), R.grid(V, 6, columnwise=True)
    thr_u, thr_v = thr_u[rs.permutation(7)], thr_v[rs.permutation(6)]
    for c in range(k):                                               # and every column in an order of its own
        thr_u[:, c], thr_v[:, c] = thr_u[rs.permutation(7), c], thr_v[rs.permutation(6), c]
    P = Panels(X, U, V, thr_u, thr_v)
    want = P.expected()
    pairs = np.stack([rs.randint(0, 7, size=50), rs.randint(0, 6, size=50)], axis=1)
    pre = rs.randint(1, 1000, size=(50, 2)).astype(np.int64)
    got = pair_counts(L, P, pairs, pre) - pre
    assert np.array_equal(got, np.array([want[a, b] for a, b in pairs]))


def test_more_panels_than_one_batch(env):
    """A above the panels one launch walks: the entry point cuts the grid into batches, each nested in itself."""
    L, d = env
    _, _, a_batch = plan(L, 128, 4, 3)
    A, B = a_batch + 6, 3
    X, U, V = make_case(70, 45, 5, "planted", seed=321)
    P = Panels(X, U, V, R.grid(U, A, columnwise=True), R.grid(V, B, columnwise=True))
    pre = np.full((A, B, 2), 5, np.int64)
    assert np.array_equal(grid_counts(L, P, pre) - pre, P.expected())
