"""The dense objective sums by direct C ABI calls, cell by cell: csrc/residual.hip (residual_kernel in its six instantiations,
product_kernel, thresh_transform_kernel), csrc/thresh64.hip (transform64_pair_kernel, dense64_kernel<GRAD>, sum_partials_kernel),
csrc/mae.hip (mae_kernel<32|64>, mae32_kernel<32|64, tiled|plain>) and csrc/resid_f32.hip (resid_f32_ring_kernel<32|64>).

A sum is checked cell by cell in two ways (tests/objective_ref.py, proved by tests/test_objective_sums_cpu.py): on inputs whose every
term, every fp32 lane partial and the fp64 total are exact and differ from cell to cell, so that the comparison is ==; and by probes
that leave ONE cell non-zero.  Every test that names a launch path asserts that path first, from the library's own plan queries
(bmf_residual_plan, bmf_mae_plan, bmf_residual_tiled_plan): a changed launch rule fails the test instead of moving it to another path.

Bounds that are not == are the project's existing ones, cited where they are used."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import objective_ref as R  # noqa: E402

BIG = 1e30          # poison for factor rows the masking kernels must ignore: finite, its products overflow to inf
SENTINEL = -7.25


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=None):
    a = np.array(a, dtype=dtype, order="C")     # a copy: the shared host inputs are read-only
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def zeros(n, dtype=torch.float64):
    return torch.zeros(n, dtype=dtype, device="cuda")


def at(t, elems):
    """device pointer `elems` elements into tensor t"""
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def plan(fn, a, b):
    x, y = C.c_int(-1), C.c_int(-1)
    assert fn(a, b, C.byref(x), C.byref(y)) == 0
    return x.value, y.value


def up(x, q):
    return -(-x // q) * q


def kk(kp):
    """a rank that leaves padding columns [k, kp) and puts k - 1 in the upper lane half"""
    return 27 if kp == 32 else 61


# ------------------------------------------------------------------------------------------------------------------------------
# residual_kernel / product_kernel: launch paths
# ------------------------------------------------------------------------------------------------------------------------------
# name -> (m, n, what the plan must say about (groups, per, tiles))
RES_SHAPES = {
    "ragged": (130, 70, lambda g, per, tiles: per == 1 and g == tiles == 3),                 # one tile per group, ragged m and n
    "one_tile": (100, 27, lambda g, per, tiles: (g, per, tiles) == (1, 1, 1)),                # exactly one column tile
    "few_rows": (20, 70, lambda g, per, tiles: per == 1 and g == 3),                          # m < 32: three waves of the block idle
    "long_row": (128, 65606, lambda g, per, tiles: per >= 3 and tiles % per != 0 and g > 1),  # one row block, short last group
    "tall": (8192, 34 * 32 - 5, lambda g, per, tiles: per >= 3 and tiles % per != 0 and g > 1),
}


def res_plan(L, name):
    m, n, ok = RES_SHAPES[name]
    g, per = plan(L.lib.bmf_residual_plan, m, n)
    tiles = -(-n // 32)
    assert ok(g, per, tiles), (name, g, per, tiles)
    assert (g - 1) * per < tiles <= g * per
    return m, n, up(m, 128), up(n, 64)


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", list(RES_SHAPES))
def test_residual_sums_exact_on_every_path(L, name, kp):
    """bmf_residual_sums (residual_kernel<KP, false, false>) == the exact sums, with clean padding and with everything the contract
    says is ignored poisoned: X bits of rows >= m and columns >= n set, factor rows >= m / >= n large."""
    m, n, m_pad, n_pad = res_plan(L, name)
    k = kk(kp)
    c = R.exact_case(m, n, k)
    ldx = n_pad // 32 + 1
    for poison in (False, True):
        Xd = dev(R.x_words(m, n, m_pad, ldx, poison=poison))
        Ud = dev(R.pad_factor(c["U"], m_pad, kp, fill=BIG if poison else 0.0))
        Vd = dev(R.pad_factor(c["V"], n_pad, kp, fill=BIG if poison else 0.0))
        sums = zeros(4)
        L.check(L.lib.bmf_residual_sums(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), None, stream()))
        got = sums.cpu().numpy()
        assert (got[0], got[1]) == (c["s_abs"], c["s_sq"]), (poison, got, c["s_abs"], c["s_sq"])
        assert got[2] == 0 and got[3] == 0
    # two calls without zeroing add up; a raised stop flag leaves the sums alone
    L.check(L.lib.bmf_residual_sums(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), None, stream()))
    assert (sums[0].item(), sums[1].item()) == (2 * c["s_abs"], 2 * c["s_sq"])
    for flag, mult in ((1, 2), (-5, 2), (0, 3)):
        stop = dev(np.array([flag], np.int32))
        L.check(L.lib.bmf_residual_sums(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), L.ptr(stop), stream()))
        assert (sums[0].item(), sums[1].item()) == (mult * c["s_abs"], mult * c["s_sq"]), flag


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", list(RES_SHAPES))
def test_residual_sums_f32_exact_on_every_path(L, name, kp):
    """bmf_residual_sums_f32 (residual_kernel<KP, false, true>): a real-valued X, zero padded as its contract says; factor rows of the
    padding poisoned."""
    m, n, m_pad, n_pad = res_plan(L, name)
    k = kk(kp)
    c = R.exact_real_case(m, n, k)
    ldx = n_pad + 32
    X = np.zeros((m_pad, ldx), np.float32)
    X[:m, :n] = R.real_x(m, n)
    Xd = dev(X)
    for poison in (False, True):
        Ud = dev(R.pad_factor(c["U"], m_pad, kp, fill=BIG if poison else 0.0))
        Vd = dev(R.pad_factor(c["V"], n_pad, kp, fill=BIG if poison else 0.0))
        sums = zeros(4)
        L.check(L.lib.bmf_residual_sums_f32(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), stream()))
        got = sums.cpu().numpy()
        assert (got[0], got[1]) == (c["s_abs"], c["s_sq"]), (poison, got, c["s_abs"], c["s_sq"])
    L.check(L.lib.bmf_residual_sums_f32(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), stream()))
    assert (sums[0].item(), sums[1].item()) == (2 * c["s_abs"], 2 * c["s_sq"])


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", list(RES_SHAPES))
def test_real_product_element_by_element(L, name, kp):
    """bmf_real_product (product_kernel<KP>): every element == the exact product, the slack of ldo > n and the rows >= m untouched."""
    m, n, m_pad, n_pad = res_plan(L, name)
    k = kk(kp)
    c = R.exact_case(m, n, k)
    ldo = n + 3
    Ud, Vd = dev(R.pad_factor(c["U"], m_pad, kp, fill=BIG)), dev(R.pad_factor(c["V"], n_pad, kp, fill=BIG))
    rows = min(m_pad, m + 5)
    out = torch.full((rows, ldo), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(L.lib.bmf_real_product(L.ptr(Ud), m_pad, m, L.ptr(Vd), n_pad, n, kp, L.ptr(out), ldo, stream()))
    got = out.cpu().numpy()
    assert np.array_equal(got[:m, :n].astype(np.float64), c["U"] @ c["V"].T)
    assert (got[:m, n:] == SENTINEL).all() and (got[m:] == SENTINEL).all()


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", ["ragged", "long_row"])
def test_residual_random_real_factors(L, name, kp):
    """Random real factors: rtol 1e-6, the bound of test_residual_sums / test_tiled_real_matrix_kernels (exact-fp32 passes), against
    fp64 from the same fp32-rounded inputs; product elements at the 2e-6 of test_real_product."""
    m, n, m_pad, n_pad = res_plan(L, name)
    k = kk(kp)
    rng = np.random.default_rng([31, m, n, kp])
    U, V = R.random_factor(rng, m, k), R.random_factor(rng, n, k)
    Ud, Vd = dev(R.pad_factor(U, m_pad, kp, fill=BIG)), dev(R.pad_factor(V, n_pad, kp, fill=BIG))
    ldx = n_pad // 32
    Xd = dev(R.x_words(m, n, m_pad, ldx, poison=True))
    sums = zeros(4)
    L.check(L.lib.bmf_residual_sums(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), None, stream()))
    want = R.dense_sums(R.x_block, m, n, U, V)
    np.testing.assert_allclose(sums.cpu().numpy()[:2], want, rtol=1e-6)
    X = np.zeros((m_pad, n_pad), np.float32)
    X[:m, :n] = R.real_x(m, n) * np.float32(0.37)
    sums.zero_()
    L.check(L.lib.bmf_residual_sums_f32(L.ptr(dev(X)), m_pad, n_pad, m, n, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(sums), stream()))
    want = R.dense_sums(lambda i, j: X[np.ix_(i, j)], m, n, U, V)
    np.testing.assert_allclose(sums.cpu().numpy()[:2], want, rtol=1e-6)
    out = torch.full((m, n), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(L.lib.bmf_real_product(L.ptr(Ud), m_pad, m, L.ptr(Vd), n_pad, n, kp, L.ptr(out), n, stream()))
    np.testing.assert_allclose(out.cpu().numpy(), U.astype(np.float64) @ V.astype(np.float64).T, rtol=2e-6)


# ------------------------------------------------------------------------------------------------------------------------------
# the thresholding objective, fp32 (the only route to residual_kernel<KP, GRAD = true>) and its transform
# ------------------------------------------------------------------------------------------------------------------------------
def nan_padded(F, rows_pad, kp, dtype):
    """F inside rows_pad x kp with NaN in every padding row and in the padding columns [k, kp) of every row"""
    out = np.full((rows_pad, kp), np.nan, dtype)
    out[:F.shape[0], :F.shape[1]] = F
    return out


def zero_padded(F, rows_pad, kp):
    return R.pad_factor(F, rows_pad, kp, dtype=np.float64)


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", ["ragged", "few_rows", "one_tile", "long_row", "tall"])
def test_thresh_eval_fp32_exact_on_every_path(L, name, kp):
    """bmf_thresh_eval on saturated inputs (transformed factors in {0, 1/2, 1}, derivative factors in {0, 1}: every term exact):
    out[0..1] == exact; dF to 2e-5 of scale, the bound of test_thresh_eval_against_golden; the transformed factors left in `work`
    element by element; NaN in every input the contract says is ignored."""
    m, n, m_pad, n_pad = res_plan(L, name)
    k = kk(kp)
    c = R.sat_case(m, n, k)
    ldx = n_pad // 32
    work = torch.full(((2 * m_pad + 2 * n_pad) * kp,), SENTINEL, dtype=torch.float32, device="cuda")
    outs = {}
    for poison in (False, True):
        Xd = dev(R.x_words(m, n, m_pad, ldx, poison=poison))
        pad = nan_padded if poison else (lambda F, r, q, dt: R.pad_factor(F, r, q, dtype=dt))
        Ud, Vd = dev(pad(c["U"], m_pad, kp, np.float32)), dev(pad(c["V"], n_pad, kp, np.float32))
        for grad in (1, 0):
            out = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(L.lib.bmf_thresh_eval(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), n_pad, L.ptr(Vd), k, kp, R.SAT_X, R.SAT_X, R.SAT_LAM,
                                          grad, L.ptr(work), L.ptr(out), stream()))
            o = outs[poison, grad] = out.cpu().numpy()
            assert (o[0], o[1]) == (c["out"][0], c["out"][1]), (poison, grad, o, c["out"])
            if grad:
                scale = np.abs(c["out"][2:]).max() + 1.0
                assert abs(o[2] - c["out"][2]) < 2e-5 * scale and abs(o[3] - c["out"][3]) < 2e-5 * scale, (o, c["out"])
                w = work.cpu().numpy().astype(np.float64)
                a, b = m_pad * kp, n_pad * kp
                for got, want, rp in ((w[:a], c["Us"], m_pad), (w[a:2 * a], c["dUs"], m_pad), (w[2 * a:2 * a + b], c["Vs"], n_pad),
                                      (w[2 * a + b:], c["dVs"], n_pad)):
                    assert np.array_equal(got.reshape(rp, kp), zero_padded(want, rp, kp))
            else:
                assert o[2] == 0 and o[3] == 0


@pytest.mark.parametrize("kp", [32, 64])
def test_thresh_eval_fp32_random_factors(L, kp):
    """Random factors against the longdouble reference on the fp32-rounded factors: F at the 2e-6 and dF at the 2e-5 of scale of
    test_thresh_eval_against_golden."""
    m, n, m_pad, n_pad = res_plan(L, "ragged")
    k = kk(kp)
    rng = np.random.default_rng([32, kp])
    U, V = rng.random((m, k)).astype(np.float32), rng.random((n, k)).astype(np.float32)
    X = R.x_block(np.arange(m), np.arange(n))
    ldx = n_pad // 32
    Xd, Ud, Vd = dev(R.x_words(m, n, m_pad, ldx, poison=True)), dev(nan_padded(U, m_pad, kp, np.float32)), dev(nan_padded(V, n_pad, kp, np.float32))
    work = zeros((2 * m_pad + 2 * n_pad) * kp, torch.float32)
    out = zeros(4)
    for lam, u, v in ((10.0, 0.4, 0.55), (100.0, 0.5, 0.3)):
        L.check(L.lib.bmf_thresh_eval(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), n_pad, L.ptr(Vd), k, kp, u, v, lam, 1, L.ptr(work), L.ptr(out), stream()))
        want = R.thresh_ref(X, U, V, u, v, lam)[0].astype(np.float64)
        o = out.cpu().numpy()
        assert o[1] == pytest.approx(want[1], rel=2e-6) and o[0] == pytest.approx(want[0], rel=2e-6)
        scale = np.abs(want[2:]).max() + 1.0
        assert abs(o[2] - want[2]) < 2e-5 * scale and abs(o[3] - want[3]) < 2e-5 * scale


def transform_tolerance(z, ulp):
    """Element bound of the transforms, from the formats alone: z = lam (F - x) carries two roundings, |dz| <= 2 |z| ulp, which exp turns
    into a relative error of its value; exp itself, the division and the products of s and d add a few roundings more (8 allowed); the
    result is then rounded to the output format once (fp32: ulp = 2^-24 dominates)."""
    return (2 * np.abs(z) + 8) * 2.0 ** -53 + ulp


@pytest.mark.parametrize("kp", [32, 64])
def test_thresh_transform_fp32_element_by_element(L, kp):
    """bmf_thresh_transform: S and D (NULL and non-NULL) at every edge of the sigmoid; rows >= rows and columns >= k are written as 0
    without reading the input (NaN there)."""
    rows, rows_pad, k, lam = 70, 128, kk(kp), 10.0
    rng = np.random.default_rng([33, kp])
    for x in (0.0, 0.375):
        F = rng.random((rows, k)).astype(np.float32)
        edge = R.transform_inputs(x, lam, np.float32)
        F[0, :len(edge)] = edge
        F[rows - 1, k - len(edge):] = edge
        Fd = dev(nan_padded(F, rows_pad, kp, np.float32))
        z = (F.astype(np.longdouble) - np.longdouble(x)) * lam
        s, d = R.sigmoid_pair(z, lam)
        tol = transform_tolerance(z.astype(np.float64), 2.0 ** -24)
        for with_d in (True, False):
            S = torch.full((rows_pad, kp), SENTINEL, dtype=torch.float32, device="cuda")
            D = torch.full((rows_pad, kp), SENTINEL, dtype=torch.float32, device="cuda")
            L.check(L.lib.bmf_thresh_transform(L.ptr(Fd), rows_pad, rows, k, kp, x, lam, L.ptr(S), L.ptr(D) if with_d else None, stream()))
            gs, gd = S.cpu().numpy().astype(np.float64), D.cpu().numpy().astype(np.float64)
            assert not gs[rows:].any() and not gs[:, k:].any()
            assert (np.abs(gs[:rows, :k] - s) <= tol * s + 2.0 ** -149).all()
            if with_d:
                assert not gd[rows:].any() and not gd[:, k:].any()
                assert (np.abs(gd[:rows, :k] - d) <= tol * d + 2.0 ** -149).all()
            else:
                assert (gd == SENTINEL).all()
        assert gs[0, 0] == 0.5


# ------------------------------------------------------------------------------------------------------------------------------
# bmf_thresh_eval64
# ------------------------------------------------------------------------------------------------------------------------------
def eval64(L, Xd, m_pad, ldx, m, n, Ud, n_pad, Vd, k, kp, u, v, lam, grad, work):
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_thresh_eval64(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), n_pad, L.ptr(Vd), k, kp, u, v, lam, grad, L.ptr(work), L.ptr(out), stream()))
    return out.cpu().numpy()


def eval64_exact(L, m, n, m_pad, n_pad, k, kp):
    """saturated inputs: out[0..1] ==; dF at 1e-9 of scale (test_thresh_eval64_against_golden); want_grad 0 and 1 and a repeated call
    and the poisoned call bit-identical; the work buffers element by element"""
    c = R.sat_case(m, n, k)
    ldx = n_pad // 32
    nwork = int(L.lib.bmf_thresh_eval64_work(m_pad, n_pad, kp))
    assert nwork == (2 * m_pad + 2 * n_pad) * kp + (m_pad // 64) * (n_pad // 64) * 4
    outs = {}
    for poison in (False, True):
        Xd = dev(R.x_words(m, n, m_pad, ldx, poison=poison))
        pad = nan_padded if poison else (lambda F, r, q, dt: R.pad_factor(F, r, q, dtype=dt))
        Ud, Vd = dev(pad(c["U"], m_pad, kp, np.float64)), dev(pad(c["V"], n_pad, kp, np.float64))
        work = torch.full((nwork,), SENTINEL, dtype=torch.float64, device="cuda")
        o0 = eval64(L, Xd, m_pad, ldx, m, n, Ud, n_pad, Vd, k, kp, R.SAT_X, R.SAT_X, R.SAT_LAM, 0, work)
        a, b = m_pad * kp, n_pad * kp
        w = work.cpu().numpy()
        assert np.array_equal(w[:a].reshape(m_pad, kp), zero_padded(c["Us"], m_pad, kp))
        assert np.array_equal(w[2 * a:2 * a + b].reshape(n_pad, kp), zero_padded(c["Vs"], n_pad, kp))
        assert (w[a:2 * a] == SENTINEL).all() and (w[2 * a + b:2 * a + 2 * b] == SENTINEL).all()    # want_grad = 0 never writes dUs / dVs
        o1 = eval64(L, Xd, m_pad, ldx, m, n, Ud, n_pad, Vd, k, kp, R.SAT_X, R.SAT_X, R.SAT_LAM, 1, work)
        o2 = eval64(L, Xd, m_pad, ldx, m, n, Ud, n_pad, Vd, k, kp, R.SAT_X, R.SAT_X, R.SAT_LAM, 1, work)
        w = work.cpu().numpy()
        for got, want, rp in ((w[:a], c["Us"], m_pad), (w[a:2 * a], c["dUs"], m_pad), (w[2 * a:2 * a + b], c["Vs"], n_pad),
                              (w[2 * a + b:2 * a + 2 * b], c["dVs"], n_pad)):
            assert np.array_equal(got.reshape(rp, kp), zero_padded(want, rp, kp))
        assert (o1[0], o1[1]) == (c["out"][0], c["out"][1]), (poison, o1, c["out"])
        assert o0[0].tobytes() == o1[0].tobytes() and o0[1].tobytes() == o1[1].tobytes() and o1.tobytes() == o2.tobytes()
        np.testing.assert_allclose(o1[2:], c["out"][2:], rtol=1e-9, atol=1e-9 * np.abs(c["out"][2:]).max())
        outs[poison] = o1
    assert outs[False].tobytes() == outs[True].tobytes()


@pytest.mark.parametrize("k,kp", [(1, 32), (15, 32), (16, 32), (17, 32), (32, 32), (16, 64), (17, 64), (33, 64), (64, 64)])
def test_thresh_eval64_every_k(L, k, kp):
    """dense64_kernel's chunk loop (k0 < k, 16 at a time) at k below, at and above every multiple of 16, both kp; 3 x 5 tiles (odd
    multiples of 64) with m and n ragged inside the last tile"""
    eval64_exact(L, 150, 300, 192, 320, k, kp)


@pytest.mark.parametrize("m,n,k,kp,min_blocks", [(4160 - 20, 320 - 9, 33, 64, 257), (4160 - 20, 1088 - 9, 17, 32, 1025)])
def test_thresh_eval64_many_blocks(L, m, n, k, kp, min_blocks):
    """sum_partials_kernel adding 2 (65 x 5 tiles) and 5 (65 x 17 tiles) blocks per thread; at kp = 64 the 4160 rows are more than the
    1024 blocks x 256 threads of transform64_pair_kernel cover in one trip"""
    m_pad, n_pad = up(m, 64), up(n, 64)
    blocks = (m_pad // 64) * (n_pad // 64)
    assert blocks >= min_blocks and -(-blocks // 256) == (2 if min_blocks == 257 else 5)
    if kp == 64:
        assert m_pad * kp > 1024 * 256
    eval64_exact(L, m, n, m_pad, n_pad, k, kp)


@pytest.mark.parametrize("k,kp", [(15, 32), (33, 64)])
def test_thresh_eval64_random_factors_and_transform_elements(L, k, kp):
    """Random fp64 factors against the longdouble reference: sums at the 1e-11 and dF at the 1e-9 of test_thresh_eval64_against_golden;
    Us, dUs, Vs, dVs read back from `work` element by element, with the first row of each factor at every edge of the sigmoid."""
    m, n, m_pad, n_pad, lam = 150, 300, 192, 320, 10.0
    rng = np.random.default_rng([34, k])
    X = R.x_block(np.arange(m), np.arange(n))
    ldx = n_pad // 32
    Xd = dev(R.x_words(m, n, m_pad, ldx, poison=True))
    work = zeros(int(L.lib.bmf_thresh_eval64_work(m_pad, n_pad, kp)))
    for x in (0.0, 0.375):
        U, V = rng.random((m, k)) - 0.5 + x, rng.random((n, k)) - 0.5 + x
        edge = R.transform_inputs(x, lam, np.float64)
        U[0, :min(k, len(edge))] = edge[:k]
        V[n - 1, :min(k, len(edge))] = edge[::-1][:k]
        Ud, Vd = dev(nan_padded(U, m_pad, kp, np.float64)), dev(nan_padded(V, n_pad, kp, np.float64))
        o = eval64(L, Xd, m_pad, ldx, m, n, Ud, n_pad, Vd, k, kp, x, x, lam, 1, work)
        want, (Us, dUs, Vs, dVs) = R.thresh_ref(X, U, V, x, x, lam)
        np.testing.assert_allclose(o[:2], want[:2].astype(np.float64), rtol=1e-11)
        np.testing.assert_allclose(o[2:], want[2:].astype(np.float64), rtol=1e-9, atol=1e-9 * float(np.abs(want[2:]).max()))
        w = work.cpu().numpy()
        a, b = m_pad * kp, n_pad * kp
        for got, ref, F, rows, rp in ((w[:a], Us, U, m, m_pad), (w[a:2 * a], dUs, U, m, m_pad), (w[2 * a:2 * a + b], Vs, V, n, n_pad),
                                      (w[2 * a + b:2 * a + 2 * b], dVs, V, n, n_pad)):
            got = got.reshape(rp, kp)
            assert not got[rows:].any() and not got[:, k:].any()
            tol = transform_tolerance((F - x) * lam, 2.0 ** -53)
            assert (np.abs(got[:rows, :k] - ref) <= tol * ref + 2.0 ** -1074).all()


def test_thresh_eval64_work_refuses_bad_arguments(L):
    f = L.lib.bmf_thresh_eval64_work
    assert f(192, 320, 32) == (2 * 192 + 2 * 320) * 32 + 3 * 5 * 4 and f(64, 64, 64) == 4 * 64 * 64 + 4
    for bad in ((0, 64, 32), (64, 0, 32), (-64, 64, 32), (100, 64, 32), (64, 100, 32), (64, 64, 48), (64, 64, 0), (64, 64, 128)):
        assert f(*bad) == -1, bad


# ------------------------------------------------------------------------------------------------------------------------------
# single-cell probes
# ------------------------------------------------------------------------------------------------------------------------------
PA, PB = 0.75, 0.625       # dyadic: the product 0.46875 and its square are exact in every format


def word_bit(j):
    """(word, int32 value) of bit j of a row of packed words"""
    return j // 32, (1 << (j % 32)) - (1 << 32 if j % 32 == 31 else 0)


def probe_lists(m, m_pad, n, n_pad, kp, k):
    return ([0, 31, 32, 127, 128, m - 1, m, m_pad - 1], [0, 3, 4, 7, 8, 31, 32, 63, 64, n - 1, n, n_pad - 1], [0, kp // 2 - 1, kp // 2, k - 1])


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("real_x", [False, True])
def test_single_cell_probes_residual(L, kp, real_x):
    """bmf_residual_sums / bmf_residual_sums_f32 with ONE non-zero cell: X[i][j] = 1 over zero factors gives (1, 1); U[i][l] = a,
    V[j][l] = b over a zero X gives (ab, a^2 b^2); cells outside m x n give 0."""
    m, n, m_pad, n_pad, k = 130, 70, 256, 128, kk(kp)
    I, J, Ls = probe_lists(m, m_pad, n, n_pad, kp, k)
    ldx = n_pad if real_x else n_pad // 32
    Xd = torch.zeros((m_pad, ldx), dtype=torch.float32 if real_x else torch.int32, device="cuda")
    Ud, Vd = zeros((m_pad, kp), torch.float32), zeros((n_pad, kp), torch.float32)
    probes = [(i, j, None) for i in I for j in J] + [(i, j, l) for i in I for j in J for l in Ls]
    sums = zeros(4 * len(probes))
    want = np.zeros((len(probes), 4))

    def launch(p):
        if real_x:
            L.check(L.lib.bmf_residual_sums_f32(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, at(sums, 4 * p), stream()))
        else:
            L.check(L.lib.bmf_residual_sums(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), L.ptr(Vd), kp, at(sums, 4 * p), None, stream()))

    for p, (i, j, l) in enumerate(probes):
        inside = i < m and j < n
        if l is None:
            w, val = (j, 1.0) if real_x else word_bit(j)
            Xd[i, w] = val
            launch(p)
            Xd[i, w] = 0
            want[p, :2] = (1, 1) if inside else (0, 0)
        else:
            Ud[i, l] = PA
            Vd[j, l] = PB
            launch(p)
            Ud[i, l] = 0
            Vd[j, l] = 0
            want[p, :2] = (PA * PB, (PA * PB) ** 2) if inside else (0, 0)
    got = sums.cpu().numpy().reshape(-1, 4)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(probes[p], got[p].tolist(), want[p].tolist()) for p in bad[:8]]


@pytest.mark.parametrize("kp", [32, 64])
def test_single_cell_probes_thresh_eval64(L, kp):
    """bmf_thresh_eval64 with one non-zero cell, through inputs whose transform is exactly 0, 1/2 or 1 (see objective_ref.sat_factor)"""
    m, n, m_pad, n_pad, k = 130, 70, 256, 128, kk(kp)
    I, J, Ls = probe_lists(m, m_pad, n, n_pad, kp, k)
    ldx = n_pad // 32
    lo, mid, hi = R.SAT_X - 200.0, R.SAT_X, R.SAT_X + 200.0       # s = 0, 1/2 (d = 1), 1
    Xd = torch.zeros((m_pad, ldx), dtype=torch.int32, device="cuda")
    Ud = torch.full((m_pad, kp), lo, dtype=torch.float64, device="cuda")
    Vd = torch.full((n_pad, kp), lo, dtype=torch.float64, device="cuda")
    work = zeros(int(L.lib.bmf_thresh_eval64_work(m_pad, n_pad, kp)))
    probes = [(i, j, None) for i in I for j in J] + [(i, j, l) for i in I for j in J for l in Ls]
    outs = torch.full((4 * len(probes),), SENTINEL, dtype=torch.float64, device="cuda")
    want = np.zeros((len(probes), 4))
    for p, (i, j, l) in enumerate(probes):
        inside = i < m and j < n
        if l is None:
            w, val = word_bit(j)
            Xd[i, w] = val
            want[p] = (1, 1, 0, 0) if inside else (0, 0, 0, 0)
        else:
            half_u = (i + j + l) % 2 == 0                         # which factor sits AT the threshold (s = 1/2, derivative 1)
            Ud[i, l] = mid if half_u else hi
            Vd[j, l] = hi if half_u else mid
            # R = -1/2; dUs Vs^T = 1 (half_u) or 0; Us dVs^T = 0 or 1
            want[p] = (0.5, 0.25, -0.5 if half_u else 0.0, 0.0 if half_u else -0.5) if inside else (0, 0, 0, 0)
        L.check(L.lib.bmf_thresh_eval64(L.ptr(Xd), m_pad, ldx, m, n, L.ptr(Ud), n_pad, L.ptr(Vd), k, kp, R.SAT_X, R.SAT_X, R.SAT_LAM, 1,
                                        L.ptr(work), at(outs, 4 * p), stream()))
        if l is None:
            Xd[i, w] = 0
        else:
            Ud[i, l] = lo
            Vd[j, l] = lo
    got = outs.cpu().numpy().reshape(-1, 4)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(probes[p], got[p].tolist(), want[p].tolist()) for p in bad[:8]]


MAE_VARIANTS = ["three", "one", "auto", "tiled"]


def mae_call(L, variant, XT, ldxt, m_pad, n_pad, Ud, Vd, kp, ws, out):
    a = (L.ptr(XT), ldxt, m_pad, n_pad, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(ws), out)
    if variant == "three":
        return L.lib.bmf_mae_sum_ex(*a, 0, stream())
    if variant == "one":
        return L.lib.bmf_mae_sum_ex(*a, 1, stream())
    if variant == "auto":
        return L.lib.bmf_mae_sum(*a, stream())
    return L.lib.bmf_mae_sum_tiled(*a, stream())


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("variant", MAE_VARIANTS)
def test_single_cell_probes_mae(L, variant, kp):
    """The four MAE entry points with one non-zero cell (no masks: every cell of the padded problem is in range): two row blocks, four
    stages; the tiled variant sets its bit through the tiled layout."""
    m_pad, n_pad, k = 512, 256, kk(kp)
    ldxt = m_pad // 32
    I = [0, 31, 32, 63, 64, 127, 128, 255, 256, m_pad - 1]
    J = [0, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, n_pad - 1]
    Ls = [0, kp // 2 - 1, kp // 2, k - 1]
    XT = torch.zeros(n_pad * ldxt, dtype=torch.int32, device="cuda")
    Ud, Vd = zeros((m_pad, kp), torch.float32), zeros((n_pad, kp), torch.float32)
    ws = zeros(2 * (m_pad + n_pad) * kp, torch.int16)
    probes = [(i, j, None) for i in I for j in J] + [(i, j, l) for i in I for j in J for l in Ls]
    sums = zeros(len(probes))
    want = np.zeros(len(probes))
    for p, (i, j, l) in enumerate(probes):
        if l is None:
            w, val = word_bit(i)
            idx = j * ldxt + w if variant != "tiled" else (((j >> 8) * (ldxt >> 4) + (w >> 4)) * 256 + (j & 255)) * 16 + (w & 15)
            XT[idx] = val
            want[p] = 1
        else:
            Ud[i, l] = PA
            Vd[j, l] = PB
            want[p] = PA * PB
        L.check(mae_call(L, variant, XT, ldxt, m_pad, n_pad, Ud, Vd, kp, ws, at(sums, p)))
        if l is None:
            XT[idx] = 0
        else:
            Ud[i, l] = 0
            Vd[j, l] = 0
    got = sums.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(probes[p], got[p], want[p]) for p in bad[:8]]


# ------------------------------------------------------------------------------------------------------------------------------
# mae_kernel / mae32_kernel: launch paths
# ------------------------------------------------------------------------------------------------------------------------------
def mae_exact(L, m, n, m_pad, n_pad, kp, variants, reps=1):
    """every variant == the exact sum of the m x n problem zero padded to m_pad x n_pad, in each of `reps` launches"""
    c = R.exact_case(m, n, kk(kp))
    ldxt = m_pad // 32
    xt = R.xt_words(m, n, n_pad, ldxt)
    Ud, Vd = dev(R.pad_factor(c["U"], m_pad, kp)), dev(R.pad_factor(c["V"], n_pad, kp))
    ws = zeros(2 * (m_pad + n_pad) * kp, torch.int16)
    got = {}
    for v in variants:
        XT = dev(R.tile_bits(xt) if v == "tiled" else xt)
        out = zeros(2 * reps)
        for r in range(reps):
            L.check(mae_call(L, v, XT, ldxt, m_pad, n_pad, Ud, Vd, kp, ws, at(out, 2 * r)))
        got[v] = out.cpu().numpy().tolist()
    assert got == {v: [c["s_abs"], 0.0] * reps for v in variants}, (got, c["s_abs"])


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("row_blocks", [1, 2, 7, 8, 9, 10])
def test_mae_row_blocks_one_stage_per_group(L, row_blocks, kp):
    """Row-block counts that 8 divides and does not divide: the XCD remap rb = (id & 7) * rb_per_xcd + local % rb_per_xcd must visit
    every row block once and the surplus workgroups must return (a block summed twice or skipped moves the exact sum); one stage per
    group.  The tiled X^T needs m_pad % 512 == 0: even counts only."""
    m_pad, n_pad = 256 * row_blocks, 256
    groups, per = plan(L.lib.bmf_mae_plan, m_pad, n_pad)
    assert (groups, per) == (4, 1)
    mae_exact(L, m_pad - 3, n_pad - 5, m_pad, n_pad, kp, MAE_VARIANTS if row_blocks % 2 == 0 else MAE_VARIANTS[:3])


# name -> (stages per group wanted, a short last range wanted, variants, candidate (m_pad, n_pad): the first that fits the device at hand;
# a 256-CU part takes the first of each, the second is worked out for 304 CUs).  The tiled X^T needs n_pad % 256 == 0, i.e. a stage
# count that 4 divides: 2 or 4 stages per group then never leave a short range, so the tiled variant gets shapes of its own for those.
MAE_STAGE_CASES = {
    "2": (2, True, ["three", "one"], [(16384, 64 * 49), (16384, 64 * 59)]),
    "2_tiled": (2, False, ["tiled"], [(16384, 64 * 52), (16384, 64 * 60)]),
    "3": (3, True, ["three", "one", "tiled"], [(16384, 64 * 100), (16384, 64 * 116)]),
    "4": (4, True, ["three", "one"], [(16384, 64 * 145), (16384, 64 * 173)]),
    "4_tiled": (4, False, ["tiled"], [(16384, 64 * 148), (16384, 64 * 176)]),
}


def mae_stage_shape(L, name):
    stages, short, variants, candidates = MAE_STAGE_CASES[name]
    for m_pad, n_pad in candidates:
        groups, per = plan(L.lib.bmf_mae_plan, m_pad, n_pad)
        total = n_pad // 64
        assert (groups - 1) * per < total <= groups * per
        if (per == stages if stages < 4 else per >= 4) and (total % per != 0 or not short) and groups >= 2 and m_pad // 256 >= 2:
            return m_pad, n_pad, variants
    pytest.fail(f"no candidate shape gives {stages} stages per group on this device: {candidates}")


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", list(MAE_STAGE_CASES))
def test_mae_ring_depths(L, name, kp):
    """The 3-deep LDS ring shorter than itself (2 stages per group), exactly full (3) and in steady state (>= 4), with a shorter last
    range wherever the variant's shape rules allow one, on 64 row blocks."""
    m_pad, n_pad, variants = mae_stage_shape(L, name)
    mae_exact(L, m_pad - 3, n_pad - 5, m_pad, n_pad, kp, variants)


@pytest.mark.parametrize("kp", [32, 64])
def test_mae_single_product_launch_after_launch(L, kp):
    """mae32_kernel carries the X words of the next stage in registers filled by a hand-placed LDS read; the compiler once copied half
    of such a pair ahead of the wait for it, so that a launch now and then (4 in 100 at kp = 32) scored 32 rows of a tile against
    the previous stage's bits -- a sum a few cells off, and only with several stages per range (HISTORY.md).  Twenty-five launches of
    each single-product variant, every one exact."""
    m_pad, n_pad, _ = mae_stage_shape(L, "2")
    mae_exact(L, m_pad - 3, n_pad - 5, m_pad, n_pad, kp, ["one"], reps=25)
    m_pad, n_pad, _ = mae_stage_shape(L, "2_tiled")
    mae_exact(L, m_pad - 3, n_pad - 5, m_pad, n_pad, kp, ["tiled"], reps=25)


@pytest.mark.parametrize("kp", [32, 64])
def test_zero_padding_kernels_do_not_see_the_padding(L, kp):
    """The kernels without masks: one problem padded two ways gives the identical exact sum."""
    for m_pad, n_pad in ((256, 64), (512, 320)):
        mae_exact(L, 250, 60, m_pad, n_pad, kp, ["three", "one", "auto"])
        tiled_resid_exact(L, 250, 60, m_pad, n_pad, kp)
    for m_pad, n_pad in ((512, 256), (1024, 512)):
        mae_exact(L, 250, 60, m_pad, n_pad, kp, ["tiled"])


@pytest.mark.parametrize("kp", [32, 64])
def test_mae_auto_mode_either_side_of_2_24_cells(L, kp):
    """bmf_mae_sum picks the three-product pass below 2^24 padded cells and the single product from there on: it returns what the
    explicit mode returns, to that mode's bound (2e-6 / 2e-5, test_mae_sum_bf16_mfma; fp64 atomics: not bit-reproducible), and
    both are that close to fp64 from the same fp32 factors."""
    k = kk(kp)
    for (m_pad, n_pad), mode, tol in (((4096, 4032), "three", 2e-6), ((4096, 4096), "one", 2e-5)):
        assert (m_pad * n_pad >= 1 << 24) == (mode == "one")
        m, n = m_pad - 3, n_pad - 5
        rng = np.random.default_rng([35, n_pad, kp])
        U, V = R.random_factor(rng, m, k), R.random_factor(rng, n, k)
        want = R.dense_sums(R.x_block, m, n, U, V)[0]
        ldxt = m_pad // 32
        XT, Ud, Vd = dev(R.xt_words(m, n, n_pad, ldxt)), dev(R.pad_factor(U, m_pad, kp)), dev(R.pad_factor(V, n_pad, kp))
        ws = zeros(2 * (m_pad + n_pad) * kp, torch.int16)
        got = {}
        for v in ("auto", "three", "one"):
            out = zeros(1)
            L.check(mae_call(L, v, XT, ldxt, m_pad, n_pad, Ud, Vd, kp, ws, L.ptr(out)))
            got[v] = out.item()
        assert got["auto"] == pytest.approx(got[mode], rel=tol) and got["auto"] == pytest.approx(want, rel=tol), (got, want)
        assert got["three"] == pytest.approx(want, rel=2e-6) and got["one"] == pytest.approx(want, rel=2e-5), (got, want)


def test_mae_argument_checks(L):
    m_pad, n_pad, kp = 512, 256, 32
    ldxt = m_pad // 32
    XT = torch.zeros(n_pad * (ldxt + 16), dtype=torch.int32, device="cuda")      # room for the call with ldxt + 16 below
    Ud, Vd = zeros((m_pad, kp), torch.float32), zeros((n_pad, kp), torch.float32)
    ws, out = zeros(2 * (m_pad + n_pad) * kp, torch.int16), zeros(2)
    lib, s = L.lib, stream()
    good = (L.ptr(XT), ldxt, m_pad, n_pad, L.ptr(Ud), L.ptr(Vd), kp, L.ptr(ws), L.ptr(out))
    assert lib.bmf_mae_sum_tiled(*good, s) == 0 and lib.bmf_mae_sum(*good, s) == 0 and lib.bmf_mae_sum_ex(*good, 0, s) == 0

    def with_(**kw):
        names = ["XT", "ldxt", "m_pad", "n_pad", "U", "V", "kp", "ws", "out"]
        return tuple(kw.get(nm, g) for nm, g in zip(names, good))

    for bad in (dict(m_pad=m_pad + 1), dict(m_pad=m_pad - 256 + 128), dict(n_pad=n_pad + 32), dict(n_pad=0), dict(kp=48), dict(ldxt=ldxt - 4),
                dict(ldxt=ldxt + 2), dict(XT=None), dict(U=None), dict(ws=None), dict(out=None), dict(XT=at(XT, 1))):
        assert lib.bmf_mae_sum(*with_(**bad), s) == -1, bad
        assert lib.bmf_mae_sum_ex(*with_(**bad), 1, s) == -1, bad
        assert lib.bmf_mae_sum_tiled(*with_(**bad), s) == -1, bad
    # the tiled copy: n_pad % 256, ldxt == m_pad / 32, ldxt % 16
    assert lib.bmf_mae_sum_tiled(*with_(n_pad=n_pad - 64), s) == -1 and b"tiled" in lib.bmf_last_error()
    assert lib.bmf_mae_sum_tiled(*with_(ldxt=ldxt + 16), s) == -1 and b"tiled" in lib.bmf_last_error()
    assert lib.bmf_mae_sum_tiled(*with_(m_pad=256, ldxt=8), s) == -1 and b"tiled" in lib.bmf_last_error()
    assert lib.bmf_mae_sum_ex(*with_(n_pad=n_pad - 64), 1, s) == 0 and lib.bmf_mae_sum_ex(*with_(ldxt=ldxt + 16), 1, s) == 0
    a, b = C.c_int(), C.c_int()
    assert lib.bmf_mae_plan(m_pad + 1, n_pad, C.byref(a), C.byref(b)) == -1 and lib.bmf_mae_plan(m_pad, n_pad, None, C.byref(b)) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# resid_f32_ring_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def tiled_resid_exact(L, m, n, m_pad, n_pad, kp):
    """bmf_tile_f32 + bmf_frag_rows_f32 + bmf_residual_sums_f32_tiled == the exact sums == bmf_residual_sums_f32 on the row-major copy"""
    c = R.exact_real_case(m, n, kk(kp))
    X = np.zeros((m_pad, n_pad), np.float32)
    X[:m, :n] = R.real_x(m, n)
    Xd, Ud, Vd = dev(X), dev(R.pad_factor(c["U"], m_pad, kp)), dev(R.pad_factor(c["V"], n_pad, kp))
    tiled, frag = zeros(m_pad * n_pad, torch.float32), zeros(n_pad * kp, torch.float32)
    L.check(L.lib.bmf_tile_f32(L.ptr(Xd), m_pad, n_pad, n_pad, L.ptr(tiled), stream()))
    L.check(L.lib.bmf_frag_rows_f32(L.ptr(Vd), n_pad, kp, L.ptr(frag), stream()))
    s1, s2 = zeros(4), zeros(4)
    L.check(L.lib.bmf_residual_sums_f32_tiled(L.ptr(tiled), m_pad, n_pad, L.ptr(Ud), L.ptr(frag), kp, L.ptr(s1), stream()))
    m128 = up(m_pad, 128)      # the row-major kernel wants m_pad % 128 == 0 and factor rows for whole 128-row blocks
    Xr, Ur = zeros((m128, n_pad), torch.float32), zeros((m128, kp), torch.float32)
    Xr[:m_pad] = Xd
    Ur[:m_pad] = Ud
    L.check(L.lib.bmf_residual_sums_f32(L.ptr(Xr), m128, n_pad, m, n, L.ptr(Ur), L.ptr(Vd), kp, L.ptr(s2), stream()))
    g1, g2 = s1.cpu().numpy().tolist(), s2.cpu().numpy().tolist()
    assert g1 == g2 == [c["s_abs"], c["s_sq"], 0.0, 0.0], (g1, g2, c["s_abs"], c["s_sq"])
    L.check(L.lib.bmf_residual_sums_f32_tiled(L.ptr(tiled), m_pad, n_pad, L.ptr(Ud), L.ptr(frag), kp, L.ptr(s1), stream()))
    assert s1.cpu().numpy().tolist() == [2 * c["s_abs"], 2 * c["s_sq"], 0.0, 0.0]       # added to what the buffer holds


@pytest.mark.parametrize("row_tiles", [1, 3])
@pytest.mark.parametrize("stages", [1, 2, 3, 4, 5, 9, 17, 23])
def test_tiled_residual_ring_depths(L, stages, row_tiles):
    """The 4-deep ring of resid_f32_ring_kernel with fewer stages than slots, exactly as many, more, and two splits with a shorter last
    one (17 = 9 + 8, 23 = 12 + 11 stages)."""
    m_pad, n_pad = 64 * row_tiles, 64 * stages
    splits, sps = plan(L.lib.bmf_residual_tiled_plan, m_pad, n_pad)
    if stages >= 17:
        assert splits == 2 and stages % sps != 0 and sps < stages <= 2 * sps
    else:
        assert (splits, sps) == (1, stages)
    for kp in (32, 64):
        tiled_resid_exact(L, m_pad - 7, n_pad - 5, m_pad, n_pad, kp)


@pytest.mark.parametrize("kp", [32, 64])
def test_tiled_residual_random_real_factors(L, kp):
    """rtol 1e-6: the bound of test_tiled_real_matrix_kernels, on the two-split shape with a short last split"""
    m, n, m_pad, n_pad, k = 185, 64 * 23 - 5, 192, 64 * 23, kk(kp)
    assert plan(L.lib.bmf_residual_tiled_plan, m_pad, n_pad) == (2, 12)
    rng = np.random.default_rng([36, kp])
    U, V = R.random_factor(rng, m, k), R.random_factor(rng, n, k)
    X = np.zeros((m_pad, n_pad), np.float32)
    X[:m, :n] = rng.random((m, n))
    Xd, Ud, Vd = dev(X), dev(R.pad_factor(U, m_pad, kp)), dev(R.pad_factor(V, n_pad, kp))
    tiled, frag, s1 = zeros(m_pad * n_pad, torch.float32), zeros(n_pad * kp, torch.float32), zeros(4)
    L.check(L.lib.bmf_tile_f32(L.ptr(Xd), m_pad, n_pad, n_pad, L.ptr(tiled), stream()))
    L.check(L.lib.bmf_frag_rows_f32(L.ptr(Vd), n_pad, kp, L.ptr(frag), stream()))
    L.check(L.lib.bmf_residual_sums_f32_tiled(L.ptr(tiled), m_pad, n_pad, L.ptr(Ud), L.ptr(frag), kp, L.ptr(s1), stream()))
    want = R.dense_sums(lambda i, j: X[np.ix_(i, j)], m, n, U, V)
    np.testing.assert_allclose(s1.cpu().numpy()[:2], want, rtol=1e-6)


@pytest.mark.parametrize("kp", [32, 64])
def test_mae_random_real_factors_multi_stage(L, kp):
    """Random real factors at a shape with several stages per group: 2e-6 for the three-product pass, 2e-5 for the single product (plain
    and tiled), the bounds of test_mae_sum_bf16_mfma."""
    m_pad, n_pad, _ = mae_stage_shape(L, "2_tiled")
    m, n, k = m_pad - 3, n_pad - 5, kk(kp)
    rng = np.random.default_rng([37, kp])
    U, V = R.random_factor(rng, m, k), R.random_factor(rng, n, k)
    want = R.dense_sums(R.x_block, m, n, U, V)[0]
    ldxt = m_pad // 32
    xt = R.xt_words(m, n, n_pad, ldxt)
    Ud, Vd = dev(R.pad_factor(U, m_pad, kp)), dev(R.pad_factor(V, n_pad, kp))
    ws = zeros(2 * (m_pad + n_pad) * kp, torch.int16)
    for v, tol in (("three", 2e-6), ("one", 2e-5), ("tiled", 2e-5)):
        out = zeros(1)
        L.check(mae_call(L, v, dev(R.tile_bits(xt) if v == "tiled" else xt), ldxt, m_pad, n_pad, Ud, Vd, kp, ws, L.ptr(out)))
        assert out.item() == pytest.approx(want, rel=tol), (v, out.item() / want - 1)
