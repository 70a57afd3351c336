"""The kernels only the rank 64 < k <= 128 path has (csrc/wide.hip, bmf_resid_sums_wide in csrc/mae.hip, bmf_masked_pass_wide /
bmf_masked_counts_wide in csrc/masked.hip), one call each, against NumPy in fp64 on the fp32-rounded inputs -- at ragged and tiny
shapes, with outputs and scratch filled with NaN first so that an element a kernel leaves unwritten fails.  The whole-trajectory tests
(tests/test_wide_gpu.py) can hide one wrong term under the factor gate for a few iterations; these cannot."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402

BK = 64
F16_NAN = 0x7E00   # a quiet fp16 NaN, for the uint16 workspace


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    return _lib


def stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f32(a):
    """a as the kernels see it: rounded to fp32, back in fp64 for the reference."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def nan_f32(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def pack_rows(B, rows_pad, words):
    """Boolean rows x cols -> int32 [rows_pad][words], bit c % 32 of word c / 32 (the BitMatrix layout)."""
    out = np.zeros((rows_pad, words * 32), np.uint8)
    out[: B.shape[0], : B.shape[1]] = B
    return np.packbits(out, axis=1, bitorder="little").view(np.int32)


def factor_bits(Fb, rows_pad):
    """Boolean factor (rows x k, 64 < k <= 128) -> per block b: rowbits int64[rows_pad], colbits int32[64][rows_pad / 32]."""
    rows, k = Fb.shape
    out = []
    for b in range(2):
        blk = np.zeros((rows_pad, BK), np.uint8)
        blk[:rows, : min(BK, k - BK * b)] = Fb[:, BK * b: BK * b + BK]
        rowbits = np.packbits(blk, axis=1, bitorder="little").view(np.uint64)[:, 0].view(np.int64)
        colbits = np.packbits(np.ascontiguousarray(blk.T), axis=1, bitorder="little").view(np.int32)
        out.append((dev(rowbits.copy()), dev(colbits)))
    return out


def two_blocks(F, rows_pad):
    """F (rows x k) -> two zero-padded rows_pad x 64 fp32 device blocks."""
    out = []
    for b in range(2):
        t = np.zeros((rows_pad, BK), np.float32)
        part = F[:, BK * b: BK * b + BK]
        t[: F.shape[0], : part.shape[1]] = part
        out.append(dev(t))
    return out


# ---- bmf_fg_f32: out (+)= F G ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_pad", [128, 384, 1664, 20352, 20480])
@pytest.mark.parametrize("ldg", [64, 128])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_fg_f32(L, rows_pad, ldg, accumulate):
    rs = np.random.RandomState(rows_pad + ldg + accumulate)
    F = (rs.standard_normal((rows_pad, BK)) * 10.0 ** rs.uniform(-3, 0, (rows_pad, 1))).astype(np.float32)
    G = rs.standard_normal((BK, ldg)).astype(np.float32)
    G[:, BK:] = np.nan   # columns past the block are never read
    out0 = rs.standard_normal((rows_pad, BK)).astype(np.float32)
    out = dev(out0) if accumulate else nan_f32((rows_pad, BK))
    Fd_, Gd_ = dev(F), dev(G)   # (kept alive until the kernel has run)
    L.check(L.lib.bmf_fg_f32(L.ptr(Fd_), rows_pad, L.ptr(Gd_), ldg, L.ptr(out), accumulate, stream()), "bmf_fg_f32")
    got = out.cpu().numpy().astype(np.float64)
    Fd, Gd = f32(F), f32(G[:, :BK])
    want = Fd @ Gd + (f32(out0) if accumulate else 0.0)
    scale = np.abs(Fd) @ np.abs(Gd) + (np.abs(f32(out0)) if accumulate else 0.0)
    assert np.isfinite(got).all()
    err = np.abs(got - want) / np.maximum(scale, 1e-30)
    assert err.max() < 4e-6, (rows_pad, ldg, accumulate, err.max())   # 64 fp32 additions: at most 64 x 2^-24 of the scale


def test_fg_f32_refuses_bad_shapes(L):
    F, G, out = torch.zeros((256, BK), device="cuda"), torch.zeros((BK, BK), device="cuda"), torch.zeros((256, BK), device="cuda")
    assert L.lib.bmf_fg_f32(L.ptr(F), 200, L.ptr(G), BK, L.ptr(out), 0, stream()) == -1
    assert L.lib.bmf_fg_f32(L.ptr(F), 256, L.ptr(G), 32, L.ptr(out), 0, stream()) == -1
    assert L.lib.bmf_fg_f32(L.ptr(F), 256, L.ptr(G), BK, L.ptr(out), 0, stream()) == 0


# ---- bmf_gram_cross + bmf_reduce_slabs: A^T B ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_pad", [2, 130, 512, 20096])
@pytest.mark.parametrize("blocks", [1, 3, 7, 256, 1024])
@pytest.mark.parametrize("same", [False, True])
def test_gram_cross(L, rows_pad, blocks, same):
    rs = np.random.RandomState(rows_pad * 7 + blocks + same)
    A = (np.abs(rs.standard_normal((rows_pad, BK))) * 10.0 ** rs.uniform(-3, 0, (1, BK))).astype(np.float32)
    B = A if same else rs.standard_normal((rows_pad, BK)).astype(np.float32)
    Ad = dev(A)
    Bd = Ad if same else dev(B)
    slabs = nan_f32((blocks, BK, BK))
    out32 = nan_f32((BK, BK))
    out64 = torch.full((BK, BK), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_gram_cross(L.ptr(Ad), L.ptr(Bd), rows_pad, L.ptr(slabs), blocks, stream()), "bmf_gram_cross")
    L.check(L.lib.bmf_reduce_slabs(L.ptr(slabs), BK * BK, blocks, BK * BK, L.ptr(out32), L.ptr(out64), stream()), "bmf_reduce_slabs")
    S = slabs.cpu().numpy()
    assert np.isfinite(S).all()
    # every slab is written; a block whose waves all start past the last row pair comes back zero
    pairs, nwaves = rows_pad // 2, 4 * blocks
    per = -(-pairs // nwaves)
    idle = [b for b in range(blocks) if 4 * b * per >= pairs]
    if idle:
        assert not S[idle].any(), (rows_pad, blocks, idle[:4])
    got = out64.cpu().numpy()
    Ad64, Bd64 = f32(A), f32(B)
    want = Ad64.T @ Bd64
    scale = np.abs(Ad64).T @ np.abs(Bd64)
    err = np.abs(got - want) / np.maximum(scale, 1e-30)
    assert err.max() < 2e-5, (rows_pad, blocks, same, err.max())
    np.testing.assert_allclose(out32.cpu().numpy(), got, rtol=1e-6, atol=0)
    if same:
        np.testing.assert_allclose(got, got.T, rtol=1e-6, atol=0)


def test_gram_cross_refuses_bad_arguments(L):
    A = torch.zeros((4, BK), device="cuda")
    slabs = torch.zeros((1025, BK, BK), device="cuda")
    assert L.lib.bmf_gram_cross(L.ptr(A), L.ptr(A), 3, L.ptr(slabs), 1, stream()) == -1
    assert L.lib.bmf_gram_cross(L.ptr(A), L.ptr(A), 4, L.ptr(slabs), 0, stream()) == -1
    assert L.lib.bmf_gram_cross(L.ptr(A), L.ptr(A), 4, L.ptr(slabs), 1025, stream()) == -1


# ---- bmf_cover_count_wide: TP / FP of the Boolean product over 128 factors ------------------------------------------------------
def cover_counts(L, X, Ub, Vb, calls=1):
    m, n = X.shape
    m_pad, n_pad = -(-max(m, 1) // 512) * 512, -(-n // 512) * 512
    words = n_pad // 32
    Xd = dev(pack_rows(X, m_pad, words))
    (ra, _), (rb, _) = factor_bits(Ub, m_pad)
    (_, ca), (_, cb) = factor_bits(Vb, n_pad)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(calls):
        L.check(L.lib.bmf_cover_count_wide(L.ptr(Xd), m_pad, words, words, L.ptr(ra), L.ptr(rb), L.ptr(ca), L.ptr(cb), words, L.ptr(counts),
                                           stream()), "bmf_cover_count_wide")
    return tuple(int(c) for c in counts.cpu().numpy())


def want_counts(X, Ub, Vb):
    tp, fp, _, _ = orc.confusion_counts(X.astype(np.float64), orc.boolean_product(Ub.astype(np.float64), Vb.astype(np.float64), 0.5, 0.5))
    return int(tp), int(fp)


@pytest.mark.parametrize("k", [65, 96, 127, 128])
@pytest.mark.parametrize("m,n", [(1, 1), (37, 63), (300, 517), (130, 4200)])
def test_cover_count_wide_random(L, k, m, n):
    rs = np.random.RandomState(m * 131 + n + k)
    X = (rs.rand(m, n) < 0.3).astype(np.uint8)
    Ub = (rs.rand(m, k) < 0.04).astype(np.uint8)
    Vb = (rs.rand(n, k) < 0.04).astype(np.uint8)
    if m > 2:
        Ub[1, :] = 0          # a row with no factor
        X[2, :] = 0           # an empty row of X
    assert cover_counts(L, X, Ub, Vb) == want_counts(X, Ub, Vb), (k, m, n)


@pytest.mark.parametrize("k", [65, 128])
def test_cover_count_wide_edges(L, k):
    rs = np.random.RandomState(k)
    m, n = 200, 700
    X = (rs.rand(m, n) < 0.3).astype(np.uint8)
    # a cover that comes only from block 1
    Ub = np.zeros((m, k), np.uint8)
    Vb = np.zeros((n, k), np.uint8)
    Ub[:, BK:] = rs.rand(m, k - BK) < 0.3
    Vb[:, BK:] = rs.rand(n, k - BK) < 0.3
    want = want_counts(X, Ub, Vb)
    assert want[0] > 0 and cover_counts(L, X, Ub, Vb) == want
    # only factor 63 (bit 63 of the first word), only the last factor (bit 63 of the second word at k = 128)
    for f in (BK - 1, k - 1):
        Ub = np.zeros((m, k), np.uint8)
        Vb = np.zeros((n, k), np.uint8)
        Ub[rs.rand(m) < 0.5, f] = 1
        Vb[rs.rand(n) < 0.5, f] = 1
        want = want_counts(X, Ub, Vb)
        assert want[0] > 0 and want[1] > 0 and cover_counts(L, X, Ub, Vb) == want, f
    Ub = (rs.rand(m, k) < 0.05).astype(np.uint8)
    Vb = (rs.rand(n, k) < 0.05).astype(np.uint8)
    for Xe in (np.zeros((m, n), np.uint8), np.ones((m, n), np.uint8)):
        assert cover_counts(L, Xe, Ub, Vb) == want_counts(Xe, Ub, Vb)
    # the counts accumulate over calls
    tp, fp = want_counts(X, Ub, Vb)
    assert cover_counts(L, X, Ub, Vb, calls=2) == (2 * tp, 2 * fp)


# ---- bmf_resid_sums_wide: sum |X - U V^T|, sum (X - U V^T)^2 ---------------------------------------------------------------------
def resid_sums(L, X, U, V, m_pad, n_pad, tiled):
    ldxt = m_pad // 32
    XT = dev(pack_rows(X.T, n_pad, ldxt))
    if tiled:
        T = torch.empty_like(XT)
        L.check(L.lib.bmf_tile_bits(L.ptr(XT), n_pad, ldxt, ldxt, L.ptr(T), stream()), "bmf_tile_bits")
        XT = T
    UA, UB = two_blocks(U, m_pad)
    VA, VB = two_blocks(V, n_pad)
    ws = torch.full(((m_pad + n_pad) * 2 * BK,), F16_NAN, dtype=torch.int16, device="cuda")
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_resid_sums_wide(L.ptr(XT), ldxt, m_pad, n_pad, L.ptr(UA), L.ptr(UB), L.ptr(VA), L.ptr(VB), L.ptr(ws), L.ptr(sums),
                                      int(tiled), stream()), "bmf_resid_sums_wide")
    return sums.cpu().numpy()


def want_sums(X, U, V):
    R = X.astype(np.float64) - f32(U) @ f32(V).T
    return np.abs(R).sum(), (R * R).sum()


def near_exact(rs, m, n, k, spread=0.03):
    """X = Ub Vb^T with one factor per row of U (a disjoint cover, 0 / 1 exactly, spread over both blocks), and U, V that reproduce
    it to within a few percent per cell: the per-cell error of the product is what the sums see."""
    Ub = np.zeros((m, k))
    Ub[np.arange(m), rs.randint(k, size=m)] = 1.0
    Vb = (rs.rand(n, k) < 0.3).astype(np.float64)
    X = (Ub @ Vb.T).astype(np.uint8)
    return X, Ub * (1 + spread * rs.standard_normal((m, k))), Vb * (1 + spread * rs.standard_normal((n, k)))


SHAPES = [(1, 1), (1, 63), (37, 64), (256, 300), (300, 1), (300, 63), (1000, 64), (5000, 300)]


@pytest.mark.parametrize("k", [65, 100, 128])
@pytest.mark.parametrize("m,n", SHAPES)
def test_resid_sums_wide(L, m, n, k):
    """Random factors with magnitudes over 1e-3 .. 1, and a near-exact fit; plain and tiled X^T.  The scalar gate, 1e-4 relative,
    at every size: below 2^24 padded cells one fp16 product per cell does not average out."""
    rs = np.random.RandomState(m * 7 + n + k)
    m_pad = -(-m // 256) * 256
    X = (rs.rand(m, n) < 0.3).astype(np.uint8)
    U = np.abs(rs.standard_normal((m, k))) * 0.4 * 10.0 ** rs.uniform(-3, 0, (m, k))
    V = np.abs(rs.standard_normal((n, k))) * 0.4
    Xn, Un, Vn = near_exact(rs, m, n, k)
    for tiled in (False, True):
        mp, np_ = (-(-m // 512) * 512, -(-n // 512) * 512) if tiled else (m_pad, -(-n // 64) * 64)
        for case, (Xc, Uc, Vc) in (("random", (X, U, V)), ("near-exact", (Xn, Un, Vn))):
            got = resid_sums(L, Xc, Uc, Vc, mp, np_, tiled)
            want = want_sums(Xc, Uc, Vc)
            assert np.isfinite(got).all()
            assert got[0] == pytest.approx(want[0], rel=1e-4, abs=1e-9), (case, tiled, got[0] / want[0] - 1)
            assert got[1] == pytest.approx(want[1], rel=1e-4, abs=1e-12), (case, tiled, got[1] / want[1] - 1)


def test_resid_sums_wide_at_2_24_cells(L):
    """From 2^24 padded cells the single fp16 product per cell (its error averages out over the sum): random factors."""
    rs = np.random.RandomState(3)
    m, n, k = 4000, 4096, 97
    X = (rs.rand(m, n) < 0.3).astype(np.uint8)
    U = np.abs(rs.standard_normal((m, k))) * 0.1
    V = np.abs(rs.standard_normal((n, k))) * 0.1
    want = want_sums(X, U, V)
    for tiled in (False, True):
        got = resid_sums(L, X, U, V, 4096, 4096, tiled)
        assert got[0] == pytest.approx(want[0], rel=2e-5) and got[1] == pytest.approx(want[1], rel=2e-5), (tiled, got / np.array(want) - 1)


def test_resid_sums_wide_accumulates_and_refuses(L):
    rs = np.random.RandomState(8)
    m, n, k = 40, 70, 90
    X = (rs.rand(m, n) < 0.4).astype(np.uint8)
    U, V = rs.rand(m, k) * 0.1, rs.rand(n, k) * 0.1
    XT = dev(pack_rows(X.T, 128, 8))
    UA, UB = two_blocks(U, 256)
    VA, VB = two_blocks(V, 128)
    ws = torch.zeros(((256 + 128) * 2 * BK,), dtype=torch.int16, device="cuda")
    sums = torch.tensor([1.0, 2.0], dtype=torch.float64, device="cuda")
    args = (L.ptr(UA), L.ptr(UB), L.ptr(VA), L.ptr(VB), L.ptr(ws), L.ptr(sums))
    L.check(L.lib.bmf_resid_sums_wide(L.ptr(XT), 8, 256, 128, *args, 0, stream()), "bmf_resid_sums_wide")
    want = want_sums(X, U, V)
    got = sums.cpu().numpy()
    assert got[0] == pytest.approx(1.0 + want[0], rel=1e-6) and got[1] == pytest.approx(2.0 + want[1], rel=1e-6)
    assert L.lib.bmf_resid_sums_wide(L.ptr(XT), 8, 128, 128, *args, 0, stream()) == -1    # m_pad % 256
    assert L.lib.bmf_resid_sums_wide(L.ptr(XT), 8, 256, 96, *args, 0, stream()) == -1     # n_pad % 64
    assert L.lib.bmf_resid_sums_wide(L.ptr(XT), 8, 256, 128, *args, 1, stream()) == -1    # tiled: n_pad % 256, ldxt % 16


# ---- bmf_masked_pass_wide / bmf_masked_counts_wide on rows of several 64-cell segments -------------------------------------------
@pytest.mark.parametrize("k", [65, 128])
@pytest.mark.parametrize("weighted", [False, True])
def test_masked_pass_wide_long_rows(L, k, weighted):
    from pybmf_amd.engine import SparseObs
    rs = np.random.RandomState(k + weighted)
    m, n = 300, 517
    obs = rs.rand(m, n) < 0.05
    obs[7, :] = True       # one row observes every column: nine segments
    obs[:, 100] = True     # one column observes every row: five segments
    obs[11, :] = False     # an empty row
    r, c = np.nonzero(obs)
    vals = (rs.rand(len(r)) < 0.4).astype(np.float32)
    w = (rs.rand(len(r)) + 0.5).astype(np.float32) if weighted else None
    S = SparseObs(r, c, vals, w, (m, n))
    assert S.csr["nseg"] > m and S.csc["nseg"] > n
    U = (rs.rand(m, k) * 0.3).astype(np.float32)
    V = (rs.rand(n, k) * 0.3).astype(np.float32)
    Wd = np.zeros((m, n))
    Wd[r, c] = 1.0 if w is None else f32(w)
    Xd = np.zeros((m, n))
    Xd[r, c] = vals
    U64, V64 = f32(U), f32(V)
    P = U64 @ V64.T
    for ls, rows, Fs, Fo, Fo64, Wx, Wp in ((S.csr, m, U, V, V64, Wd * Xd, Wd * P), (S.csc, n, V, U, U64, (Wd * Xd).T, (Wd * P).T)):
        Fs0, Fs1 = two_blocks(Fs, rows)
        Fo0, Fo1 = two_blocks(Fo, Fo.shape[0])
        part = [nan_f32((max(ls["nseg"], 1), 2, BK)) for _ in range(2)]
        num = [nan_f32((rows, BK)) for _ in range(2)]
        den = [nan_f32((rows, BK)) for _ in range(2)]
        sums = torch.zeros(2, dtype=torch.float64, device="cuda")
        L.check(L.lib.bmf_masked_pass_wide(L.ptr(ls["ptr"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), L.ptr(ls["wgt"]), rows, L.ptr(ls["seg_row"]),
                                           L.ptr(ls["seg_beg"]), ls["nseg"], L.ptr(ls["row_seg_ptr"]), L.ptr(Fs0), L.ptr(Fs1), L.ptr(Fo0), L.ptr(Fo1),
                                           L.ptr(part[0]), L.ptr(part[1]), L.ptr(num[0]), L.ptr(num[1]), L.ptr(den[0]), L.ptr(den[1]),
                                           L.ptr(sums), stream()), "bmf_masked_pass_wide")
        want_num, want_den = Wx @ Fo64, Wp @ Fo64
        for b in range(2):
            cols = slice(BK * b, min(BK * b + BK, k))
            kb = cols.stop - cols.start
            gn, gd = num[b].cpu().numpy(), den[b].cpu().numpy()
            assert np.isfinite(gn).all() and np.isfinite(gd).all(), b
            np.testing.assert_allclose(gn[:, :kb], want_num[:, cols], rtol=2e-5, atol=1e-6)
            np.testing.assert_allclose(gd[:, :kb], want_den[:, cols], rtol=2e-5, atol=1e-6)
            assert not gn[:, kb:].any() and not gd[:, kb:].any()   # the zero padding of the factors stays zero
            if ls is S.csr:
                assert not gn[11].any() and not gd[11].any()       # the empty row
        assert float(sums[0]) == pytest.approx(float((Wd * (Xd - P) ** 2).sum()), rel=1e-5)
        assert float(sums[1]) == pytest.approx(float((Wd * np.abs(Xd - P)).sum()), rel=1e-5)
    # the observed-cell counts with both blocks: a cover from block 0 only, block 1 only, factor 63, the last factor, and all
    Ubits, Vbits = U > 0.25, V > 0.25
    for sel in (slice(0, BK), slice(BK, k), slice(BK - 1, BK), slice(k - 1, k), slice(0, k)):
        Ub = np.zeros((m, k), np.uint8)
        Vb = np.zeros((n, k), np.uint8)
        Ub[:, sel], Vb[:, sel] = Ubits[:, sel], Vbits[:, sel]
        (ua, _), (ub, _) = factor_bits(Ub, 512)
        (va, _), (vb, _) = factor_bits(Vb, 1024)
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        ls = S.csr
        L.check(L.lib.bmf_masked_counts_wide(L.ptr(ls["cell_row"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), len(r), L.ptr(ua), L.ptr(ub), L.ptr(va),
                                             L.ptr(vb), L.ptr(counts), stream()), "bmf_masked_counts_wide")
        pd = ((Ub.astype(np.int64) @ Vb.T.astype(np.int64)) > 0)[r, c]
        gt = vals != 0
        want = (int((gt & pd).sum()), int((~gt & pd).sum()), int((gt & ~pd).sum()), int((~gt & ~pd).sum()))
        assert tuple(int(v) for v in counts.cpu().numpy()) == want, sel
