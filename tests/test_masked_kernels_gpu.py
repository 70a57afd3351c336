"""Every observed-cell kernel of csrc/masked.hip and csrc/thresh64.hip, one direct call per template instantiation, against the
cell-by-cell fp64 restatements of tests/masked_ref.py (pinned to the oracle by tests/test_masked_kernels_cpu.py), evaluated on the
values the kernel sees: the fp32-rounded factors, values and weights for the fp32 kernels, the fp64 factors for thresh64.

Which template each case selects (masked_pass_launch: G = 64 at kp = 64, else 16 for kcols <= 16, else 32):

  (k, kcols, kp)   G    masked_segments_kernel<KP, LINK, G>, LINK = 0 / SIGMOID / KL      masked_rows_kernel
  (3, 3, 32)       16   <32, 0, 16>  <32, SIGMOID, 16>  <32, KL, 16>                      <32>
  (16, 16, 32)     16   the same three, every lane of a 16-lane group in use
  (17, 17, 32)     32   <32, 0, 32>  <32, SIGMOID, 32>  <32, KL, 32>                      <32>
  (32, 32, 32)     32   the same three, every lane in use        (kcols = kp: also through bmf_masked_link_pass)
  (9, 32, 32)      32   the same three, told nothing about the width: what bmf_masked_pass / bmf_masked_link_pass select
  (33, 33, 64)     64   <64, 0, 64>  <64, SIGMOID, 64>  <64, KL, 64>                      <64>
  (64, 64, 64)     64   the same three, every lane in use        (kcols = kp: also through bmf_masked_link_pass)

  That is nine of the twelve instantiations.  The other three, <32, LINK, 64>, are compiled but no argument reaches them: with kp = 32
  the launcher picks G = 16 or 32 whatever kcols is (kcols <= kp is required), so they cannot be called through the C interface.

  masked_thresh64_launch, the same rule on kcols = k:        masked64_kernel<KP, GRAD, G>, GRAD = false / true
  k = 3, 16   (kp 32)   G = 16                                <32, false, 16>  <32, true, 16>
  k = 17, 32  (kp 32)   G = 32                                <32, false, 32>  <32, true, 32>     (k = 32 also through bmf_masked_thresh64)
  k = 33, 64  (kp 64)   G = 64                                <64, false, 64>  <64, true, 64>     (k = 64 also through bmf_masked_thresh64)

  bmf_masked_thresh (fp32):  kp = 32 / 64, dUs = dVs = NULL / given      masked_thresh_kernel<32, false> <32, true> <64, false> <64, true>

Gates.  fp32 segment kernels: num / den rtol 2e-5 + atol 1e-6, sums rel 1e-5 (plain link, the gate of test_masked_gpu.py) or 2e-5 (sigmoid
and KL, the gate of test_link_gpu.py for the same quantities of the dense link pass).  fp64: F rel 1e-11 + abs 1e-9, dF 1e-9 (max|dF| + 1),
transform 1e-14 relative (the gates of test_thresh_eval64_against_golden / test_thresh_trace64_shapes).  bmf_masked_thresh: F rel 2e-6, dF
2e-5 (max|dF| + 1) (the same-inputs comparison of test_thresh_eval_against_golden).  No entry is left out of any comparison.  Every case
records its worst error as a fraction of its gate; run with -s to see the table printed when the module ends."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import masked_ref as R  # noqa: E402
import oracle as orc  # noqa: E402

N = 600
# a row on each side of every step boundary of the three group widths (4 / 8 / 16 / 32 cells per step), an empty row, and a row of ten
# 64-cell segments (masked_rows_kernel: one unrolled batch of eight and a tail of two); then 40 random lengths
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 600] + \
    np.random.RandomState(2024).randint(1, 201, size=40).tolist()
M = len(LENGTHS)
EMPTY_ROW, ZROW, FULL_COL, ZCOL = 0, 5, 123, 77     # ZROW / ZCOL: the zero factor rows of the KL cases (every cell there has x = 0)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    print()
    for key in sorted(WORST, key=str):
        print("WORST", key, " ".join(f"{n}={v:.3g}" for n, v in sorted(WORST[key].items())))


def note(key, **figures):
    slot = WORST.setdefault(key, {})
    for name, value in figures.items():
        slot[name] = max(slot.get(name, 0.0), float(value))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gate_fraction(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is what np.testing.assert_allclose(rtol, atol) accepts"""
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def lanes_per_cell(kp, kcols):
    return 64 if kp == 64 else (16 if kcols <= 16 else 32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the shared cell lists (fixed seeds; every value and weight is exact in fp32) and their device forms
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cells(real, weights):
    rs = np.random.RandomState(100 + 2 * real + weights)
    rows, cols, x, w = R.make_cells(LENGTHS, N, rs, real=real, weights=weights, full_col=FULL_COL)
    if real:
        x[(rows == ZROW) | (cols == ZCOL)] = 0.0
        assert (cols == ZCOL).sum() >= 2 and (x == 0).sum() > (rows == ZROW).sum() + (cols == ZCOL).sum()   # stored zeros elsewhere too
    assert np.bincount(rows, minlength=M).tolist() == LENGTHS and np.bincount(cols, minlength=N)[FULL_COL] == M - 1
    for a in (x, w):
        if a is not None:
            assert (a.astype(np.float32).astype(np.float64) == a).all()
            a.setflags(write=False)
    return rows, cols, x, w


@functools.lru_cache(maxsize=None)
def obs(real, weights):
    from pybmf_amd.engine import SparseObs
    rows, cols, x, w = cells(real, weights)
    S = SparseObs(rows, cols, x, w, (M, N))
    assert S.csr["nseg"] == sum((ln + 63) // 64 for ln in LENGTHS) and S.csc["rows"] == N
    return S


@functools.lru_cache(maxsize=None)
def factors(k, kp, link, lamda):
    """fp32 factors, zero padded to kp columns.  Plain link: uniform in (0, 1).  Sigmoid: scaled row by row so that the products span
    about [0, 3] -- lamda (p - 1/2) runs far into both tails.  KL: bounded away from zero, but for one zero row in each factor."""
    rs = np.random.RandomState(1000 * k + 10 * link + int(lamda))
    U, V = np.zeros((M, kp), np.float32), np.zeros((N, kp), np.float32)
    if link == R.LINK_SIGMOID:
        a = np.sqrt(12.0 / k)
        U[:, :k], V[:, :k] = a * rs.rand(M, k) * rs.rand(M, 1), a * rs.rand(N, k) * rs.rand(N, 1)
    elif link == R.LINK_KL:
        U[:, :k], V[:, :k] = rs.rand(M, k) + 0.05, rs.rand(N, k) + 0.05
        U[ZROW], V[ZCOL] = 0.0, 0.0
    else:
        U[:, :k], V[:, :k] = rs.rand(M, k), rs.rand(N, k)
    return U, V


@functools.lru_cache(maxsize=None)
def segments_want(k, kp, link, lamda, weights, transposed):
    rows, cols, x, w = cells(link == R.LINK_KL, weights)
    U, V = factors(k, kp, link, lamda)
    U, V = U[:, :k].astype(np.float64), V[:, :k].astype(np.float64)
    if link == R.LINK_SIGMOID:
        p = np.einsum("ek,ek->e", U[rows], V[cols])
        assert p.min() < 0.05 and p.max() > 2.0 and lamda * (p.max() - 0.5) > 15
    return R.segments_ref(cols, rows, x, w, V, U, link, lamda) if transposed else R.segments_ref(rows, cols, x, w, U, V, link, lamda)


def run_pass(ls, Fs, Fo, kp, kcols, link, lamda, with_sums, entry="bmf_masked_link_pass_k"):
    from pybmf_amd import _lib as L
    rows, nseg = ls["rows"], ls["nseg"]
    num, den = torch.full((rows, kp), -1.0, device="cuda"), torch.full((rows, kp), -1.0, device="cuda")
    part = torch.full((max(nseg, 1), 2, kp), -1.0, device="cuda")
    sums = torch.zeros(2, dtype=torch.float64, device="cuda") if with_sums else None
    head = (L.ptr(ls["ptr"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), L.ptr(ls["wgt"]), rows, L.ptr(ls["seg_row"]), L.ptr(ls["seg_beg"]), nseg,
            L.ptr(ls["row_seg_ptr"]), L.ptr(Fs), L.ptr(Fo), kp)
    tail = (L.ptr(part), L.ptr(num), L.ptr(den), L.ptr(sums))
    if entry == "bmf_masked_link_pass_k":
        L.check(L.lib.bmf_masked_link_pass_k(*head, kcols, *tail, link, float(lamda), stream()), entry)
    elif entry == "bmf_masked_link_pass":
        L.check(L.lib.bmf_masked_link_pass(*head, *tail, link, float(lamda), stream()), entry)
    else:
        raise ValueError(entry)
    return num.cpu().numpy(), den.cpu().numpy(), None if sums is None else sums.cpu().numpy()


def check_pass(got, want, k, kp, link, key, zero_rows):
    num, den, sums = got
    wnum, wden, wsums = want
    assert np.isfinite(num).all() and np.isfinite(den).all()
    assert (num >= 0).all() and (den >= 0).all()                       # every entry overwritten: the -1 prefill is gone
    for r in zero_rows:
        assert (num[r] == 0).all() and (den[r] == 0).all()
    assert (num[:, k:] == 0).all() and (den[:, k:] == 0).all()         # padding columns: exactly zero
    if link == R.LINK_KL:
        assert (den == 0).all()
    fn, fd = gate_fraction(num[:, :k], wnum, 2e-5, 1e-6), gate_fraction(den[:, :k], wden, 2e-5, 1e-6)
    big = np.abs(wnum) > 1e-2
    note(key, num_gate=fn, den_gate=fd, num_rel=(np.abs(num[:, :k] - wnum)[big] / np.abs(wnum)[big]).max() if big.any() else 0.0)
    print(key, f"num {fn:.3f} den {fd:.3f} of the gate")
    np.testing.assert_allclose(num[:, :k], wnum, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(den[:, :k], wden, rtol=2e-5, atol=1e-6)
    if sums is not None:
        rel = 1e-5 if link == R.LINK_PLAIN else 2e-5
        s0 = abs(sums[0] - wsums[0]) / abs(wsums[0])
        s1 = abs(sums[1] - wsums[1]) / abs(wsums[1]) if wsums[1] else abs(sums[1])
        note(key, sums0_gate=s0 / rel, sums1_gate=s1 / rel)
        print(key, f"sums {s0:.3g} {s1:.3g} relative")
        assert sums[0] == pytest.approx(wsums[0], rel=rel)
        if link == R.LINK_KL:
            assert sums[1] == 0.0
        else:
            assert sums[1] == pytest.approx(wsums[1], rel=rel)


SHAPES = [(3, 3, 32), (16, 16, 32), (17, 17, 32), (32, 32, 32), (9, 32, 32), (33, 33, 64), (64, 64, 64)]
LINKS = [(R.LINK_PLAIN, 0.0), (R.LINK_SIGMOID, 10.0), (R.LINK_SIGMOID, 100.0), (R.LINK_KL, 0.0)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. bmf_masked_link_pass_k
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True], ids=["mask", "weights"])
@pytest.mark.parametrize("link,lamda", LINKS, ids=["plain", "sigmoid10", "sigmoid100", "kl"])
@pytest.mark.parametrize("k,kcols,kp", SHAPES)
def test_link_pass_k_cell_by_cell(k, kcols, kp, link, lamda, weights):
    """Every reachable masked_segments_kernel instantiation (table above), with and without weights, with sums and without, both
    orientations, on rows of every length around the step boundaries.  Each call: outputs fully overwritten, empty / zero rows and padding
    columns exactly zero, num / den / sums inside the gate, and bit-identical num / den when repeated.

    Measured on an MI355X against tests/masked_ref.py, worst over every case and both orientations, as a fraction of the num / den gate
    (rtol 2e-5 + atol 1e-6) | worst relative error of the entries above 1e-2 | worst relative error of sums:
      plain            G16 0.009  G32 0.012  G64 0.023   | 2.6e-7 | 4.1e-9
      KL               G16 0.010  G32 0.011  G64 0.020   | 4.0e-7 | 1.4e-9
      sigmoid 10       G16 0.032  G32 0.041  G64 0.036   | 1.7e-6 | 3.5e-9
      sigmoid 100      G16 0.32   G32 0.38   G64 0.31    | 7.3e-6 | 4.5e-9
    so __expf and the fp32 product under lamda = 100 stay inside the gate of the dense link pass, and the gates are kept as they were."""
    S = obs(link == R.LINK_KL, weights)
    U, V = factors(k, kp, link, lamda)
    Ud, Vd = dev(U), dev(V)
    for transposed, ls, Fs, Fo, zrow in ((False, S.csr, Ud, Vd, ZROW), (True, S.csc, Vd, Ud, ZCOL)):
        want = segments_want(k, kp, link, lamda, weights, transposed)
        key = ("link_pass", ("plain", "sigmoid", "kl")[link], f"G{lanes_per_cell(kp, kcols)}", f"kp{kp}", f"lamda{lamda:g}")
        zero_rows = ([EMPTY_ROW] if not transposed else []) + ([zrow] if link == R.LINK_KL else [])
        first = run_pass(ls, Fs, Fo, kp, kcols, link, lamda, True)
        check_pass(first, want, k, kp, link, key, zero_rows)
        again = run_pass(ls, Fs, Fo, kp, kcols, link, lamda, True)
        bare = run_pass(ls, Fs, Fo, kp, kcols, link, lamda, False)
        check_pass(bare, want, k, kp, link, key, zero_rows)
        for other in (again, bare):          # fixed order of additions: the same bits, with or without the residual sums
            assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])
        if kcols == kp:                      # bmf_masked_link_pass is the same launch
            plain = run_pass(ls, Fs, Fo, kp, kcols, link, lamda, True, entry="bmf_masked_link_pass")
            assert np.array_equal(first[0], plain[0]) and np.array_equal(first[1], plain[1])
            assert plain[2][0] == pytest.approx(first[2][0], rel=1e-12) and plain[2][1] == pytest.approx(first[2][1], rel=1e-12)


@pytest.mark.parametrize("k,kp", [(3, 32), (17, 32), (33, 64)])
def test_kl_zero_factor_row_adds_exactly_nothing(k, kp):
    """The cells of the zero factor row alone (all x = 0, p = 0): the numerator, and this row's whole contribution to sums[0], are exactly
    0 -- 0 log 0 = 0 and no 0 / 0."""
    from pybmf_amd.engine import SparseObs
    rows, cols, x, w = cells(True, True)
    sel = rows == ZROW
    assert sel.sum() == LENGTHS[ZROW] and (x[sel] == 0).all()
    S = SparseObs(rows[sel], cols[sel], x[sel], w[sel], (M, N))
    U, V = factors(k, kp, R.LINK_KL, 0.0)
    assert (U[ZROW] == 0).all()
    num, den, sums = run_pass(S.csr, dev(U), dev(V), kp, k, R.LINK_KL, 0.0, True)
    assert (num == 0).all() and (den == 0).all() and sums[0] == 0.0 and sums[1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. the grid-stride loop of masked_segments_kernel: more than 8192 blocks x 4 waves of segments
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_rows():
    from pybmf_amd.engine import SparseObs
    rs = np.random.RandomState(7)
    m, n = 33000, 50
    rows, cols, x, w = R.make_cells(rs.randint(1, 3, size=m).tolist(), n, rs, weights=True)
    return (m, n), (rows, cols, x, w), SparseObs(rows, cols, x, w, (m, n))


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("link,lamda", [(R.LINK_PLAIN, 0.0), (R.LINK_SIGMOID, 10.0)], ids=["plain", "sigmoid10"])
def test_link_pass_strides_over_more_segments_than_waves(link, lamda, kp):
    (m, n), (rows, cols, x, w), S = many_rows()
    k = 6
    assert S.csr["nseg"] > 32768                       # 8192 blocks of 4 waves: above this the segment loop takes a second trip
    rs = np.random.RandomState(8)
    U, V = np.zeros((m, kp), np.float32), np.zeros((n, kp), np.float32)
    scale = np.sqrt(12.0 / k) if link == R.LINK_SIGMOID else 1.0
    U[:, :k], V[:, :k] = scale * rs.rand(m, k) * rs.rand(m, 1), scale * rs.rand(n, k)
    want = R.segments_ref(rows, cols, x, w, U[:, :k].astype(np.float64), V[:, :k].astype(np.float64), link, lamda)
    got = run_pass(S.csr, dev(U), dev(V), kp, k, link, lamda, True)
    check_pass(got, want, k, kp, link, ("link_pass_stride", ("plain", "sigmoid")[link], f"G{lanes_per_cell(kp, k)}"), [])


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. bmf_thresh_transform64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,rows_pad,k,kp", [(70, 128, 20, 32), (5, 64, 40, 64), (300, 301, 32, 32)])
@pytest.mark.parametrize("lamda", [10.0, 100.0])
def test_thresh_transform64_against_the_oracle(rows, rows_pad, k, kp, lamda):
    """S = sigmoid(lamda (F - x)) and D = dXdx(F, x) to 1e-14 relative on every real entry, padding rows and columns exactly 0 whatever F
    holds there, D = NULL accepted; entries 10 above and 10 below the threshold at lamda = 100 (|z| = 1000: the reference's own
    exp(-z) sigmoid(z)^2 is inf * 0 there) come out finite, as the limits 1 / 0 and 0 / 0."""
    from pybmf_amd import _lib as L
    rs = np.random.RandomState(rows + k)
    x = 0.4
    F = rs.rand(rows_pad, kp) * 1.2 - 0.1                    # garbage in the padding too: the kernel must not look at it
    F[0, 0], F[1, 1], F[2, 0] = x + 10.0, x - 10.0, x        # far tails, and exactly on the threshold
    Fd = dev(F)
    S, D = torch.full((rows_pad, kp), -1.0, dtype=torch.float64, device="cuda"), torch.full((rows_pad, kp), -1.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_thresh_transform64(L.ptr(Fd), rows_pad, rows, k, kp, x, lamda, L.ptr(S), L.ptr(D), stream()))
    S, D = S.cpu().numpy(), D.cpu().numpy()
    assert np.isfinite(S).all() and np.isfinite(D).all()
    assert (S[rows:] == 0).all() and (D[rows:] == 0).all() and (S[:, k:] == 0).all() and (D[:, k:] == 0).all()
    wantS = orc.stable_sigmoid((F[:rows, :k] - x) * lamda)
    wantD = orc.thresh_dXdx(F[:rows, :k], x, lamda)
    ok = np.isfinite(wantD)                                  # the reference's form overflows for z < -709: the limit there is 0
    assert ok.sum() >= wantD.size - 1 and (lamda < 100 or not ok[1, 1])
    assert (D[:rows, :k][~ok] == 0).all()
    assert S[0, 0] == 1.0 and S[2, 0] == 0.5 and D[2, 0] == lamda / 4
    eS = np.abs(S[:rows, :k] - wantS) / wantS.clip(1e-300)
    eD = np.abs(D[:rows, :k] - wantD)[ok] / np.abs(wantD[ok]).clip(1e-300)
    note(("transform64", f"lamda{lamda:g}"), S_rel=eS.max(), D_rel=eD.max())
    print("transform64", lamda, f"S {eS.max():.3g} D {eD.max():.3g} relative")
    np.testing.assert_allclose(S[:rows, :k], wantS, rtol=1e-14, atol=0)
    np.testing.assert_allclose(D[:rows, :k][ok], wantD[ok], rtol=1e-14, atol=0)
    S2 = torch.full((rows_pad, kp), -1.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_thresh_transform64(L.ptr(Fd), rows_pad, rows, k, kp, x, lamda, L.ptr(S2), None, stream()))
    assert np.array_equal(S2.cpu().numpy(), S)


# ---------------------------------------------------------------------------------------------------------------------------------------
# d. bmf_masked_thresh64_k / bmf_masked_thresh64
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def thresh_want(k, weights, lamda):
    rows, cols, x, w = cells(False, weights)
    rs = np.random.RandomState(50 + k)
    U, V = rs.rand(M, k), rs.rand(N, k)
    u, v = 0.45, 0.6
    return U, V, u, v, R.thresh_ref(rows, cols, x, w, U, V, u, v, lamda)


@pytest.mark.parametrize("lamda", [10.0, 100.0])
@pytest.mark.parametrize("weights", [False, True], ids=["mask", "weights"])
@pytest.mark.parametrize("k", [3, 16, 17, 32, 33, 64])
def test_masked_thresh64_cell_by_cell(k, weights, lamda):
    """All six masked64_kernel instantiations (table above) behind the device transform, as BinaryMFThreshold runs them: F to 1e-11, dF to
    1e-9 (max|dF| + 1), with weights in {0.5, 1, 3} (squared in F, once in dF); 1 and 3 workgroups make the segment loop stride; `out`
    is written (not added to) and bit-identical when repeated."""
    from pybmf_amd import _lib as L
    kp = 32 if k <= 32 else 64
    U, V, u, v, (wf, wg1, wg2) = thresh_want(k, weights, lamda)
    ls = obs(False, weights).csr
    nseg = ls["nseg"]
    Up, Vp = np.zeros((M, kp)), np.zeros((N, kp))
    Up[:, :k], Vp[:, :k] = U, V
    Ud, Vd = dev(Up), dev(Vp)
    Us, dUs = torch.empty((M, kp), dtype=torch.float64, device="cuda"), torch.empty((M, kp), dtype=torch.float64, device="cuda")
    Vs, dVs = torch.empty((N, kp), dtype=torch.float64, device="cuda"), torch.empty((N, kp), dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_thresh_transform64(L.ptr(Ud), M, M, k, kp, u, lamda, L.ptr(Us), L.ptr(dUs), stream()))
    L.check(L.lib.bmf_thresh_transform64(L.ptr(Vd), N, N, k, kp, v, lamda, L.ptr(Vs), L.ptr(dVs), stream()))
    scale = max(abs(wg1), abs(wg2)) + 1.0

    def call(grad, blocks, by_k=True):
        partial = torch.full((4 * blocks,), 7.0, dtype=torch.float64, device="cuda")
        out = torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
        head = (L.ptr(ls["ptr"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), L.ptr(ls["wgt"]), L.ptr(ls["seg_row"]), L.ptr(ls["seg_beg"]), nseg,
                L.ptr(Us), L.ptr(dUs) if grad else None, L.ptr(Vs), L.ptr(dVs) if grad else None, kp)
        if by_k:
            L.check(L.lib.bmf_masked_thresh64_k(*head, k, L.ptr(partial), blocks, L.ptr(out), stream()))
        else:
            L.check(L.lib.bmf_masked_thresh64(*head, L.ptr(partial), blocks, L.ptr(out), stream()))
        return out.cpu().numpy()

    for grad in (False, True):
        for blocks in (1, 3, (nseg + 3) // 4):
            o = call(grad, blocks)
            key = ("masked_thresh64", f"G{lanes_per_cell(kp, k)}", f"lamda{lamda:g}")
            note(key, F_rel=abs(o[0] - wf) / wf, dF_gate=(max(abs(o[1] - wg1), abs(o[2] - wg2)) / (1e-9 * scale)) if grad else 0.0)
            print(key, grad, blocks, f"F {abs(o[0] - wf) / wf:.3g}", f"dF {abs(o[1] - wg1):.3g} {abs(o[2] - wg2):.3g} scale {scale:.3g}")
            assert o[3] == -3.0                                           # three words written, the fourth is not the kernel's
            assert 0.5 * o[0] == pytest.approx(0.5 * wf, rel=1e-11, abs=1e-9)
            if grad:
                assert abs(o[1] - wg1) <= 1e-9 * scale and abs(o[2] - wg2) <= 1e-9 * scale
            else:
                assert o[1] == 0.0 and o[2] == 0.0                        # F only: the gradient words are written as zeros
            assert np.array_equal(o, call(grad, blocks))                  # written, not accumulated; fixed order
            if k == kp:
                assert np.array_equal(o, call(grad, blocks, by_k=False))


# ---------------------------------------------------------------------------------------------------------------------------------------
# e. bmf_masked_thresh, the fp32 form
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", [False, True], ids=["F", "F+dF"])
@pytest.mark.parametrize("k,kp", [(20, 32), (40, 64)])
def test_masked_thresh_fp32_cell_by_cell(k, kp, grad):
    """The four masked_thresh_kernel instantiations on fp32 transformed factors, with weights, against the restatement on the same rounded
    factors; the kernel ADDS to out: a second call doubles it."""
    from pybmf_amd import _lib as L
    rows, cols, x, w = cells(False, True)
    ls = obs(False, True).csr
    rs = np.random.RandomState(60 + k)
    U, V, u, v, lamda = rs.rand(M, k), rs.rand(N, k), 0.45, 0.6, 10.0
    T = []
    for F, t in ((U, u), (V, v)):
        for A in (orc.stable_sigmoid((F - t) * lamda), orc.thresh_dXdx(F, t, lamda)):
            P = np.zeros((F.shape[0], kp), np.float32)
            P[:, :k] = A
            T.append(P)
    Us, dUs, Vs, dVs = T
    wf, wg1, wg2 = R.thresh_cells_ref(rows, cols, x, w, *(A[:, :k].astype(np.float64) for A in (Us, dUs, Vs, dVs)))
    scale = max(abs(wg1), abs(wg2)) + 1.0
    d = [dev(A) for A in T]
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    for times in (1, 2):
        L.check(L.lib.bmf_masked_thresh(L.ptr(ls["ptr"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), L.ptr(ls["wgt"]), L.ptr(ls["seg_row"]),
                                        L.ptr(ls["seg_beg"]), ls["nseg"], L.ptr(d[0]), L.ptr(d[1]) if grad else None, L.ptr(d[2]),
                                        L.ptr(d[3]) if grad else None, kp, L.ptr(out), stream()))
        o = out.cpu().numpy()
        key = ("masked_thresh_fp32", f"kp{kp}")
        note(key, F_gate=abs(o[0] - times * wf) / (times * wf) / 2e-6,
             dF_gate=max(abs(o[1] - times * wg1), abs(o[2] - times * wg2)) / (2e-5 * times * scale) if grad else 0.0)
        print(key, grad, times, f"F {abs(o[0] - times * wf) / (times * wf):.3g}", f"dF {abs(o[1] - times * wg1):.3g} {abs(o[2] - times * wg2):.3g}")
        assert o[3] == 0.0
        assert 0.5 * o[0] == pytest.approx(0.5 * times * wf, rel=2e-6)
        if grad:
            assert abs(o[1] - times * wg1) < 2e-5 * times * scale and abs(o[2] - times * wg2) < 2e-5 * times * scale
        else:
            assert o[1] == 0.0 and o[2] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# f. bmf_masked_counts
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_masked_counts_exact_over_more_cells_than_threads():
    """70 000 cells: more than 256 blocks x 256 threads, so the cell loop strides; bits 0 and 63 alone decide some cells; the counts are
    ADDED to what the four words hold."""
    from pybmf_amd import _lib as L
    from pybmf_amd.engine import SparseObs
    rs = np.random.RandomState(9)
    m, n, nnz = 300, 400, 70000
    flat = np.sort(rs.choice(m * n, size=nnz, replace=False))
    rows, cols = flat // n, flat % n
    x = (rs.rand(nnz) < 0.4).astype(np.float64)
    pool = np.array([0, 1, 1 << 63, (1 << 63) | 1, 1 << 17, (1 << 17) | 1], dtype=np.uint64)
    ub, vb = rs.choice(pool, size=m), rs.choice(pool, size=n)
    both = ub[rows] & vb[cols]
    assert (both == np.uint64(1)).any() and (both == np.uint64(1 << 63)).any() and (both == 0).any()
    S = SparseObs(rows, cols, x, None, (m, n))
    ls = S.csr
    assert nnz > 256 * 256
    start = [5, 6, 7, 1 << 40]
    counts = dev(np.array(start, dtype=np.int64))
    ubd, vbd = dev(ub.view(np.int64)), dev(vb.view(np.int64))
    L.check(L.lib.bmf_masked_counts(L.ptr(ls["cell_row"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), nnz, L.ptr(ubd), L.ptr(vbd), L.ptr(counts), stream()))
    got = [int(c) - s for c, s in zip(counts.cpu().tolist(), start)]
    want = R.counts_ref(rows, cols, x, ub, vb)
    assert tuple(got) == want and sum(got) == nnz and min(want) > 0
    # the other orientation: the same cells by column, the bit words swapped
    lc = S.csc
    counts = dev(np.zeros(4, dtype=np.int64))
    L.check(L.lib.bmf_masked_counts(L.ptr(lc["cell_row"]), L.ptr(lc["idx"]), L.ptr(lc["val"]), nnz, L.ptr(vbd), L.ptr(ubd), L.ptr(counts), stream()))
    assert tuple(counts.cpu().tolist()) == want


# ---------------------------------------------------------------------------------------------------------------------------------------
# g. bmf_masked_scalars
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [True, False], ids=["sums2+counts", "neither"])
def test_masked_scalars_gathers_the_eight_words(extras):
    """nbU = 300 > 256 threads (the strided loop), nbV = 1; only the EVEN words of the partials count (the odd ones hold NaN here); the
    partials are small integers, so every order of additions gives the same double: exact equality."""
    from pybmf_amd import _lib as L
    rs = np.random.RandomState(10)
    nbU, nbV = 300, 1
    partU, partV = np.full(2 * nbU, np.nan), np.full(2 * nbV, np.nan)
    partU[0::2], partV[0::2] = rs.randint(0, 1000, size=nbU), 77.0
    sums = dev(np.array([123.4567, np.nan, np.nan, np.nan]))
    sums2, counts = dev(np.array([3.25, 9.5])), dev(np.array([11, 22, 33, 44], dtype=np.int64))
    out = dev(np.array([-1.0] * 7 + [9.0]))
    pU, pV = dev(partU), dev(partV)
    L.check(L.lib.bmf_masked_scalars(L.ptr(sums), L.ptr(pU), nbU, L.ptr(pV), nbV, L.ptr(sums2) if extras else None,
                                     L.ptr(counts) if extras else None, L.ptr(out), stream()))
    o = out.cpu().numpy()
    assert o[0] == 123.4567 and o[1] == partU[0::2].sum() and o[2] == 77.0 and o[7] == 0.0
    if extras:
        assert o[3:7].tolist() == [3.25, 9.5, 11.0, 22.0]
        assert sums2.cpu().tolist() == [0.0, 0.0] and counts.cpu().tolist() == [0, 0, 33, 44]     # reset for the next iteration
    else:
        assert o[3:7].tolist() == [0.0, 0.0, 0.0, 0.0]
        assert sums2.cpu().tolist() == [3.25, 9.5] and counts.cpu().tolist() == [11, 22, 33, 44]
    assert sums.cpu().numpy()[0] == 123.4567
