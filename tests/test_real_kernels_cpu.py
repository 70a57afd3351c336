"""tests/real_kernels_ref.py proved on the CPU: the restated orders are permutations (with their inverses) and agree with the formulas
written as plain loops, the bf16 splits are what the headers say, the exact contraction inputs are exact in fp32 in any order and on
the three-way split path, no stage partial of a real (row, column) vanishes, and the emulated six-product contraction shows which
dropped product the per-element bound of the GPU tests catches."""
import numpy as np
import pytest

import objective_ref as R
import real_kernels_ref as K

ROWS, KPS = [64, 192, 384], [32, 64]
# (stages, splits) of the ring kernels' tests: one split of 1 .. 9 stages, short last splits, one stage each, a zero-stage split, and
# (plain form only) more splits than stages
RING_PLANS = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (9, 1), (8, 3), (17, 2), (23, 4), (5, 5), (5, 4)]
PLAIN_ONLY_PLANS = [(2, 3)]
DIRECT_REDS = [8, 24, 40, 72, 504, 520]


# ---- the orders -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_pad", ROWS)
def test_orders_are_permutations_with_inverses(rows_pad):
    for kp in KPS:
        n = rows_pad * kp
        for src in (K.frag_src(rows_pad, kp), K.frag_rows_src(rows_pad, kp)):
            assert np.array_equal(np.sort(src), np.arange(n))
            inv = K.inverse(src)
            assert np.array_equal(src[inv], np.arange(n)) and np.array_equal(inv[src], np.arange(n))
    for red, lda in ((64, 64), (320, 320), (320, 332)):
        src = K.tile_src(rows_pad, red, lda)
        rows, cols = src // lda, src % lda
        assert np.array_equal(np.sort(rows * red + cols), np.arange(rows_pad * red)) and cols.max() == red - 1     # never the slack of lda
        inv = K.inverse(src, rows_pad * lda)
        assert np.array_equal(inv[src], np.arange(src.size)) and (inv.reshape(rows_pad, lda)[:, red:] == -1).all()
    n = rows_pad * 32
    addend, src = K.frag_rows_bf16_src(rows_pad)
    assert np.array_equal(np.sort(addend * n + src), np.arange(2 * n))             # every (addend, element) exactly once
    part, src = K.frag_bf16x3_src(rows_pad)
    assert np.array_equal(np.sort(part * n + src), np.arange(3 * n))


def test_orders_agree_with_the_formulas_as_loops():
    """the vectorised maps against the header's formulas written out index by index (one stage pair: every field takes every value)"""
    rows_pad, red, lda = 128, 128, 140
    src = K.tile_src(rows_pad, red, lda)
    for tile in range(2):
        for st in range(2):
            for q in range(4):
                for rl in range(32):
                    for c in range(8):
                        i = ((((tile * 2 + st) * 4 + q) * 32 + rl) * 8 + c) * 4
                        want = (64 * tile + 32 * (q & 1) + rl) * lda + 64 * st + 32 * (q >> 1) + 4 * (c ^ ((rl >> 1) & 7))
                        assert src[i:i + 4].tolist() == [want, want + 1, want + 2, want + 3]
    for kp in KPS:
        NT, f, fr = kp // 32, K.frag_src(128, kp), K.frag_rows_src(128, kp)
        for st in range(2):
            for kh in range(2):
                for h in range(2):
                    for r in (0, 5, 31):
                        for u in range(4):
                            for nt in range(NT):
                                i = ((((st * 2 + kh) * 4 + u) * NT + nt) * 64 + 32 * h + r) * 4
                                assert f[i:i + 4].tolist() == [(64 * st + 32 * kh + 8 * u + 4 * h + t) * kp + 32 * nt + r for t in range(4)]
                        for q in range(kp // 8):
                            i = (((st * 2 + kh) * (kp // 8) + q) * 64 + 32 * h + r) * 4
                            want = (64 * st + 32 * kh + r) * kp + (kp // 2) * h + 4 * q
                            assert fr[i:i + 4].tolist() == [want + t for t in range(4)]
    addend, s2 = K.frag_rows_bf16_src(128)
    part, s3 = K.frag_bf16x3_src(128)
    for st in range(2):
        for kh in range(2):
            for h in range(2):
                for r in (0, 5, 31):
                    for q in range(4):
                        for w in range(4):
                            i = 2 * ((((st * 2 + kh) * 4 + q) * 64 + 32 * h + r) * 4 + w)
                            want = (64 * st + 32 * kh + r) * 32 + 16 * (q >> 1) + 8 * h + 2 * w
                            assert s2[i:i + 2].tolist() == [want, want + 1] and addend[i:i + 2].tolist() == [q & 1] * 2
                    for ks in range(2):
                        for p in range(3):
                            for j in range(8):
                                i = 2 * ((((st * 2 + kh) * 2 + ks) * 3 + p) * 256 + (32 * h + r) * 4 + (j >> 1)) + (j & 1)
                                assert s3[i] == (64 * st + 32 * kh + 8 * (2 * ks + (j >> 2)) + 4 * h + (j & 3)) * 32 + r and part[i] == p


def test_position_coded_inputs_name_their_place():
    for rows, cols in ((384, 64), (384, 332)):
        X = K.position_coded(rows, cols)
        assert X.dtype == np.float32 and np.array_equal(X.ravel().astype(np.int64), np.arange(rows * cols) + 1)
    X = K.position_coded(128, 140)
    t = K.tile_f32(X, 128)
    assert np.array_equal(t.astype(np.int64) - 1, K.tile_src(128, 128, 140))


# ---- the bf16 splits ------------------------------------------------------------------------------------------------------------------------
def test_bf16_value_inputs_and_splits():
    F = K.bf16_value_inputs(192, 0)
    bits = F.view(np.uint32)
    mag = np.abs(F[F != 0])
    assert 2.0 ** -20 <= mag.min() and mag.max() < 2.0 ** 21 and (F < 0).sum() > 1000 and (bits == 0x80000000).any() and (bits == 0).any()
    assert ((bits & 0x7FFFFF) == 0).sum() > 300 and ((bits & 0x1FFFF) == 0x8000).sum() > 300 and ((bits & 0x1FFFF) == 0x18000).sum() > 300
    assert ((bits & 0xFF) != 0).mean() > 0.5                                           # full 24-bit mantissas
    hi, lo = K.split2_rne(F)
    h, l = K.as_f32(hi), K.as_f32(lo)
    assert (np.abs(F - h) <= np.abs(F) * 2.0 ** -8).all() and (np.abs((F - h) - l) <= np.abs(F - h) * 2.0 ** -8).all()
    down, up = (bits & 0x1FFFF) == 0x8000, (bits & 0x1FFFF) == 0x18000
    assert np.array_equal(hi[down], (bits[down] >> 16).astype(np.uint16)) and np.array_equal(hi[up], ((bits[up] >> 16) + 1).astype(np.uint16))
    assert np.array_equal(hi[bits == 0x80000000], np.full((bits == 0x80000000).sum(), 0x8000, np.uint16)) and not lo[F == 0].any()
    nxt = (bits & 0x7FFFFF) == 0x7FFFFF                                                 # rounds up into the next binade
    assert nxt.any() and np.array_equal(np.abs(h[nxt]), 2.0 ** (((bits[nxt] >> 23) & 0xFF).astype(np.float64) - 126))
    parts = [K.as_f32(p).astype(np.float64) for p in K.split3_trunc(F)]
    assert np.array_equal(parts[0] + parts[1] + parts[2], F.astype(np.float64))        # hi + mid + lo == x exactly
    assert np.array_equal(K.split3_trunc(F)[0], (bits >> 16).astype(np.uint16))        # truncation, not rounding
    assert (np.abs(parts[1]) <= 2.0 ** -7 * np.abs(parts[0])).all() and (np.abs(parts[2]) <= 2.0 ** -14 * np.abs(parts[0])).all()
    # the applied orders hold what the maps say
    f2 = K.frag_rows_bf16(F).view(np.uint16)
    addend, src = K.frag_rows_bf16_src(192)
    assert np.array_equal(f2, np.where(addend == 0, hi.ravel()[src], lo.ravel()[src]))
    f3 = K.frag_bf16x3(F).view(np.uint16)
    part, src = K.frag_bf16x3_src(192)
    assert f3.size == 192 * 96 and np.array_equal(K.as_f32(f3[part == 1]).astype(np.float64), parts[1].ravel()[src[part == 1]])


# ---- the exact contraction inputs -----------------------------------------------------------------------------------------------------------
def test_dense_factor():
    F = K.dense_factor(1467, 27)
    assert np.array_equal(np.abs(F) * 8, np.rint(np.abs(F) * 8)) and np.abs(F).min() == 0.125 and np.abs(F).max() == 1.0
    assert (F[:, 0::2] > 0).all() and (F[:, 1::2] < 0).all()
    assert all(abs((np.abs(F) == v / 8).mean() - 0.125) < 0.02 for v in range(1, 9))
    assert (np.abs(np.diff(F, axis=0)).sum(1) > 0).all() and (np.abs(np.diff(np.abs(F), axis=1)).sum(0) > 0).all()
    hi, mid, lo = K.split3_trunc(F.astype(np.float32))
    assert np.array_equal(K.as_f32(hi).astype(np.float64), F) and not mid.any() and not lo.any()
    h2, l2 = K.split2_rne(F.astype(np.float32))
    assert np.array_equal(K.as_f32(h2).astype(np.float64), F) and not l2.any()
    A = R.real_x(185, 1467).astype(np.float32)
    assert not K.split3_trunc(A)[1].any() and not K.split3_trunc(A)[2].any()


def fp32_orders(A, F):
    """the contraction accumulated in fp32 forwards and backwards over the reduction index"""
    fwd = np.zeros((A.shape[0], F.shape[1]), np.float32)
    bwd = np.zeros_like(fwd)
    red = A.shape[1]
    for j in range(red):
        fwd += A[:, j:j + 1] * F[j:j + 1, :]
        bwd += A[:, red - 1 - j:red - j] * F[red - 1 - j:red - j, :]
    return fwd, bwd


@pytest.mark.parametrize("rows_pad,red,k,kp", [(192, 1472, 27, 32), (128, 1472, 59, 64), (64, 320, 32, 32), (128, 520, 64, 64)])
def test_exact_contraction_in_fp32_any_order_and_fp64(rows_pad, red, k, kp):
    c = K.contraction_case(rows_pad, red, k, kp)
    A, F = c["A"], c["F"]
    assert not A[c["rows"]:].any() and not A[:, c["real"]:].any() and not F[c["real"]:].any() and not F[:, k:].any()
    assert np.array_equal(A[:c["rows"], :c["real"]].astype(np.float64), R.real_x(c["rows"], c["real"]))
    fwd, bwd = fp32_orders(A, F)
    exact = A.astype(np.float64) @ F.astype(np.float64)
    assert np.array_equal(fwd, bwd) and np.array_equal(fwd.astype(np.float64), exact)
    assert np.array_equal(K.bf3_contraction(A, F), exact)                              # mid = lo = 0: the bf16 x 3 path is exact too
    assert np.abs(exact).max() * 64 < 2 ** 24 and np.array_equal(exact * 64, np.rint(exact * 64))
    # every partial over any subset is bounded by the sum of magnitudes, which stays below 2^24 units
    assert (np.abs(A).astype(np.float64) @ np.abs(F).astype(np.float64)).max() * 64 < 2 ** 24
    if red % 64 == 0:
        # no stage partial of a real (row, column) is zero, and the stages of a row differ from one another
        st = K.slab_products(A, F, K.slab_ranges(red // 64, red // 64), 64)
        assert (st[:, :c["rows"], :k] != 0).all()
        assert (np.abs(np.diff(st[:, :c["rows"], :k], axis=0)) > 0).mean() > 0.95
        # the slabs of a plan add up to the product
        for splits in (1, 3, 4):
            sl = K.slab_products(A, F, K.slab_ranges(red // 64, splits), 64)
            assert np.array_equal(sl.sum(0), exact)


def test_sparse_exact_factor_would_leave_zero_stage_partials():
    """why the contraction takes the dense factor: objective_ref.exact_factor has at most four non-zeros per row"""
    c = R.exact_real_case(185, 1467, 27)
    A = np.zeros((192, 1472))
    A[:185, :1467] = R.real_x(185, 1467)
    F = R.pad_factor(c["V"], 1472, 32, np.float64)
    st = K.slab_products(A, F, K.slab_ranges(23, 23), 64)[:, :185, :27]
    assert 0.05 < (st == 0).mean() < 0.15
    fwd, bwd = fp32_orders(A.astype(np.float32), F.astype(np.float32))                 # ... though it is exact in any order as well
    assert np.array_equal(fwd, bwd) and np.array_equal(fwd.astype(np.float64), A @ F)


def test_slab_ranges_of_the_plans():
    assert K.slab_ranges(8, 3) == [(0, 3), (3, 6), (6, 8)] and K.slab_ranges(17, 2) == [(0, 9), (9, 17)]
    assert K.slab_ranges(23, 4) == [(0, 6), (6, 12), (12, 18), (18, 23)] and K.slab_ranges(5, 5) == [(s, s + 1) for s in range(5)]
    assert K.slab_ranges(5, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)]                     # a zero-stage split
    assert K.slab_ranges(2, 3) == [(0, 1), (1, 2), (2, 2)]                             # splits above stages
    per = {-(-s // p) if s % p == 0 or p == 1 else None for s, p in RING_PLANS}
    assert {1, 2, 3, 4, 5, 6, 7, 9} <= per
    # the direct kernel: 1, 3, 5, 9, 63, 65 groups of 8 -- the four-at-a-time loop zero, one and many times, with every remainder 0 .. 3
    groups = [r // 8 for r in DIRECT_REDS]
    assert groups == [1, 3, 5, 9, 63, 65]
    rem = {(b - a) % 4 for g in groups for s in (1, 2, 3) if s <= g for a, b in K.slab_ranges(g, s)}
    assert rem == {0, 1, 2, 3}
    # the unaligned-out case: 3 stages = 24 groups in 5 slabs splits differently by stages and by groups
    assert K.slab_ranges(3, 5) == [(0, 1), (1, 2), (2, 3), (3, 3), (3, 3)] and K.slab_ranges(24, 5) == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 24)]


@pytest.mark.parametrize("rows_pad,red,k", [(64, 320, 27), (192, 1472, 27), (192, 1472, 32)])
def test_residual_case_is_exact(rows_pad, red, k):
    c = K.residual_case(rows_pad, red, k)
    A, F, G = (c[x].astype(np.float64) for x in "AFG")
    r = A - G @ F.T
    assert np.abs(r).max() <= 4 and np.array_equal(r * 64, np.rint(r * 64))
    assert (float(np.abs(r).sum()), float((r * r).sum())) == (c["s_abs"], c["s_sq"])   # the zero padding adds nothing
    assert not K.split2_rne(c["F"])[1].any() and not K.split2_rne(c["G"])[1].any()     # hi is the value, lo = 0
    out = A @ F
    fwd, bwd = fp32_orders(c["A"], c["F"])
    assert np.array_equal(fwd, bwd) and np.array_equal(fwd.astype(np.float64), out)
    # a start value of the sums that the exact sums add to without rounding
    assert (3.5 + c["s_abs"]) - c["s_abs"] == 3.5 and (-1.25 + c["s_sq"]) - c["s_sq"] == -1.25


def test_cross_term_probe_values():
    """a 16-bit value has a non-zero hi and lo, hi + lo is the value, and f * f is not an fp32 number (so s_sq = float32(f * f) names the
    kernel's own fma)"""
    f = np.float32(1.0 + 2.0 ** -7 + 2.0 ** -9 + 2.0 ** -15)
    hi, lo = K.split2_rne(np.array([f]))
    assert K.as_f32(hi)[0] != 0 and K.as_f32(lo)[0] != 0 and K.as_f32(hi)[0] + K.as_f32(lo)[0] == f
    assert np.float64(f) * np.float64(f) != np.float64(np.float32(np.float64(f) * np.float64(f)))
    assert K.as_f32(hi)[0] != f and K.as_f32(lo)[0] != f


# ---- the bound of the general-data test and what it catches --------------------------------------------------------------------------------
def test_per_element_bound_catches_every_dropped_product_with_a_hi_operand():
    """|got - fp64| <= 3e-6 (|A| @ |F|) per element, the project's bound (test_tiled_real_matrix_kernels) applied per element.  The
    six-product contraction in fp64 is well inside it; without any product that has a `hi` operand it is outside for EVERY real element,
    so the GPU test cannot pass with one of them lost.  mid * mid is of the order 2^-16 of the scale times the two relative remainders
    and is recorded, not required."""
    c = K.general_case(192, 1472, 27)
    A, F = c["A"], c["F"]
    assert A.min() >= 0 and F.min() >= 0
    exact = A.astype(np.float64) @ F.astype(np.float64)
    scale = np.abs(A).astype(np.float64) @ np.abs(F).astype(np.float64)
    real = np.zeros(exact.shape, bool)
    real[:c["rows"], :27] = True
    err = lambda got: np.abs(got - exact)[real] / scale[real]   # noqa: E731
    assert err(K.bf3_contraction(A, F)).max() < 2.0 ** -23                              # what the six products leave out: lo * mid and below
    caught = {}
    for drop in K.BF3_PRODUCTS:
        caught[drop] = float((err(K.bf3_contraction(A, F, drop)) > 3e-6).mean())
        if "hi" in drop:
            assert caught[drop] == 1.0, (drop, caught[drop])
    print("fraction of elements outside 3e-6 without mid * mid:", caught[("mid", "mid")])
    assert 0.0 <= caught[("mid", "mid")] <= 1.0
