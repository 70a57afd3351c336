"""Bit-for-bit NumPy restatements of the three exact-fp32 MFMA kernels behind every k x k Gram matrix and every re-associated
denominator -- gram_partial_kernel<1>, <2> (csrc/util.hip: bmf_gram_partial, bmf_gram_partial_i8), gram_cross_kernel and fg_f32_kernel
(csrc/wide.hip: bmf_gram_cross, bmf_fg_f32) -- with their launch arithmetic (restated, not imported), the input makers, the case tables
and the error bound that tests/test_gram_kernels_cpu.py (which proves all of this on the host) and tests/test_gram_kernels_gpu.py share.

The order every restatement assumes (v_mfma_f32_32x32x2_f32 is a k-ordered chain of fp32 fused multiply-adds, one rounding per term):

  a slab   wave gw = 4 b + w owns the row pairs [gw per, min(gw per + per, pairs)), pairs = rows_pad / 2, per = ceil(pairs / (4 blocks));
           its sum starts at +0.0f and takes, pair after pair ascending, acc = fmaf(A[2p][i], B[2p][j], acc) and then
           acc = fmaf(A[2p + 1][i], B[2p + 1][j], acc) (k = 0 is the even row, k = 1 the odd one; the four pairs of an unrolled trip of
           gram_partial_kernel in the order of the pairs); slab_b = (c_0 + c_1) + (c_2 + c_3) in fp32.  A = B = F for bmf_gram_partial.
  F . G    for s = 0 .. 31: acc = fmaf(F[r][s], G[s][j], acc), then acc = fmaf(F[r][32 + s], G[32 + s][j], acc) (the two lane halves
           hold the two halves of the row); out = acc, or float32(out_old + acc) with `accumulate`.

Arrays are float32 throughout; the fp64 references of the bound are formed from them."""
import fractions
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24                         # unit roundoff of fp32
NAN_BITS = 0x7FC00000                  # the quiet NaN the outputs and guards are filled with


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 fused multiply-add, correctly rounded
# ------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) element by element: the fp64 product of two fp32 numbers is exact (48 bits); TwoSum gives p + c = s + e exactly;
    s is moved to the neighbour with an odd last bit when e != 0 (round to odd at 53 bits), and the cast of that to fp32 rounds the
    exact sum once (53 >= 24 + 2).  A plain fp64 a * b + c followed by a cast rounds twice."""
    a, b, c = (np.asarray(x) for x in (a, b, c))
    assert a.dtype == F32 and b.dtype == F32 and c.dtype == F32
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = np.atleast_1d(p + c)
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return odd.astype(F32).reshape(p.shape)


def round_fraction_f32(x: fractions.Fraction) -> np.float32:
    """x rounded to the nearest fp32, ties to even, in integer arithmetic (normal and subnormal range; no overflow handling)"""
    if x == 0:
        return F32(0.0)
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()            # 2^(e-1) < |x| < 2^(e+1)
    if fractions.Fraction(n, d) < fractions.Fraction(2) ** e:
        e -= 1                                     # now 2^e <= |x| < 2^(e+1)
    q = fractions.Fraction(2) ** (max(e, -126) - 23)
    m = round(x / q)                               # Python rounds a Fraction half to even
    return F32(float(m * q))                       # m q has at most 24 bits: the conversions are exact


# ------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ------------------------------------------------------------------------------------------------------------------------------
def pairs_per(rows_pad, blocks):
    """(pairs, per): the row pairs of the launch and the pairs a wave owns"""
    assert rows_pad > 0 and rows_pad % 2 == 0 and 1 <= blocks <= 1024
    pairs, nwaves = rows_pad // 2, 4 * blocks
    return pairs, -(-pairs // nwaves)


def partition(rows_pad, blocks):
    """(pairs, per, [(p0, p1) per wave gw = 4 b + w]); an idle wave has p0 == p1"""
    pairs, per = pairs_per(rows_pad, blocks)
    ranges = []
    for gw in range(4 * blocks):
        p0 = gw * per
        ranges.append((p0, min(p0 + per, pairs)) if p0 < pairs else (p0, p0))
    return pairs, per, ranges


def describe(rows_pad, blocks):
    """what a (rows_pad, blocks) launch of gram_partial_kernel exercises, from the restated arithmetic: `trips` / `tail` are the trips
    of the 4-pair unrolled loop and of the tail loop in a full wave"""
    pairs, per, ranges = partition(rows_pad, blocks)
    counts = [p1 - p0 for p0, p1 in ranges]
    busy = [n > 0 for n in counts]
    busy_blocks = [any(busy[4 * b:4 * b + 4]) for b in range(blocks)]
    return dict(per=per, tail=per % 4, trips=per // 4, tail_only=per < 4,
                clipped=any(0 < n < per for n in counts),
                idle_wave_in_busy_block=any(busy_blocks[b] and not all(busy[4 * b:4 * b + 4]) for b in range(blocks)),
                idle_blocks=blocks - sum(busy_blocks))


def owner_block(row, rows_pad, blocks):
    """the slab that owns `row`"""
    return (row // 2) // pairs_per(rows_pad, blocks)[1] // 4


def block_rows(b, rows_pad, blocks):
    """the rows [r0, r1) of slab b (empty for an idle block)"""
    pairs, per = pairs_per(rows_pad, blocks)
    p0 = min(4 * b * per, pairs)
    return 2 * p0, 2 * min(p0 + 4 * per, pairs)


# name, rows_pad, blocks: bmf_gram_partial at kp = 32 (gram_partial_kernel<1>) and kp = 64 (<2>)
GRAM_CASES = [
    ("one_pair_three_idle_waves", 2, 1),
    ("tail_loop_only", 6, 1),
    ("per5_one_trip_tail1", 80, 2),
    ("per6_one_trip_tail2", 96, 2),
    ("per7_one_trip_tail3", 112, 2),
    ("per9_two_trips_clipped_last_wave", 134, 2),
    ("per4_partial_last_block", 130, 5),
    ("48_idle_blocks", 128, 64),
    ("per16_four_trips_no_tail", 384, 3),
    ("per46_eleven_trips_tail2", 2560, 7),
    ("960_idle_blocks", 512, 1024),
]
CROSS_ROWS = [2, 6, 130, 134, 512, 2560]       # bmf_gram_cross: every rows_pad with every blocks
CROSS_BLOCKS = [1, 3, 7, 1024]
FG_ROWS = [128, 384, 1664]                     # bmf_fg_f32: 1, 3 and 13 workgroups
BK = 64


# ------------------------------------------------------------------------------------------------------------------------------
# the chains
# ------------------------------------------------------------------------------------------------------------------------------
def slab_chain(A, B, rows_pad, blocks, kp):
    """slabs[blocks][kp][kp] of bmf_gram_cross(A, B) (kp = 64) or, with B = A, of bmf_gram_partial: the fmaf chains of all busy waves
    advanced together, one row at a time.  Columns at or beyond kp are not touched."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.dtype == F32 and B.dtype == F32 and A.shape[0] == rows_pad == B.shape[0]
    pairs, per = pairs_per(rows_pad, blocks)
    nbusy = -(-pairs // per)
    acc = np.zeros((nbusy, kp, kp), F32)
    for t in range(per):
        p = np.arange(nbusy) * per + t
        live = (p < pairs)[:, None, None]
        p = np.minimum(p, pairs - 1)
        for h in range(2):
            a, b = A[2 * p + h, :kp], B[2 * p + h, :kp]
            acc = np.where(live, fma32(a[:, :, None], b[:, None, :], acc), acc)
    nb = -(-nbusy // 4)
    w = np.zeros((4 * nb, kp, kp), F32)
    w[:nbusy] = acc
    w = w.reshape(nb, 4, kp, kp)
    slabs = np.zeros((blocks, kp, kp), F32)                      # +0.0 wherever no wave of the block owns a pair
    slabs[:nb] = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    return slabs


def fg_chain(F, G, out_old=None):
    """bmf_fg_f32: out[rows][64]; G is (64, ldg), columns at or beyond 64 are not touched; out_old != None is `accumulate`"""
    F, G = np.asarray(F), np.asarray(G)
    assert F.dtype == F32 and G.dtype == F32 and F.shape[1] == BK and G.shape[0] == BK
    acc = np.zeros((F.shape[0], BK), F32)
    for s in range(32):
        for k in (s, 32 + s):
            acc = fma32(F[:, k, None], G[None, k, :BK], acc)
    return acc if out_old is None else (np.asarray(out_old, F32) + acc).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------
# the bound (a diagnostic: it tells "another order" from "other numbers" when a bitwise gate fails)
# ------------------------------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1 - n * U)


def slab_roundings(rows_pad, blocks):
    """roundings on the path of a slab entry: two per pair of the wave chain, two for the sum of the four waves"""
    return 2 * pairs_per(rows_pad, blocks)[1] + 2


def slab_exact(A, B, rows_pad, blocks, kp):
    """(fp64 partial Gram of each busy slab's rows, the sum of |terms| of each), [busy_blocks][kp][kp]: the slabs behind them are idle
    and must be +0.0.  The fp64 sums themselves are good to rows 2^-53 of the second, which bound() adds."""
    A64, B64 = np.asarray(A)[:, :kp].astype(np.float64), np.asarray(B)[:, :kp].astype(np.float64)
    nb = blocks - describe(rows_pad, blocks)["idle_blocks"]
    want, mag = np.zeros((nb, kp, kp)), np.zeros((nb, kp, kp))
    for b in range(nb):
        r0, r1 = block_rows(b, rows_pad, blocks)
        assert r1 > r0
        want[b] = A64[r0:r1].T @ B64[r0:r1]
        mag[b] = np.abs(A64[r0:r1]).T @ np.abs(B64[r0:r1])
    return want, mag


def bound(n32, n64, mag):
    """gamma_n32 sum |terms| for the fp32 path plus n64 2^-53 sum |terms| for an fp64 reference of n64 additions"""
    return (gamma(n32) + n64 * 2.0 ** -53) * mag


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def column_exponents(n, rs):
    e = np.rint(np.linspace(-20, 10, n)).astype(np.int64)
    rs.shuffle(e)
    return e


def tracer_rows(rows_pad, blocks):
    """first and last row of the ranges of the waves 0, 1, 3, 4 and of the last two busy waves (the last one is the clipped one, the
    pairs 3 | 4 the seam between slab 0 and slab 1): at most eight distinct rows"""
    pairs, per, ranges = partition(rows_pad, blocks)
    nbusy = -(-pairs // per)
    rows = []
    for gw in (0, nbusy - 1, 3, 4, 1, nbusy - 2):
        if 0 <= gw < nbusy:
            p0, p1 = ranges[gw]
            for r in (2 * p0, 2 * p1 - 1):
                if r not in rows:
                    rows.append(r)
    return rows[:8]


ZERO_COL = 2


def tracer_cols(n, kp):
    return [(5 + 7 * t) % kp for t in range(n)]


def exact_ints(rows_pad, kp, blocks, seed):
    """(ints[rows_pad][kp] in [-7, 7], exponents[kp], tracers [(col, row)]): column ZERO_COL all zero; a tracer column has one
    non-zero, at its row"""
    rs = np.random.RandomState(seed)
    ints = rs.randint(-7, 8, size=(rows_pad, kp)).astype(np.int64)
    ints[:, ZERO_COL] = 0
    rows = tracer_rows(rows_pad, blocks)
    tracers = list(zip(tracer_cols(len(rows), kp), rows))
    for t, (c, r) in enumerate(tracers):
        ints[:, c] = 0
        ints[r, c] = (3 + t % 5) * (-1) ** t
    return ints, column_exponents(kp, rs), tracers


def with_padding_columns(core, ld):
    """core (rows, kp) as float32 in a (rows, ld) array whose further columns are NaN: a read of them poisons the result"""
    out = np.full((core.shape[0], ld), np.nan, F32)
    out[:, :core.shape[1]] = core
    return out


@functools.lru_cache(maxsize=None)
def exact_factor(rows_pad, kp, blocks, seed=1):
    """(F float32 (rows_pad, kp), ints, exponents, tracers): F = ints 2^e_c, so that every partial sum of every chain is an integer
    below 2^24 times 2^(e_i + e_j) -- representable, whatever the order"""
    ints, e, tracers = exact_ints(rows_pad, kp, blocks, seed)
    F = (ints * 2.0 ** e[None, :]).astype(F32)
    assert np.array_equal(F.astype(np.float64), ints * 2.0 ** e[None, :])
    F.setflags(write=False)
    return F, ints, e, tracers


def exact_slabs(intsA, eA, intsB, eB, rows_pad, blocks):
    """the integer partial Gram of each slab's rows, scaled: float32, exact"""
    kp = intsA.shape[1]
    out = np.zeros((blocks, kp, kp), np.float64)
    scale = 2.0 ** (eA[:, None] + eB[None, :])
    for b in range(blocks):
        r0, r1 = block_rows(b, rows_pad, blocks)
        if r1 > r0:
            n = intsA[r0:r1].T @ intsB[r0:r1]
            assert np.abs(n).max() < 2 ** 24
            out[b] = n * scale
    got = out.astype(F32)
    assert np.array_equal(got.astype(np.float64), out)
    return got


@functools.lru_cache(maxsize=None)
def mixed_factor(rows_pad, kp, seed=2):
    """normal deviates of both signs, per-column scales 10^U(-6, 3), the last min(37, rows_pad / 4) rows zero (the padding)"""
    rs = np.random.RandomState(seed)
    F = (rs.standard_normal((rows_pad, kp)) * 10.0 ** rs.uniform(-6, 3, kp)[None, :]).astype(F32)
    F[rows_pad - min(37, rows_pad // 4):] = 0
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def exact_fg(rows_pad, seed=3):
    """(F, G (64, 64), out_old, intsF, intsG, intsO, d): F[r][s] = intsF 2^e_s, G[s][j] = intsG 2^(d_j - e_s), out_old = intsO 2^d_j:
    every term and every partial of out[r][j] is a small integer times 2^d_j.  Column ZERO_COL of F and of G is zero."""
    rs = np.random.RandomState(seed + rows_pad)
    iF = rs.randint(-7, 8, size=(rows_pad, BK)).astype(np.int64)
    iG = rs.randint(-7, 8, size=(BK, BK)).astype(np.int64)
    iO = rs.randint(-7, 8, size=(rows_pad, BK)).astype(np.int64)
    iF[:, ZERO_COL] = 0
    iG[:, ZERO_COL] = 0
    e, d = column_exponents(BK, rs), column_exponents(BK, rs)
    F = (iF * 2.0 ** e[None, :]).astype(F32)
    G = (iG * 2.0 ** (d[None, :] - e[:, None])).astype(F32)
    O = (iO * 2.0 ** d[None, :]).astype(F32)
    assert np.array_equal(G.astype(np.float64), iG * 2.0 ** (d[None, :] - e[:, None]))
    for a in (F, G, O):
        a.setflags(write=False)
    return F, G, O, iF, iG, iO, d


@functools.lru_cache(maxsize=None)
def mixed_fg(rows_pad, seed=4):
    """(F, G (64, 64), out_old): the mixed factor, a G and an out_old of normal deviates with per-column scales 10^U(-6, 3)"""
    rs = np.random.RandomState(seed + rows_pad)
    F = mixed_factor(rows_pad, BK, seed + 100)
    G = (rs.standard_normal((BK, BK)) * 10.0 ** rs.uniform(-6, 3, BK)[None, :]).astype(F32)
    O = (rs.standard_normal((rows_pad, BK)) * 10.0 ** rs.uniform(-6, 3, BK)[None, :]).astype(F32)
    G.setflags(write=False)
    O.setflags(write=False)
    return F, G, O


# references shared by the tests that follow one another on one case (the largest hold 16 MiB of slabs: two are kept)
@functools.lru_cache(maxsize=2)
def gram_reference(kind, rows_pad, blocks, kp):
    """(F (rows_pad, kp), the slabs the device must give bit for bit, fp64 partial Grams, sums of |terms|, tracers)"""
    if kind == "exact":
        F, ints, e, tracers = exact_factor(rows_pad, kp, blocks)
        want = exact_slabs(ints, e, ints, e, rows_pad, blocks)
    else:
        F, tracers = mixed_factor(rows_pad, kp), []
        want = slab_chain(F, F, rows_pad, blocks, kp)
    ref64, mag = slab_exact(F, F, rows_pad, blocks, kp)
    want.setflags(write=False)
    return F, want, ref64, mag, tracers


@functools.lru_cache(maxsize=2)
def cross_reference(kind, rows_pad, blocks, same):
    """(A, B, slabs to the bit, fp64 partial products, sums of |terms|, tracers); B is A itself when `same`"""
    if kind == "exact":
        A, iA, eA, tracers = exact_factor(rows_pad, BK, blocks, 5)
        B, iB, eB, _ = (A, iA, eA, tracers) if same else exact_factor(rows_pad, BK, blocks, 6)
        want = exact_slabs(iA, eA, iB, eB, rows_pad, blocks)
    else:
        A, tracers = mixed_factor(rows_pad, BK, 7), []
        B = A if same else mixed_factor(rows_pad, BK, 8)
        want = slab_chain(A, B, rows_pad, blocks, BK)
    ref64, mag = slab_exact(A, B, rows_pad, blocks, BK)
    want.setflags(write=False)
    return A, B, want, ref64, mag, tracers


@functools.lru_cache(maxsize=2)
def fg_reference(kind, rows_pad, accumulate):
    """(F, G (64, 64), out_old, out to the bit, fp64 result, sum of |terms|)"""
    if kind == "exact":
        F, G, O, iF, iG, iO, d = exact_fg(rows_pad)
        n = iF @ iG + (iO if accumulate else 0)
        want = (n * 2.0 ** d[None, :]).astype(F32)
        assert np.abs(n).max() < 2 ** 24 and np.array_equal(want.astype(np.float64), n * 2.0 ** d[None, :])
    else:
        F, G, O = mixed_fg(rows_pad)
        want = fg_chain(F, G, O if accumulate else None)
    F64, G64, O64 = (a.astype(np.float64) for a in (F, G, O))
    ref64 = F64 @ G64 + (O64 if accumulate else 0.0)
    mag = np.abs(F64) @ np.abs(G64) + (np.abs(O64) if accumulate else 0.0)
    want.setflags(write=False)
    return F, G, O, want, ref64, mag
