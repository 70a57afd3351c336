"""References and input makers for the real-valued WNMF kernels: csrc/xf_f32.hip (tile_f32_kernel, frag_f32_kernel, frag_rows_bf16_kernel,
frag_bf16x3_kernel, xf_f32_kernel<NT>, xf_f32_ring_kernel<NT>, xf_f32_bf3_ring_kernel, xf_f32_resid_ring_kernel<BF3>), frag_rows_f32_kernel
of csrc/resid_f32.hip and real_update_kernel of csrc/wnmf_real.hip.  NumPy only; tests/test_real_kernels_cpu.py proves what is claimed here,
tests/test_real_kernels_gpu.py uses it against the kernels.

The re-ordering kernels are restated from the formulas of include/bmf_hip.h and of the kernels' header comments as SOURCE MAPS: `src[i]` is
the flat index of the input element that output element i holds.  A contraction is tested slab by slab on inputs whose every product
and every partial sum is exact in fp32 in ANY order:

  A = objective_ref.real_x: multiples of 1/8 in [0, 1.875], 11/16 of the cells zero;
  F = dense_factor: every entry in {1..8}/8, hashed from (row, column), column j multiplied by (-1)^j.
  * a product is a multiple of 2^-6 of magnitude <= 1.875 = 120 units; the terms of one output column share a sign, so every partial sum
    of any subset in any order is an integer of magnitude <= 120 * len units, below 2^24 for reductions below 139 000: exact in fp32;
  * values of at most 4 significant bits are their own bf16 hi part: on the three-way split path mid = lo = 0 and the one surviving
    product hi * hi is the fp32 product;
  * a dense factor leaves no stage partial of a real (row, column) zero (proved for the shapes used), so a slab that took a stage of
    its neighbour, dropped one or counted one twice differs from the exact slab.
The fused residual sums use objective_ref.exact_real_case unchanged: |r| <= 4, 16 cells per lane and stage (proved there)."""
import functools

import numpy as np

import objective_ref as R
from test_mu_epilogue_cpu import bf16_addends


# ------------------------------------------------------------------------------------------------------------------------------
# the orders, as source maps
# ------------------------------------------------------------------------------------------------------------------------------
def tile_src(rows_pad, red, lda):
    """bmf_tile_f32: tiled[((((tile * (red / 64) + st) * 4 + q) * 32 + rl) * 8 + c) * 4 + e]
    = X[(64 tile + 32 rw + rl) * lda + 64 st + 32 kh + 4 (c ^ ((rl >> 1) & 7)) + e],  q = 2 kh + rw"""
    assert rows_pad % 64 == 0 and red % 64 == 0 and lda >= red
    i = np.arange(rows_pad * red, dtype=np.int64)
    e, c, rl, q, blk = i & 3, (i >> 2) & 7, (i >> 5) & 31, (i >> 10) & 3, i >> 12
    rw, kh = q & 1, q >> 1
    tile, st = blk // (red // 64), blk % (red // 64)
    return (64 * tile + 32 * rw + rl) * lda + 64 * st + 32 * kh + 4 * (c ^ ((rl >> 1) & 7)) + e


def frag_src(rows_pad, kp):
    """bmf_frag_f32: frag[((((st * 2 + kh) * 4 + u) * NT + nt) * 64 + 32 h + r) * 4 + t] = F[(64 st + 32 kh + 8 u + 4 h + t) * kp + 32 nt + r]"""
    assert rows_pad % 64 == 0 and kp % 32 == 0
    NT = kp // 32
    i = np.arange(rows_pad * kp, dtype=np.int64)
    t, r, h, g = i & 3, (i >> 2) & 31, (i >> 7) & 1, i >> 8
    nt, g2 = g % NT, g // NT
    u, kh, st = g2 & 3, (g2 >> 2) & 1, g2 >> 3
    return (64 * st + 32 * kh + 8 * u + 4 * h + t) * kp + 32 * nt + r


def frag_rows_src(rows_pad, kp):
    """bmf_frag_rows_f32: frag[(((st * 2 + cw) * (kp / 8) + q) * 64 + 32 h + r) * 4 + t] = V[(64 st + 32 cw + r) * kp + (kp / 2) h + 4 q + t]"""
    assert rows_pad % 64 == 0 and kp % 32 == 0
    VL = kp // 8
    i = np.arange(rows_pad * kp, dtype=np.int64)
    t, r, h, g = i & 3, (i >> 2) & 31, (i >> 7) & 1, i >> 8
    q, g2 = g % VL, g // VL
    cw, st = g2 & 1, g2 >> 1
    return (64 * st + 32 * cw + r) * kp + (kp // 2) * h + 4 * q + t


def frag_rows_bf16_src(rows_pad):
    """bmf_frag_rows_bf16 (kp = 32), per 16-bit half: half b of word
    frag[(((st * 2 + kh) * 4 + q) * 64 + 32 h + r) * 4 + w],  q = 2 ks + (0: hi, 1: lo),
    is addend q & 1 of F[64 st + 32 kh + r][16 ks + 8 h + 2 w + b].  Returns (addend, src), each rows_pad * 64 long."""
    assert rows_pad % 64 == 0
    i = np.arange(rows_pad * 64, dtype=np.int64)
    b, w, r, h, g = i & 1, (i >> 1) & 3, (i >> 3) & 31, (i >> 8) & 1, i >> 9
    q, kh, st = g & 3, (g >> 2) & 1, g >> 3
    return q & 1, (64 * st + 32 * kh + r) * 32 + 16 * (q >> 1) + 8 * h + 2 * w + b


def frag_bf16x3_src(rows_pad):
    """bmf_frag_bf16x3, per 16-bit half: half b of word frag3[(((st * 2 + kh) * 2 + ks) * 3 + part) * 256 + lane * 4 + w] is addend
    `part` (hi / mid / lo) of element j = 2 w + b of the k-step: F[64 st + 32 kh + 8 (2 ks + (j >> 2)) + 4 h + (j & 3)][r], lane = 32 h + r.
    Returns (part, src), each rows_pad * 96 long."""
    assert rows_pad % 64 == 0
    i = np.arange(rows_pad * 96, dtype=np.int64)
    j, r, h, g = i & 7, (i >> 3) & 31, (i >> 8) & 1, i >> 9
    part, g2 = g % 3, g // 3
    ks, kh, st = g2 & 1, (g2 >> 1) & 1, g2 >> 2
    return part, (64 * st + 32 * kh + 8 * (2 * ks + (j >> 2)) + 4 * h + (j & 3)) * 32 + r


def inverse(src, size=None):
    """where each input element lands: inv[src[i]] = i, -1 for input elements no output holds (the slack of a leading dimension)"""
    inv = np.full(size if size is not None else src.size, -1, np.int64)
    inv[src] = np.arange(src.size)
    return inv


# ------------------------------------------------------------------------------------------------------------------------------
# the bf16 splits
# ------------------------------------------------------------------------------------------------------------------------------
def as_f32(bits16):
    """the fp32 value of bf16 bit patterns"""
    return (np.asarray(bits16).astype(np.uint32) << 16).view(np.float32)


def split2_rne(F32):
    """(hi, lo) uint16: hi the round-to-nearest-even bf16 of x, lo the round-to-nearest-even bf16 of the fp32 remainder x - hi"""
    b = bf16_addends(np.ascontiguousarray(F32, np.float32), 2)
    return b[0], b[1]


def split3_trunc(F32):
    """(hi, mid, lo) uint16 of bmf_split3_bf16: each addend the top 16 bits of what the earlier ones left, hi + mid + lo == x exactly"""
    x = np.ascontiguousarray(F32, np.float32)
    hi = (x.view(np.uint32) >> 16).astype(np.uint16)
    r1 = x - as_f32(hi)
    mid = (r1.view(np.uint32) >> 16).astype(np.uint16)
    r2 = r1 - as_f32(mid)
    return hi, mid, (r2.view(np.uint32) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------------
# the orders applied (what the kernels must write, and the operands the contraction tests hand to the kernels)
# ------------------------------------------------------------------------------------------------------------------------------
def tile_f32(X, red):
    """bmf_tile_f32 of X (rows_pad x lda, lda >= red)"""
    X = np.ascontiguousarray(X, np.float32)
    return X.ravel()[tile_src(X.shape[0], red, X.shape[1])]


def frag_f32(F):
    F = np.ascontiguousarray(F, np.float32)
    return F.ravel()[frag_src(*F.shape)]


def frag_rows_f32(V):
    V = np.ascontiguousarray(V, np.float32)
    return V.ravel()[frag_rows_src(*V.shape)]


def words(halves16):
    """pairs of 16-bit halves (low half first) as uint32 words"""
    return np.ascontiguousarray(halves16, np.uint16).view(np.uint32)


def frag_rows_bf16(F):
    F = np.ascontiguousarray(F, np.float32)
    assert F.shape[1] == 32
    addend, src = frag_rows_bf16_src(F.shape[0])
    return words(np.stack(split2_rne(F)).reshape(2, -1)[addend, src])


def frag_bf16x3(F):
    F = np.ascontiguousarray(F, np.float32)
    assert F.shape[1] == 32
    part, src = frag_bf16x3_src(F.shape[0])
    return words(np.stack(split3_trunc(F)).reshape(3, -1)[part, src])


def position_coded(rows, cols):
    """every element a distinct integer below 2^24: its own flat index + 1"""
    assert rows * cols < 2 ** 24
    return (np.arange(rows * cols, dtype=np.float32) + 1).reshape(rows, cols)


def bf16_value_inputs(rows_pad, seed):
    """rows_pad x 32 fp32 for the two bf16 orders: full 24-bit mantissas at magnitudes 2^-20 .. 2^20 of either sign, and planted in
    hashed places: +0 and -0, powers of two, exact bf16 ties (low 16 bits 0x8000) under an even and under an odd bf16 mantissa, the
    largest mantissa (rounds up into the next binade)"""
    rng = np.random.default_rng([41, rows_pad, seed])
    n = rows_pad * 32
    bits = rng.integers(0, 1 << 23, n, dtype=np.uint32) | (rng.integers(127 - 20, 127 + 21, n, dtype=np.uint32) << 23)
    bits |= rng.integers(0, 2, n, dtype=np.uint32) << 31
    kind = (np.arange(n) * 7 + np.arange(n) // 32) % 16
    bits[kind == 1] &= np.uint32(0x80000000)                                                     # +-0
    bits[kind == 2] &= np.uint32(0xFF800000)                                                     # +-2^e
    bits[kind == 3] = (bits[kind == 3] & np.uint32(0xFFFE0000)) | np.uint32(0x8000)              # a tie under an even mantissa: down
    bits[kind == 4] = (bits[kind == 4] & np.uint32(0xFFFE0000)) | np.uint32(0x18000)             # a tie under an odd one: up
    bits[kind == 5] |= np.uint32(0x007FFFFF)                                                     # rounds up into the next binade
    return bits.view(np.float32).reshape(rows_pad, 32)


# ------------------------------------------------------------------------------------------------------------------------------
# exact contractions
# ------------------------------------------------------------------------------------------------------------------------------
def dense_factor(rows, k):
    """rows x k fp64: |F[i][j]| in {1..8}/8 from a hash of (i, j), the sign (-1)^j"""
    a = np.arange(rows).astype(np.uint32) * R._C2
    b = np.arange(k).astype(np.uint32) * R._C1
    h = a[:, None] + b[None, :]
    h ^= h >> np.uint32(15)
    h *= R._C3
    h ^= h >> np.uint32(13)
    return ((h >> np.uint32(29)).astype(np.float64) + 1) / 8.0 * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)[None, :]


def slab_ranges(units, splits):
    """the launchers' split of `units` stages (of 64) or groups (of 8): [(first, end)] per slab, empty ranges where the units run out"""
    per = -(-units // splits)
    return [(min(s * per, units), min((s + 1) * per, units)) for s in range(splits)]


def slab_products(A, F, ranges, unit):
    """[slab][rows_pad][kp] fp64: A[:, range] @ F[range] for each slab's range of reduction indices (exact on the exact inputs)"""
    A, F = np.asarray(A, np.float64), np.asarray(F, np.float64)
    return np.stack([A[:, a * unit:b * unit] @ F[a * unit:b * unit] for a, b in ranges])


@functools.lru_cache(maxsize=64)
def contraction_case(rows_pad, red, k, kp):
    """Exact A (rows_pad x red, the last 3 rows and the last 5 reduction indices zero padding) and dense F (red x kp), fp32, read-only"""
    rows, real = rows_pad - 3, max(red - 5, 1)
    A = np.zeros((rows_pad, red), np.float32)
    A[:rows, :real] = R.real_x(rows, real)
    F = R.pad_factor(dense_factor(real, k), red, kp)
    A.setflags(write=False)
    F.setflags(write=False)
    return dict(rows=rows, real=real, A=A, F=F)


@functools.lru_cache(maxsize=64)
def residual_case(rows_pad, red, k):
    """The fused pass on objective_ref.exact_real_case: A = real_x (rows x real inside rows_pad x red), F = the case's V (red x 32: the
    contracted factor), G = its U (rows_pad x 32: one row per row of A); the exact sums of A - G F^T"""
    rows, real = rows_pad - 3, max(red - 5, 1)
    c = R.exact_real_case(rows, real, k)
    A = np.zeros((rows_pad, red), np.float32)
    A[:rows, :real] = R.real_x(rows, real)
    F, G = R.pad_factor(c["V"], red, 32), R.pad_factor(c["U"], rows_pad, 32)
    for a in (A, F, G):
        a.setflags(write=False)
    return dict(rows=rows, real=real, A=A, F=F, G=G, s_abs=c["s_abs"], s_sq=c["s_sq"])


# ------------------------------------------------------------------------------------------------------------------------------
# the six-product contraction on three-way split operands, emulated
# ------------------------------------------------------------------------------------------------------------------------------
BF3_PRODUCTS = [("lo", "hi"), ("mid", "mid"), ("hi", "lo"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi")]     # (A part, F part), the kernel's order


def bf3_contraction(A, F, drop=None):
    """sum over BF3_PRODUCTS (without `drop`) of A_part @ F_part in fp64: what the bf16 x 3 kernels compute up to their fp32 accumulation"""
    pa = dict(zip(("hi", "mid", "lo"), (as_f32(p).astype(np.float64) for p in split3_trunc(A))))
    pf = dict(zip(("hi", "mid", "lo"), (as_f32(p).astype(np.float64) for p in split3_trunc(F))))
    return sum(pa[x] @ pf[y] for x, y in BF3_PRODUCTS if (x, y) != drop)


@functools.lru_cache(maxsize=4)
def general_case(rows_pad, red, k, kp=32):
    """Non-negative random fp32 A, F (red x kp) and G (rows_pad x 32, its first min(k, 32) columns), as WNMF's are; zero padding as in
    contraction_case"""
    rows, real = rows_pad - 3, red - 5
    rng = np.random.default_rng([43, rows_pad, red, k])
    A = np.zeros((rows_pad, red), np.float32)
    A[:rows, :real] = rng.random((rows, real), dtype=np.float32)
    F, G = R.pad_factor(R.random_factor(rng, real, k, 1.0), red, kp), R.pad_factor(R.random_factor(rng, rows, min(k, 32)), rows_pad, 32)
    for a in (A, F, G):
        a.setflags(write=False)
    return dict(rows=rows, real=real, A=A, F=F, G=G)
