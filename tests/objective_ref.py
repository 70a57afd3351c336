"""References and input makers for the dense objective sums: csrc/residual.hip (bmf_residual_sums, bmf_residual_sums_f32,
bmf_thresh_eval, bmf_thresh_transform, bmf_real_product), csrc/thresh64.hip (bmf_thresh_eval64), csrc/mae.hip (bmf_mae_sum, _ex,
_tiled) and csrc/resid_f32.hip (bmf_residual_sums_f32_tiled).  NumPy only; tests/test_objective_sums_cpu.py proves what is claimed
here, tests/test_objective_sums_gpu.py uses it against the kernels.

A reduction is tested cell by cell when every cell's term is EXACT and differs from its neighbours': then any cell that is dropped,
counted twice or paired with the wrong bit moves the sum, and the comparison is ==.  The exact inputs:

  U[i][l], V[j][l] in {0, 1/8, ..., 8/8}, at most four non-zeros per row (three hashed columns that depend on the row number and
  column k - 1), so   P[i][j] = sum_l U[i][l] V[j][l]  is a multiple of 2^-6 in [0, 4]  (at most 4 products, each <= 1),
  r = x - P a multiple of 2^-6 with |r| <= 4,  r^2 a multiple of 2^-12 with r^2 <= 16.
  * the factors have at most 4 significant bits: exact as fp16 (also times the MAE kernels' scale -2), as a bf16 hi part with a zero
    lo part, and as fp32; every product and every partial sum of a cell's products is a multiple of 2^-6 below 8: exact in fp32;
  * a lane's fp32 partial over c cells: sum |r| <= 4 c, a multiple of 2^-6 -> an integer below 2^8 c in units of 2^-6; the fmaf chain
    of squares <= 16 c in units of 2^-12 -> an integer below 2^16 c.  With c <= 64 (the MAE kernels; 16 for the residual and tiled
    kernels; the MAE kernels hold X_ONE |r| = 2 |r|, one more bit) everything stays below 2^24: exact in fp32 in ANY order;
  * the fp64 sums: integers below 2^16 cells in units of 2^-12, exact below 2^37 cells.
The X bits are a hash of (i, j) (density 5 / 16): no row, column or diagonal pattern that a shifted pairing could preserve."""
import functools

import numpy as np

CUS_MI355X = 256


# ------------------------------------------------------------------------------------------------------------------------------
# the launch arithmetic of the three launchers, restated (not imported): the GPU tests assert their paths from the library's own
# queries (bmf_residual_plan, bmf_mae_plan, bmf_residual_tiled_plan); these restatements are what the queries are checked against
# ------------------------------------------------------------------------------------------------------------------------------
def residual_plan(m, n):
    """(col_groups, tiles_per_group): row blocks of 128 x groups of 32-column tiles, about 1024 workgroups"""
    row_blocks, tiles = -(-m // 128), -(-n // 32)
    groups = max(1, min(-(-1024 // row_blocks), tiles))
    per = -(-tiles // groups)
    return -(-tiles // per), per


def mae_plan(m_pad, n_pad, cus=CUS_MI355X):
    """(groups, stages_per_group): row blocks of 256 x ranges of 64-column stages, about six workgroups per resident slot"""
    row_blocks, stages = m_pad // 256, n_pad // 64
    groups = max(1, min(-(-12 * cus // row_blocks), stages))
    per = -(-stages // groups)
    return -(-stages // per), per


def tiled_plan(m_pad, n_pad):
    """(splits, stages_per_split): row tiles of 64 x splits of 64-column stages, about 1024 workgroups, at least ~8 stages each"""
    tiles, stages = m_pad // 64, n_pad // 64
    splits = -(-1024 // tiles)
    if splits > stages // 8:
        splits = max(stages // 8, 1)
    per = -(-stages // splits)
    return -(-stages // per), per


# ------------------------------------------------------------------------------------------------------------------------------
# exact inputs
# ------------------------------------------------------------------------------------------------------------------------------
def exact_factor(rows, k, salt):
    """rows x k fp64, entries in {0, 1/8 .. 1}: three hashed columns per row and column k - 1, values that depend on the row"""
    F = np.zeros((rows, k))
    r = np.arange(rows, dtype=np.int64)
    for t in range(3):
        col = (r * (2 * t + 1) + (r // k) * t + t * t + salt) % k          # t = 0: every column in turn
        F[r, col] = ((r * (3 + 2 * t) + (r // 5) + salt + t) % 8 + 1) / 8.0
    F[r, k - 1] = ((r * 5 + (r // 3) + salt) % 8 + 1) / 8.0
    return F


_C1, _C2, _C3 = np.uint32(2654435761), np.uint32(2246822519), np.uint32(3266489917)


def x_block(i, j):
    """X[i][j] for index vectors i (rows) and j (columns): uint8 0 / 1, a 32-bit hash of the pair, density 5 / 16"""
    a = np.asarray(i).astype(np.uint32) * _C1
    b = np.asarray(j).astype(np.uint32) * _C2
    h = a[:, None] + b[None, :]
    h ^= h >> np.uint32(15)
    h *= _C3
    h ^= h >> np.uint32(13)
    return ((h >> np.uint32(28)) < np.uint32(5)).astype(np.uint8)


def pack_words(bits, ld):
    """rows x c uint8 bits -> rows x ld uint32 words (bit c of a row in word c // 32 at position c % 32), zero beyond c"""
    rows, c = bits.shape
    assert ld * 32 >= c
    b = np.zeros((rows, ld * 32), np.uint8)
    b[:, :c] = bits
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view(np.uint32)


def x_words(m, n, m_pad, ld, poison=False, chunk=2048):
    """The bits of the m x n hash matrix as m_pad x ld words; the padding (rows >= m, columns >= n) zero, or all ones (poison)"""
    out = np.full((m_pad, ld), 0xFFFFFFFF if poison else 0, np.uint32)
    j = np.arange(n)
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        blk = np.ones((b - a, ld * 32), np.uint8) if poison else np.zeros((b - a, ld * 32), np.uint8)
        blk[:, :n] = x_block(np.arange(a, b), j)
        out[a:b] = np.packbits(blk, axis=1, bitorder="little").view(np.uint32)
    return out


@functools.lru_cache(maxsize=2)
def xt_words(m, n, n_pad, ldt, chunk=2048):
    """The same matrix TRANSPOSED: n_pad x ldt words, row j holds X[:, j]; zero padding (shared, read-only)"""
    out = np.zeros((n_pad, ldt), np.uint32)
    i = np.arange(m)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        out[a:b] = pack_words(x_block(i, np.arange(a, b)).T, ldt)
    out.setflags(write=False)
    return out


def tile_bits(words):
    """bmf_tile_bits of a rows x ld word matrix (rows % 256 == 0, ld % 16 == 0): block (row / 256, word / 16) = 256 rows x 16 words,
    contiguous, blocks of one row tile after the other"""
    rows, ld = words.shape
    assert rows % 256 == 0 and ld % 16 == 0
    return np.ascontiguousarray(words.reshape(rows // 256, 256, ld // 16, 16).transpose(0, 2, 1, 3)).reshape(rows, ld)


def pad_factor(F, rows_pad, kp, dtype=np.float32, fill=0.0):
    """F (rows x k) inside rows_pad x kp: rows >= rows hold `fill` in ALL kp columns, columns >= k of the real rows hold 0"""
    out = np.full((rows_pad, kp), fill, dtype)
    out[:F.shape[0]] = 0
    out[:F.shape[0], :F.shape[1]] = F
    return out


def dense_sums(xfun, m, n, U, V, chunk=2048):
    """(sum |X - U V^T|, sum (X - U V^T)^2) over the m x n cells in fp64, rows in chunks; xfun(i, j) gives the cells of X"""
    U, V = np.asarray(U, np.float64)[:m], np.asarray(V, np.float64)[:n]
    j = np.arange(n)
    s_abs = s_sq = 0.0
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        R = xfun(np.arange(a, b), j).astype(np.float64) - U[a:b] @ V.T
        s_abs += float(np.abs(R).sum())
        s_sq += float((R * R).sum())
    return s_abs, s_sq


@functools.lru_cache(maxsize=8)
def exact_case(m, n, k):
    """Exact factors and the exact sums of the m x n hash matrix at rank k (shared, read-only)"""
    U, V = exact_factor(m, k, 1), exact_factor(n, k, 4)
    s_abs, s_sq = dense_sums(x_block, m, n, U, V)
    U.setflags(write=False)
    V.setflags(write=False)
    return dict(m=m, n=n, k=k, U=U, V=V, s_abs=s_abs, s_sq=s_sq)


def real_block(i, j):
    """An exact REAL-valued X for the fp32 kernels: multiples of 1/8 in [0, 1.875], a function of (i, j) (zero where the bit is 0)"""
    i, j = np.asarray(i), np.asarray(j)
    return x_block(i, j) * (((i[:, None] * 3 + j[None, :] * 5) % 15 + 1) / 8.0)


def real_x(m, n):
    return real_block(np.arange(m), np.arange(n))


@functools.lru_cache(maxsize=8)
def exact_real_case(m, n, k):
    """The factors of exact_case against the real-valued X: r = x - P is still a multiple of 2^-6 with |r| <= 4"""
    U, V = exact_factor(m, k, 1), exact_factor(n, k, 4)
    s_abs, s_sq = dense_sums(real_block, m, n, U, V)
    U.setflags(write=False)
    V.setflags(write=False)
    return dict(m=m, n=n, k=k, U=U, V=V, s_abs=s_abs, s_sq=s_sq)


def random_factor(rng, rows, k, scale=0.4):
    """real factors as the existing random tests draw them, rounded to fp32"""
    return (rng.random((rows, k)) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# the thresholding objective
# ------------------------------------------------------------------------------------------------------------------------------
def sigmoid_pair(Z, lam, dtype=np.longdouble):
    """s = sigmoid(z) and d = lam s (1 - s) (= lam exp(-z) s^2 of BinaryMFThreshold.py:211-227) from e = exp(-|z|): no overflow, no
    cancelling 1 - s"""
    Z = np.asarray(Z, dtype)
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(Z))
    pos = Z >= 0
    s = np.where(pos, 1 / (1 + e), e / (1 + e))
    d = lam * e / ((1 + e) * (1 + e))
    return s, d


def thresh_ref(X, U, V, u, v, lam, dtype=np.longdouble):
    """out[0..3] of bmf_thresh_eval / bmf_thresh_eval64 over the real cells, in `dtype`, and the transformed factors:
    sum |R|, sum R^2, sum R o (dUs Vs^T), sum R o (Us dVs^T) with R = X - Us Vs^T"""
    lam = dtype(lam)
    Us, dUs = sigmoid_pair((np.asarray(U, dtype) - dtype(u)) * lam, lam, dtype)
    Vs, dVs = sigmoid_pair((np.asarray(V, dtype) - dtype(v)) * lam, lam, dtype)
    R = np.asarray(X, dtype) - Us @ Vs.T
    out = np.array([np.abs(R).sum(), (R * R).sum(), (R * (dUs @ Vs.T)).sum(), (R * (Us @ dVs.T)).sum()], dtype)
    return out, (Us, dUs, Vs, dVs)


# Saturated inputs: with lam = 4 a factor entry x + 200 gives z = 800 -> e = exp(-800) = 0 -> s = 1, d = 0 exactly; x - 200 gives s = 0,
# d = 0; x itself gives s = 1/2, d = lam / 4 = 1.  The transformed factors are then in {0, 1/2, 1} and {0, 1}: every product, residual
# and sum of the objective AND of its gradient is a small dyadic number, exact in fp32 and fp64 in any order.
SAT_LAM, SAT_X = 4.0, 0.375


def sat_factor(rows, k, salt):
    """(F, S, D): rows x k inputs around SAT_X and the transform they must give: S = 1 where exact_factor has an even eighth, 1/2 where
    it has an odd one, 0 elsewhere"""
    q = np.rint(exact_factor(rows, k, salt) * 8).astype(np.int64)
    S = np.where(q == 0, 0.0, np.where(q % 2 == 0, 1.0, 0.5))
    F = SAT_X + 200.0 * np.where(q == 0, -1.0, np.where(q % 2 == 0, 1.0, 0.0))
    return F, S, np.where(S == 0.5, 1.0, 0.0)


@functools.lru_cache(maxsize=8)
def sat_case(m, n, k):
    """Saturated thresholding inputs over the hash matrix and the exact out[0..3] (fp64, exact: see above)"""
    U, Us, dUs = sat_factor(m, k, 2)
    V, Vs, dVs = sat_factor(n, k, 5)
    out = np.zeros(4)
    j = np.arange(n)
    for a in range(0, m, 2048):
        b = min(m, a + 2048)
        R = x_block(np.arange(a, b), j).astype(np.float64) - Us[a:b] @ Vs.T
        out += [np.abs(R).sum(), (R * R).sum(), (R * (dUs[a:b] @ Vs.T)).sum(), (R * (Us[a:b] @ dVs.T)).sum()]
    for a in (U, V, Us, dUs, Vs, dVs, out):
        a.setflags(write=False)
    return dict(m=m, n=n, k=k, U=U, V=V, Us=Us, dUs=dUs, Vs=Vs, dVs=dVs, out=out)


# z = lam (F - x) at the places where the transform can go wrong: 0, F - x = +-1e-300 (representable only around x = 0), where 1 - s starts to round to 0
# (37, 40), where exp over- / underflows (709, 800), and the nearest representable neighbours of x (a tie on each side of 0)
TRANSFORM_Z = [0.0, 37.0, -37.0, 40.0, -40.0, 709.0, -709.0, 800.0, -800.0]


def transform_inputs(x, lam, dtype):
    """factor entries that put z = lam (F - x) at TRANSFORM_Z (as nearly as `dtype` allows), F at x +- 1e-300 and at one ulp of x on
    each side"""
    x = dtype(x)
    vals = [x + dtype(z / lam) for z in TRANSFORM_Z] + [x + dtype(1e-300), x - dtype(1e-300)]
    vals += [np.nextafter(x, dtype(np.inf)), np.nextafter(x, dtype(-np.inf))]
    return np.array(vals, dtype)
