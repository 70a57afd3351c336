"""Plain NumPy fp64 restatements of the dense link family of csrc/link.hip -- the tile-fused pass (bmf_link_pass, bmf_link_pass16), the
scalar sums (bmf_link_sums, bmf_link_sums16), the operand split (bmf_link_split, bmf_link_split_pair, restated BIT FOR BIT) and the
column sums (bmf_colsum_fill) -- together with the launch arithmetic of those entry points (restated, not imported), the input makers,
the case tables and the error bounds that tests/test_link_kernels_cpu.py (which pins all of this to the oracle) and
tests/test_link_kernels_gpu.py share.

X is a dense 0/1 array; the factors are the ones the kernel sees (fp32 values held in float64).  One orientation is (X, F_self, F_other)
with rows of X = rows of F_self; the other one is (X.T, F_other, F_self)."""
import functools
import math

import numpy as np

LINK_SIGMOID, LINK_KL = 1, 2          # BMF_LINK_SIGMOID, BMF_LINK_KL of include/bmf_hip.h
KL_P_FLOOR = 1e-37                     # RULE kl_floor: the KL objective takes log(max(p, 1e-37))


# ------------------------------------------------------------------------------------------------------------------------------
# element-wise link terms
# ------------------------------------------------------------------------------------------------------------------------------
def sigmoid_parts(S):
    """sig = sigmoid(S) and d = sig (1 - sig) as e / (1 + e)^2 with e = exp(-|S|): no cancellation in either tail (sig (1 - sig) formed
    in fp64 is 0 beyond S ~ 37, d is not)."""
    S = np.asarray(S, dtype=np.float64)
    e = np.exp(-np.abs(S))
    r = 1.0 / (1.0 + e)
    return np.where(S >= 0, r, e * r), e * r * r


def link_cells(X, Fs, Fo, link, lam):
    """(P, f, g1, g2): the product, the prediction f (sigmoid(lam (P - 1/2)), or P itself for KL) and the cell weights of the two
    contractions, num = g1 @ Fo and den = g2 @ Fo (g2 is None for KL)."""
    X, Fs, Fo = (np.asarray(a, dtype=np.float64) for a in (X, Fs, Fo))
    P = Fs @ Fo.T
    if link == LINK_SIGMOID:
        sig, d = sigmoid_parts(lam * (P - 0.5))
        return P, sig, lam * X * d, lam * sig * d
    assert link == LINK_KL
    # RULE kl_zero_product: a cell with p <= 0 adds nothing to num.  This is the kernels' rule (link_pass_kernel: `p > 0 ? rcp(p) : 0`).
    # The oracle has no such rule: wnmf_kl_update divides, so x / 0 is inf (x = 1) or nan (x = 0) there; its fit loop never gets that
    # far because zeros_to_eps replaces every zero of the factors first.  The pin in test_link_kernels_cpu.py therefore uses p > 0.
    inv = np.zeros_like(P)
    pos = P > 0
    inv[pos] = 1.0 / P[pos]
    return P, P, X * inv, None


def pass_ref(X, Fs, Fo, link, lam):
    """(num, den) of one pass; den is None for KL (there it is the column-sum vector of Fo, colsum_ref)."""
    _, _, g1, g2 = link_cells(X, Fs, Fo, link, lam)
    Fo = np.asarray(Fo, dtype=np.float64)
    return g1 @ Fo, None if g2 is None else g2 @ Fo


def kl_cells(X, P):
    """x log(x / p) - x + p per cell of a 0/1 X.  RULE zero_log_zero: the cells with x = 0 give p (0 log 0 = 0); RULE kl_floor: the
    others p - 1 - log(max(p, 1e-37))."""
    X, P = np.asarray(X, dtype=np.float64), np.asarray(P, dtype=np.float64)
    return np.where(X != 0, P - 1.0 - np.log(np.maximum(P, KL_P_FLOOR)), P)


def wide_sum(a) -> float:
    """the sum of the fp64 terms accumulated in long double (pairwise): at worst a few 1e-16 of sum |a|, far inside every gate here, and
    quick on half a million cells where math.fsum is not"""
    return float(np.sum(np.asarray(a, dtype=np.float64), dtype=np.longdouble))


def sums_ref(X, U, V, link, lam, O=None):
    """[sum |x - f|, sum (x - f)^2, sum over the observed cells of the KL term (0 for the sigmoid link)].  O (0/1, None = every cell)
    restricts the THIRD sum only: the first two are whole-matrix scores whatever the mask."""
    X = np.asarray(X, dtype=np.float64)
    P, f, _, _ = link_cells(X, U, V, link, lam)
    r = X - f
    s2 = 0.0
    if link == LINK_KL:
        t = kl_cells(X, P)
        s2 = wide_sum(t if O is None else t[np.asarray(O) != 0])
    return np.array([wide_sum(np.abs(r)), wide_sum(r * r), s2])


def colsum_ref(F) -> np.ndarray:
    """column sums, each one math.fsum of its column (correctly rounded fp64)"""
    F = np.asarray(F, dtype=np.float64)
    return np.array([math.fsum(F[:, c].tolist()) for c in range(F.shape[1])])


# ------------------------------------------------------------------------------------------------------------------------------
# the split workspace, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x) -> np.ndarray:
    """float32 -> bfloat16 bits, round to nearest even (bf16_bits of csrc/common.h, restated: add 0x7fff plus the bit that would become
    the last kept one, keep the upper half).  Finite inputs only."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_value(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def link_jr(reg, h):
    """the row (of a 32-row block) that register `reg` of half-wave h holds in the 32 x 32 MFMA's C/D layout"""
    return (reg & 3) + 8 * (reg >> 2) + 4 * h


def perm_rows(rows_pad) -> np.ndarray:
    """src[jb, q, h, t] = the row of F that position t of k-chunk q, half h, of 32-row block jb holds: jb * 32 + link_jr(8 q + t, h)"""
    assert rows_pad % 32 == 0
    jb, q, h, t = np.meshgrid(np.arange(rows_pad // 32), np.arange(2), np.arange(2), np.arange(8), indexing="ij")
    return jb * 32 + link_jr(8 * q + t, h)


def column_maxima(F) -> np.ndarray:
    """max |F| per column as float32; link_colmax_kernel leaves 0 where the maximum is 0 (or not below 3e38)"""
    m = np.abs(np.asarray(F, dtype=np.float32)).max(axis=0)
    return np.where(m < np.float32(3.0e38), m, np.float32(0)).astype(np.float32)


def pair_scales(A, B):
    """(S, T, invC) of link_pair_scales_kernel: with a_k < 2^ea_k, b_k < 2^eb_k the column maxima (frexp exponents), a column pair is
    live when both are positive; S_k = 2^(15 - ea_k), M = max over the live pairs of ea_k + eb_k, T_k = 2^(15 - M + ea_k), so that
    S_k T_k = C = 2^(30 - M) for every live k; 1 / C = 2^(M - 30) (1 when no pair is live).  RULE dead_column: a pair that is not
    live gets scale 0 in both factors."""
    a, b = column_maxima(A), column_maxima(B)
    live = (a > 0) & (b > 0)
    ea, eb = np.frexp(a)[1].astype(np.int64), np.frexp(b)[1].astype(np.int64)
    if not live.any():
        z = np.zeros(a.shape, np.float32)
        return z, z.copy(), np.float32(1.0)
    M = int((ea + eb)[live].max())
    S = np.where(live, np.ldexp(1.0, 15 - ea), 0.0).astype(np.float32)
    T = np.where(live, np.ldexp(1.0, 15 - M + ea), 0.0).astype(np.float32)
    return S, T, np.float32(np.ldexp(1.0, M - 30))


def single_scale(F) -> np.float32:
    """the one scale of bmf_link_split: S = 2^(15 - ex) with max |F| = m 2^ex, m in [0.5, 1); 1 for an all-zero factor"""
    mx = np.abs(np.asarray(F, dtype=np.float32)).max()
    if not (mx > 0) or not (mx < np.float32(3.0e38)):
        return np.float32(1.0)
    return np.float32(np.ldexp(1.0, 15 - int(np.frexp(mx)[1])))


def split_words(F, scale) -> dict:
    """The four data arrays of a workspace as uint16 words: `hi`, `lo` = f16(F s), f16(F s - hi), row-major; `ph`, `pl` = bf16(F),
    bf16(F - ph) in the order [32-row block][q][h][kk][t].  `scale`: one float32 or one per column."""
    F = np.ascontiguousarray(F, dtype=np.float32)
    rows_pad, kp = F.shape
    fs = F * np.asarray(scale, dtype=np.float32)             # a power of two (or 0): exact
    assert fs.dtype == np.float32
    hi = fs.astype(np.float16)
    lo = (fs - hi.astype(np.float32)).astype(np.float16)     # the difference is exact in fp32
    bh = bf16_bits(F)
    bl = bf16_bits(F - bf16_value(bh))
    src = perm_rows(rows_pad)                                # [jb, q, h, t]
    perm = lambda w: np.ascontiguousarray(w[src].transpose(0, 1, 2, 4, 3)).ravel()      # [jb, q, h, t, kk] -> [jb, q, h, kk, t]
    return dict(hi=hi.view(np.uint16).ravel(), lo=lo.view(np.uint16).ravel(), ph=perm(bh), pl=perm(bl))


def f32_word(x) -> np.uint32:
    return np.array([x], dtype=np.float32).view(np.uint32)[0]


def pair_headers(A, B):
    """the first 4 + 2 kp words of the third array of each workspace after bmf_link_split_pair: {1.0f, this factor's share of 1 / C,
    0, 0}, the column-maximum bits, the column scales"""
    S, T, invC = pair_scales(A, B)
    out = []
    for F, sc, share in ((A, S, invC), (B, T, np.float32(1.0))):
        head = np.array([f32_word(1.0), f32_word(share), 0, 0], dtype=np.uint32)
        out.append(np.concatenate([head, column_maxima(F).view(np.uint32), sc.view(np.uint32)]))
    return out[0], out[1], S, T


def single_header(F):
    """the first four words of the third array after bmf_link_split: {S, 1 / S, bits of max |F|, 0}"""
    S = single_scale(F)
    mx = np.abs(np.asarray(F, dtype=np.float32)).max()
    return np.array([f32_word(S), f32_word(np.float32(1.0) / S), f32_word(mx) if mx > 0 else 0, 0], dtype=np.uint32), S


def split_values(words, kp, scale):
    """what the kernels read back from split_words: (the fp16 pair as (hi + lo) / s, the bf16 pair hi + lo un-permuted), float64; columns
    with scale 0 come back as 0"""
    n = words["hi"].size
    rows_pad = n // kp
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64), (kp,)) if np.ndim(scale) else np.full(kp, float(scale))
    v16 = words["hi"].view(np.float16).astype(np.float64).reshape(rows_pad, kp) + words["lo"].view(np.float16).astype(np.float64).reshape(rows_pad, kp)
    with np.errstate(divide="ignore", invalid="ignore"):
        v16 = np.where(s > 0, v16 / s, 0.0)
    src = perm_rows(rows_pad)
    vb = np.zeros((rows_pad, kp))
    pv = (bf16_value(words["ph"]).astype(np.float64) + bf16_value(words["pl"]).astype(np.float64)).reshape(rows_pad // 32, 2, 2, kp, 8)
    vb[src] = pv.transpose(0, 1, 2, 4, 3)
    return v16, vb


# ------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic, restated
# ------------------------------------------------------------------------------------------------------------------------------
def splits_for(rows, cols) -> int:
    """bmf_link_splits: workgroups = row blocks of 128 x splits, 512 resident; at most one split per 8 column tiles and 16 in all; a split
    count that would leave a slab empty is skipped; the fewest splits whose last round of 512 is at least 90 % full, else the fullest"""
    row_blocks, col_tiles = (rows + 127) // 128, (cols + 31) // 32
    smax = min(max(col_tiles // 8, 1), 16)
    best, best_fill = 1, 0.0
    for s in range(1, smax + 1):
        per = -(-col_tiles // s)
        if -(-col_tiles // per) != s:
            continue
        wgs = row_blocks * s
        fill = wgs / (-(-wgs // 512) * 512)
        if fill >= 0.9:
            return s
        if fill > best_fill:
            best, best_fill = s, fill
    return best


def pass_plan(rows, cols) -> dict:
    """what one launch of the pass does with (rows, cols): row blocks of 128, column tiles of 32, the slabs and their tile counts, where
    the last valid row sits in its block and how many columns of the last tile are valid"""
    col_tiles, splits = (cols + 31) // 32, splits_for(rows, cols)
    per = -(-col_tiles // splits)
    slabs = [min(per, col_tiles - s * per) for s in range(splits)]
    assert all(t > 0 for t in slabs) and sum(slabs) == col_tiles
    return dict(row_blocks=(rows + 127) // 128, col_tiles=col_tiles, splits=splits, per=per, slabs=slabs, last_row_pos=(rows - 1) % 128,
                ragged=cols - 32 * (col_tiles - 1))


def colsum_blocks(rows, out_rows):
    """(partial blocks, rows per block) of bmf_colsum_fill, or None where it refuses: one block per 64 rows, at most 512, at most
    out_rows / 2 (their fp64 partials live in the head of `out`), at least 1; then the rows are spread evenly"""
    pb = min((rows + 63) // 64, 512, out_rows // 2)
    pb = max(pb, 1)
    rpb = -(-rows // pb)
    pb = -(-rows // rpb)
    if not (pb * 2 <= out_rows or (pb == 1 and out_rows >= 2)):
        return None
    return pb, rpb


# ------------------------------------------------------------------------------------------------------------------------------
# error bounds, every term named.  u = 2^-24 is the unit roundoff of fp32.
# ------------------------------------------------------------------------------------------------------------------------------
FP32_RTOL, FP32_ATOL = 2e-5, 1e-6      # the project's gate for these quantities from the fp32 kernels (tests/test_link_gpu.py)
U32 = 2.0 ** -24
P_REL = 2.0 ** -22          # include/bmf_hip.h: P from the fp16 hi / lo pairs is right to 2^-22 relative to sum_k colmaxU_k colmaxV_k
S_ARITH = 4 * U32           # s = fma(p, c1, c0) in fp32: c1 = -lam log2(e) / C carries three roundings, the fma one more, each relative to
                            # lam (|p| + 1/2) at most
FUN_D = 5 * 2.0 ** -23      # d = (e r) r with e = exp2(t) (1 ulp), 1 + e (u), r = rcp (1 ulp, used twice), two products (u each)
FUN_SD = 7 * 2.0 ** -23     # sig d = r d: r once more (1 ulp + u) and one more product (u)
FUN_SIG = 2.0 ** -22        # sig = rcp(1 + exp2(t)): 1 ulp + u + 1 ulp
FUN_RCP = 2.0 ** -23        # 1 / p = rcp(p / C): the scale is a power of two, the reciprocal 1 ulp
PROD = 3 * 2.0 ** -16       # a contraction product g F from two bf16 addends per operand: bf16 keeps 8 significant bits, so hi is right to
                            # 2^-8 and hi + lo to 2^-16 -- once for g, once for F -- and the product lo lo' that is left out is at most
                            # 2^-8 2^-8 of g F: three terms of 2^-16.  (First written as 2^-16 in all, after the header's "2^-16 per
                            # product"; the single-term KL rows of the 97 x 1 case came out at 1.4 x 2^-16: the derivation was short of
                            # two of its three terms, the kernel does what its formats allow.)
OUT = U32                   # the final lam * acc in fp32; the slabs are added in fp64
CLAMP = 2.0 ** -100         # sigmoid_cell clamps e at 2^100: where exp(-s) is larger, d comes out as 2^-100 instead of something smaller,
                            # and where e underflows d comes out as 0: an absolute error of at most 2^-100 per cell
TILE_ACC = 18 * U32         # sums kernels: a lane adds its 16 cells of a tile in fp32 (16 u), r = x - f and r^2 are rounded (2 u); the
                            # tile sums are then added in fp64


def product_scale(Fs, Fo) -> float:
    """sum_k colmax|Fs|_k colmax|Fo|_k: what P's 2^-22 is relative to"""
    return float((np.abs(np.asarray(Fs, dtype=np.float64)).max(axis=0) * np.abs(np.asarray(Fo, dtype=np.float64)).max(axis=0)).sum())


def pass16_bound(X, Fs, Fo, link, lam, n_acc):
    """Element-wise bound on |num - pass_ref| and |den - pass_ref| for bmf_link_pass16, same shapes as num / den.

      dP      = P_REL * product_scale                         the error of P
      ds      = lam (dP + S_ARITH (|P| + 1/2))                carried into s = lam (P - 1/2), plus the fp32 evaluation of s
      d       : |log d|' = |1 - 2 sig| <= 1, so d(s + ds) is within a factor exp(ds) of d(s): relative expm1(ds)
      sig d   : |log (sig d)|' = |2 - 3 sig| <= 2: relative expm1(2 ds)
      1 / p   : relative (dP / P) / (1 - dP / P)              (KL; the cases keep dP / P below 1/2, asserted here)
      + FUN_* the evaluation of the function in fp32, + PROD the 16-bit contraction product, + OUT the last scaling,
      + n_acc u: the fp32 accumulation -- n_acc roundings of a partial sum that is at most the sum of the |terms|; n_acc = 3 products
        per column of the sweep (pass_acc), or 0 for a row with a single term
      + the floor lam CLAMP sum_j |Fo[j]| (sigmoid link): saturated cells are judged absolutely.  (The floor carries the same relative
        terms as a live cell: a clamped cell's d = 2^-100 goes through the same evaluation, product and sum.)"""
    X, Fs, Fo = (np.asarray(a, dtype=np.float64) for a in (X, Fs, Fo))
    P = Fs @ Fo.T
    dP = P_REL * product_scale(Fs, Fo)
    aFo = np.abs(Fo)
    common = PROD + OUT + n_acc * U32
    if link == LINK_SIGMOID:
        sig, d = sigmoid_parts(lam * (P - 0.5))
        ds = lam * (dP + S_ARITH * (np.abs(P) + 0.5))
        floor = lam * CLAMP * (1 + FUN_D + common) * aFo.sum(axis=0)      # the clamped d is itself evaluated, multiplied and summed
        gnum = lam * (X * d * (np.expm1(ds) + FUN_D + common)) @ aFo + floor
        gden = lam * (sig * d * (np.expm1(2 * ds) + FUN_SD + common)) @ aFo + floor
        return gnum, gden
    pos = P > 0
    rel = np.zeros_like(P)
    rel[pos] = dP / P[pos]
    assert rel.max(initial=0.0) < 0.5, "a KL case with a positive product below twice the error of P"
    inv = np.zeros_like(P)
    inv[pos] = 1.0 / P[pos]
    return (X * inv * (rel / (1 - rel) + FUN_RCP + common)) @ aFo, None


def pass_acc(cols) -> int:
    """fp32 roundings of one output element of the 16-bit pass: three products per column of the (padded) sweep"""
    return 3 * 32 * ((cols + 31) // 32)


def sums16_bound(X, U, V, link, lam, O=None):
    """Bounds on |sums - sums_ref| for bmf_link_sums16: per cell the error df of the prediction (sigmoid: d expm1(ds) + FUN_SIG sig; KL:
    dP + u |P|), |x - f| moves by df, (x - f)^2 by 2 |x - f| df + df^2, plus TILE_ACC times the sum of the |terms|.  KL term of a
    cell: x = 0: dP + u p;  x = 1: dP + |log(1 - dP / p)| + 4 u (|p| + 1 + |log p|) for p - 1 - __logf(p) evaluated in fp32 (p = 0 comes
    out as exactly 0 from zero operands: only the evaluation term is left there)."""
    X, U, V = (np.asarray(a, dtype=np.float64) for a in (X, U, V))
    P, f, _, _ = link_cells(X, U, V, link, lam)
    dP = P_REL * product_scale(U, V)
    if link == LINK_SIGMOID:
        _, d = sigmoid_parts(lam * (P - 0.5))
        df = d * np.expm1(lam * (dP + S_ARITH * (np.abs(P) + 0.5))) + FUN_SIG * f
    else:
        df = np.where(P != 0, dP, 0.0) + U32 * np.abs(P)
    r = np.abs(X - f)
    g0 = df.sum() + TILE_ACC * r.sum()
    g1 = (2 * r * df + df * df).sum() + TILE_ACC * (r * r).sum()
    g2 = 0.0
    if link == LINK_KL:
        t = kl_cells(X, P)
        pos = P > 0
        rel = np.zeros_like(P)
        rel[pos] = dP / P[pos]
        assert rel.max(initial=0.0) < 0.5
        dt = np.where(X != 0, np.where(pos, dP, 0.0) - np.log1p(-rel) + 4 * U32 * (np.abs(P) + 1 + np.abs(np.log(np.maximum(P, KL_P_FLOOR)))), df)
        sel = np.ones_like(P) if O is None else (np.asarray(O) != 0).astype(np.float64)
        g2 = (sel * dt).sum() + TILE_ACC * (sel * np.abs(t)).sum()
    return np.array([g0, g1, g2])


def colsum_bound(F, want) -> np.ndarray:
    """half an fp32 ulp of the result plus rows 2^-53 sum |v| for the fp64 accumulation"""
    F = np.asarray(F, dtype=np.float64)
    return 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + F.shape[0] * 2.0 ** -53 * np.abs(F).sum(axis=0)


# ------------------------------------------------------------------------------------------------------------------------------
# case tables and input makers (host, fixed seeds)
# ------------------------------------------------------------------------------------------------------------------------------
GRID_ROWS, GRID_COLS = (1, 32, 33, 128, 129), (1, 33, 65, 97, 129, 193)
K_CYCLE = (5, 32, 40, 64)               # kp = 32 with k < kp and k = kp, kp = 64 likewise
# (rows, cols, k): the grid (1..7 tiles in one slab; the last valid row at 0, 31, 32, 127 of its block; one valid column in the last
# tile), four shapes for the ragged tile (16, 17, 31 and 32 valid columns), and the three slab shapes
PASS_CASES = [(r, c, K_CYCLE[(i + j) % 4]) for i, r in enumerate(GRID_ROWS) for j, c in enumerate(GRID_COLS)] + \
             [(33, 16, 32), (129, 49, 40), (32, 63, 5), (128, 64, 64)] + \
             [(130, 545, 5), (130, 515, 40), (130, 4100, 64)]
FACTOR_SETS = ("moderate", "saturating", "unbalanced", "zero_rows")
LAMS = (1.0, 10.0, 300.0)
ZROW, ZCOL = 0, 0                       # the zero factor rows of the `zero_rows` set: row 0 of U, row 0 of V


def kp_of(k) -> int:
    return 32 if k <= 32 else 64


def pad128(n) -> int:
    return (n + 127) // 128 * 128


def empty_row(rows):
    """the row of X that is left empty (None for fewer than four rows)"""
    return rows // 2 if rows >= 4 else None


@functools.lru_cache(maxsize=None)
def make_X(rows, cols) -> np.ndarray:
    """0/1 uint8, density 0.3; the last row and the last column hold both values where they have two cells, X[0, 0] = 1 (the cell where
    the zero factor rows of the `zero_rows` set meet), and one row in the middle is empty"""
    rs = np.random.RandomState(7 * rows + cols)
    X = (rs.rand(rows, cols) < 0.3).astype(np.uint8)
    if cols >= 2:
        X[rows - 1, cols - 2] = 0
    if rows >= 2:
        X[rows - 2, cols - 1] = 0
    if rows >= 3 and cols >= 3:
        X[0, 1:3] = (1, 0)
    X[rows - 1, cols - 1] = 1
    X[0, 0] = 1
    if empty_row(rows) is not None:
        X[empty_row(rows)] = 0
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=64)
def make_factors(rows, cols, k, name):
    """fp32 (U, V), rows x k and cols x k.
      moderate     |N(0, 1)| 0.4 + 1e-3, the factors of tests/test_link_gpu.py
      saturating   scaled row by row so that the products spread over about [0, 3]: lam = 300 sends cells far into both tails; the cell
                   (0, 0) is put at P = 1/2
      unbalanced   the moderate set with column 0 tiny in U and huge in V, column k - 1 the other way round, and column 1 of U dead
      zero_rows    the moderate set with row ZROW of U and row ZCOL of V zero"""
    rs = np.random.RandomState(1000 * k + 10 * FACTOR_SETS.index(name) + rows + cols)
    if name == "saturating":
        a = np.sqrt(12.0 / k)
        U, V = a * rs.rand(rows, k) * rs.rand(rows, 1), a * rs.rand(cols, k) * rs.rand(cols, 1)
        U[0] = np.sqrt(0.5 / k) * (1 + 0.2 * rs.rand(k))
        V[0] *= 0.5 / float(U[0].astype(np.float32).astype(np.float64) @ V[0])
    else:
        U = np.abs(rs.standard_normal((rows, k))) * 0.4 + 1e-3
        V = np.abs(rs.standard_normal((cols, k))) * 0.4 + 1e-3
        if name == "unbalanced":
            U[:, 0] *= 3e-5; V[:, 0] *= 1e5
            U[:, k - 1] *= 2e4; V[:, k - 1] *= 4e-5
            U[:, 1] = 0.0
        elif name == "zero_rows":
            U[ZROW], V[ZCOL] = 0.0, 0.0
    U, V = U.astype(np.float32), V.astype(np.float32)
    U.setflags(write=False)
    V.setflags(write=False)
    return U, V


def padded_factor(F, rows_pad, kp, fill_rows=None) -> np.ndarray:
    """F inside a rows_pad x kp fp32 array: zero padding columns; padding rows zero, or copies of `fill_rows` (one row of kp values)"""
    out = np.zeros((rows_pad, kp), np.float32)
    out[:F.shape[0], :F.shape[1]] = F
    if fill_rows is not None:
        out[F.shape[0]:, :F.shape[1]] = fill_rows
    return out


def poison_row(F) -> np.ndarray:
    """finite poison for the padding rows of a factor: half of its row of largest norm, so that no column maximum moves and a dead
    column stays dead (the scales of the split workspace, and with them every result, must stay what they were)"""
    F = np.asarray(F, dtype=np.float32)
    return (0.5 * F[np.argmax(np.abs(F).sum(axis=1))]).astype(np.float32)


def pack_bits(X, rows_pad, ldx, poison=False) -> np.ndarray:
    """rows_pad x ldx little-endian uint32 words of X (bit c of a row in word c // 32 at position c % 32).  The words past the last
    column tile are all ones always (no kernel may read them); `poison` also sets the padding bits of the last tile and every bit of
    the padding rows."""
    rows, cols = X.shape
    tiles = (cols + 31) // 32
    assert ldx >= tiles and rows_pad >= rows
    b = np.full((rows_pad, ldx * 32), 1 if poison else 0, np.uint8)
    b[:rows, :cols] = X
    b[:, tiles * 32:] = 1
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view(np.uint32)


# cell localisation: row i of X has its single one at column LOCAL_PI(i, tiles)
LOCAL_ROWS = 1024
LOCAL_TILES = (4, 7)


def local_pi(tiles) -> np.ndarray:
    """pi(i) for i < 1024: in-tile row i % 32 (the lane) meets in-tile column (i // 32) % 32, in tile (5 i + i // 32) % tiles"""
    i = np.arange(LOCAL_ROWS)
    return 32 * ((5 * i + i // 32) % tiles) + (i // 32) % 32


# bmf_link_split / bmf_link_split_pair
SPLIT_ROWS = (32, 128, 4128)
SPLIT_SETS = ("moderate", "span", "dead", "zero")


@functools.lru_cache(maxsize=None)
def split_factor(rows_pad, kp, name, which) -> np.ndarray:
    """a full rows_pad x kp fp32 factor (`which` = 0 / 1: the two factors of a pair).  span: column maxima from 2^-20 to 2^20 in factor
    0 and from 2^10 down to 2^-10 in factor 1, so the pair products span 2^-10 .. 2^10 and the small pairs of factor 1 land where
    the fp16 lo addend is subnormal; dead: column 3 of factor 0 and column 7 of factor 1 zero; zero: all zero"""
    rs = np.random.RandomState(31 * rows_pad + kp + 7 * SPLIT_SETS.index(name) + which)
    F = (np.abs(rs.standard_normal((rows_pad, kp))) * 0.4 + 1e-3).astype(np.float32)
    F[rs.rand(rows_pad, kp) < 0.05] = 0.0
    if name == "span":
        e = np.linspace(-20, 20, kp).round()
        F *= np.ldexp(1.0, (e if which == 0 else (e[::-1] / 2).round()).astype(np.int64)).astype(np.float32)
    elif name == "dead":
        F[:, 3 if which == 0 else 7] = 0.0
    elif name == "zero":
        F[:] = 0.0
    F.setflags(write=False)
    return F


# bmf_colsum_fill
COLSUM_ROWS = (1, 63, 64, 65, 129, 33000)
COLSUM_OUT_ROWS = (2, 128, 1152)
