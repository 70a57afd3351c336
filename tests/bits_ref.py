"""Plain NumPy restatements of the integer kernels of csrc/cover.hip and csrc/util.hip (cover count, Boolean product bits, per-row
confusion counts, bit packing, popcount) and of the two fixed-order fp64 sums (bmf_sqdiff_sum, bmf_reduce_slabs), on the packed
little-endian uint32 words the kernels see -- no m x n dense array is formed, so the tall cases stay cheap -- together with the
input makers and the case tables that tests/test_bit_kernels_cpu.py (which pins all of this to the oracle's dense definitions) and
tests/test_bit_kernels_gpu.py share.

Bit c of a row lives in word c // 32 at position c % 32.  A factor's row word holds bit l for factor l; colw[l] is the bit-column of
factor l.  Padding words (past `words`, up to the leading dimension) and padding bytes are filled with ones by the input makers: a
kernel that ignores its mask cannot pass."""
import functools
import math

import numpy as np

POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.uint8)
CUS_MI355X = 256      # compute units of the MI355X, for the launch arithmetic restated below
ONES = np.uint32(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def popcount_rows(words) -> np.ndarray:
    """set bits per row of a 2-d uint32 array (int64), through a 16-bit table"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    assert w.ndim == 2
    out = np.zeros(w.shape[0], np.int64)
    if w.shape[1] == 0:
        return out
    step = max(1, (1 << 22) // w.shape[1])       # ~16 MiB of words at a time
    for a in range(0, w.shape[0], step):
        blk = w[a:a + step]
        out[a:a + step] = POP16[blk.view(np.uint16)].sum(axis=1, dtype=np.int64)
    return out


def popcount(words) -> int:
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return int(popcount_rows(w.reshape(1, -1) if w.ndim != 2 else w).sum())


def product_words(rowbits, colw, words, row_block=16384) -> np.ndarray:
    """pd[i, :words] = OR over the factors l set in rowbits[i] of colw[l, :words]"""
    rowbits = np.asarray(rowbits)
    rowbits = rowbits.view(np.uint64) if rowbits.dtype == np.int64 else rowbits.astype(np.uint64)
    colw = np.asarray(colw, dtype=np.uint32)
    rows = rowbits.shape[0]
    pd = np.zeros((rows, words), np.uint32)
    for a in range(0, rows, row_block):
        rb = rowbits[a:a + row_block]
        blk = pd[a:a + row_block]
        for l in range(64):
            sel = np.nonzero((rb >> np.uint64(l)) & np.uint64(1))[0]
            if sel.size:
                assert l < colw.shape[0], "a factor bit at or above kp is outside the kernels' contract"
                blk[sel] |= colw[l, :words]
    return pd


def cover_counts(Xw, words, rowbits, colw, row_block=16384):
    """(TP, FP) of the Boolean product of (rowbits, colw) against the bits Xw[:, :words]"""
    Xw = np.asarray(Xw, dtype=np.uint32)
    tp = fp = 0
    for a in range(0, Xw.shape[0], row_block):
        pd = product_words(rowbits[a:a + row_block], colw, words)
        x = Xw[a:a + row_block, :words]
        tp += popcount(x & pd)
        fp += popcount(~x & pd)
    return tp, fp


def confusion_rows(Gw, Pw, words):
    """per-row tp = |G & P| and fp = |~G & P| over the first `words` words"""
    g, p = np.asarray(Gw, dtype=np.uint32)[:, :words], np.asarray(Pw, dtype=np.uint32)[:, :words]
    return popcount_rows(g & p), popcount_rows(~g & p)


def pack_rows(X_u8, cols) -> np.ndarray:
    """bits of X_u8[:, :cols] != 0, in 2 * ceil(cols / 64) words per row (the pairs of words that hold real columns)"""
    X = np.asarray(X_u8)[:, :cols] != 0
    pairs = (cols + 63) // 64
    b = np.zeros((X.shape[0], pairs * 64), np.uint8)
    b[:, :cols] = X
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view(np.uint32)


def sqdiff(A, B, W=None) -> float:
    """sum(W o (A - B)^2), the fp64 terms summed without error (math.fsum)"""
    d = np.asarray(A, dtype=np.float64).ravel() - np.asarray(B, dtype=np.float64).ravel()
    t = d * d if W is None else np.asarray(W, dtype=np.float64).ravel() * d * d
    return math.fsum(t.tolist())


def reduce_slabs(slabs, stride, count, n) -> np.ndarray:
    """out[i] = sum_b slabs[b * stride + i] in fp64, in slab order"""
    s = np.asarray(slabs, dtype=np.float32)
    acc = np.zeros(n, np.float64)
    for b in range(count):
        acc += s[b * stride:b * stride + n].astype(np.float64)
    return acc


# ------------------------------------------------------------------------------------------------------------------------------
# input makers (host, fixed seeds)
# ------------------------------------------------------------------------------------------------------------------------------
def random_words(rng, shape) -> np.ndarray:
    """uint32 words whose bits are set with probability 0.3125 = P(a & (b | (c & d)))"""
    a, b, c, d = (rng.integers(0, 1 << 32, size=shape, dtype=np.uint32) for _ in range(4))
    return a & (b | (c & d))


def factor_row_words(rng, rows, kp, max_bits=None) -> np.ndarray:
    """uint64 row words with a mix of 0, 1, 2 and many set bits, none at or above kp.  Row 0 has bit kp - 1 alone, row 1 is zero
    (when they exist); `max_bits` = 2 keeps every row at two bits at most (the tall cases: the host reference walks set bits)."""
    one = np.uint64(1)
    b0 = one << rng.integers(0, kp, size=rows).astype(np.uint64)
    b1 = one << rng.integers(0, kp, size=rows).astype(np.uint64)
    many = rng.integers(0, 1 << 63, size=rows, dtype=np.uint64) << one | rng.integers(0, 2, size=rows).astype(np.uint64)
    if kp < 64:
        many &= np.uint64((1 << kp) - 1)
    kind = rng.integers(0, 4, size=rows)
    if max_bits is not None:
        assert max_bits == 2
        kind = np.minimum(kind, 2)
    u = np.where(kind == 0, np.uint64(0), np.where(kind == 1, b0, np.where(kind == 2, b0 | b1, many))).astype(np.uint64)
    u[0] = one << np.uint64(kp - 1)
    if rows > 1:
        u[1] = 0
    if rows > 2 and max_bits is None:
        u[2] = np.uint64((1 << kp) - 1)      # every factor at once, bit 63 included at kp = 64
    return u


def padded(core, ld, fill=ONES) -> np.ndarray:
    """core (rows x w) inside a rows x ld array whose columns past w hold `fill`"""
    out = np.full((core.shape[0], ld), fill, dtype=core.dtype)
    out[:, :core.shape[1]] = core
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# bmf_cover_count: the launch arithmetic of bmf_cover_launch, restated (not imported), and the case table
# ------------------------------------------------------------------------------------------------------------------------------
def cover_launch_plan(rows_pad, words, cus=CUS_MI355X) -> dict:
    """Which kernel, template instantiation, chunk layout and row groups bmf_cover_launch selects.

    words >= 128, the wide kernel: chunk columns = ceil(words / 640); chunk words cw = the words of one column rounded up to a multiple
    of 128 (<= 640); a lane owns N4 segments of 4 words and a tail segment of TW words: N4 = min(cw / 256, 2), the rest r = cw - 256 N4
    gives TW = 0 (r = 0), 2 (r <= 128) or 4.  Row groups: min(cus / columns, rows_pad / 64) equal groups of whole 64-row units; a wave
    (16 per block) owns rows_per_block / 16 rows and takes them 64 at a time.
    words < 128, the narrow kernel: one chunk column, up to 512 row groups of 8 waves; with at least 8 groups and at least 4 units per
    group the first half of the groups are 'big' (share 0.63 of a pair's units), the others share the rest."""
    assert rows_pad % 64 == 0 and words % 4 == 0 and rows_pad > 0 and words > 0
    units = rows_pad // 64
    if words >= 128:
        cols = (words + 639) // 640
        cw = (-(-words // cols) + 127) // 128 * 128
        n4 = min(cw // 256, 2)
        rem = cw - 256 * n4
        tw = 0 if rem == 0 else (2 if rem <= 128 else 4)
        groups = min(max(cus // cols, 1), units)
        rpb = -(-units // groups) * 64
        groups = -(-rows_pad // rpb)
        last = words - (cols - 1) * cw
        assert 0 < last <= cw and cw <= 640
        return dict(kernel="wide", n4=n4, tw=tw, cw=cw, cols=cols, last_chunk=last, ragged=last < cw, groups=groups,
                    rows_per_block=rpb, last_block_rows=rows_pad - (groups - 1) * rpb, rows_per_wave=rpb // 16, scheme="equal")
    groups = min(512, units)
    if groups >= 8 and units >= 4 * groups:
        y_big = groups // 2
        u_big = int(0.63 * 2.0 * units / groups + 0.999)
        rest = units - min(units, y_big * u_big)
        n_small = groups - y_big
        rpb = max(1, -(-rest // n_small)) * 64
        return dict(kernel="narrow", cols=1, last_chunk=words, ragged=words < 256, groups=groups, scheme="two-size", y_big=y_big,
                    rows_big=u_big * 64, rows_per_block=rpb, rows_per_wave=u_big * 8)
    rpb = -(-units // groups) * 64
    groups = -(-rows_pad // rpb)
    return dict(kernel="narrow", cols=1, last_chunk=words, ragged=words < 256, groups=groups, scheme="equal", y_big=0, rows_big=0,
                rows_per_block=rpb, last_block_rows=rows_pad - (groups - 1) * rpb, rows_per_wave=rpb // 8)


# (name, units as (a, b): rows_pad = 64 * (a * cus + b), words, ldx - words, ldcb - words, kps, max factor bits per row)
COVER_CASES = [
    # wide kernel, one full chunk: (N4, TW) = (0, 2), (1, 0), (1, 2), (2, 0), (2, 2)
    ("full128", (0, 3), 128, 0, 0, (64, 32), None),
    ("full256", (0, 3), 256, 0, 0, (64,), None),
    ("full384", (0, 3), 384, 0, 0, (64,), None),
    ("full512", (0, 3), 512, 0, 0, (64,), None),
    ("full640", (0, 3), 640, 0, 0, (64,), None),
    # one ragged chunk (260 and 516: two lanes of the tail segment on)
    ("ragged132", (0, 3), 132, 0, 0, (64, 32), None),
    ("ragged260", (0, 3), 260, 0, 0, (64,), None),
    ("ragged388", (0, 3), 388, 0, 0, (64,), None),
    ("ragged516", (0, 3), 516, 0, 0, (64,), None),
    ("ragged636", (0, 3), 636, 0, 0, (64,), None),
    # several chunk columns, the last one ragged: 2 x 384 (260), 3 x 512 (260), 4 x 512 (388)
    ("cols2", (0, 2), 644, 0, 0, (64,), None),
    ("cols3", (0, 2), 1284, 0, 0, (64,), None),
    ("cols4", (0, 2), 1924, 0, 0, (64,), None),
    # row groups of the wide kernel: one unit; a short last block; more than 64 rows per wave (second trip of the g loop)
    ("unit", (0, 1), 128, 0, 0, (64,), None),
    ("shortlast", (1, 1), 128, 0, 0, (64,), None),
    ("tall_wide", (16, 1), 128, 0, 0, (64,), 2),
    # narrow kernel
    ("narrow4", (0, 1), 4, 0, 0, (64, 32), None),
    ("narrow124", (0, 1), 124, 0, 0, (64, 32), None),
    ("narrow16_ld", (0, 5), 16, 4, 8, (64, 32), None),
    ("narrow_equal_max", (0, 2047), 4, 0, 0, (64, 32), 2),
    ("narrow_two_size", (0, 2048), 4, 0, 0, (64, 32), 2),
    ("narrow_two_size_g2", (0, 4100), 8, 0, 0, (64, 32), 2),
    # leading dimensions larger than words, ones in the padding: one wide, one narrow
    ("wide_ld", (0, 3), 260, 4, 8, (64,), None),
    ("narrow_ld", (0, 3), 124, 4, 8, (64,), None),
]
COVER_PARAMS = [(c[0], kp) for c in COVER_CASES for kp in c[5]]
_COVER_BY_NAME = {c[0]: c for c in COVER_CASES}


def cover_rows_pad(name, cus=CUS_MI355X) -> int:
    a, b = _COVER_BY_NAME[name][1]
    return 64 * (a * cus + b)


@functools.lru_cache(maxsize=3)
def cover_case(name, kp, cus=CUS_MI355X) -> dict:
    """Inputs and exact (TP, FP) of one case: X (rows_pad x ldx) and colw (kp x ldcb) with ones in the padding, u (rows_pad)."""
    _, _, words, dx, dcb, _, max_bits = _COVER_BY_NAME[name]
    rows_pad = cover_rows_pad(name, cus)
    seed = [i for i, c in enumerate(COVER_CASES) if c[0] == name][0]
    rng = np.random.default_rng([20240, seed, kp])
    X = padded(random_words(rng, (rows_pad, words)), words + dx)
    colw = padded(random_words(rng, (kp, words)), words + dcb)
    u = factor_row_words(rng, rows_pad, kp, max_bits)
    tp, fp = cover_counts(X, words, u, colw)
    for a in (X, colw, u):
        a.setflags(write=False)
    return dict(name=name, kp=kp, rows_pad=rows_pad, words=words, ldx=words + dx, ldcb=words + dcb, X=X, colw=colw, u=u, tp=tp, fp=fp)


# ------------------------------------------------------------------------------------------------------------------------------
# the other kernels' case tables
# ------------------------------------------------------------------------------------------------------------------------------
# bmf_boolean_product_bits: (name, rows, words, ldcb - words, ldo - words); 4160 x 512 row-word pairs pass the 8192 x 256 grid
PRODUCT_CASES = [("one", 1, 1, 0, 0), ("small", 3, 5, 0, 0), ("stride", 4160, 512, 0, 0), ("ld", 3, 5, 3, 5)]
PRODUCT_SENTINEL = np.uint32(0xA5A5A5A5)


@functools.lru_cache(maxsize=None)
def product_case(name, kp) -> dict:
    _, rows, words, dcb, do = {c[0]: c for c in PRODUCT_CASES}[name]
    rng = np.random.default_rng([20241, rows, words, kp, dcb])
    colw = padded(random_words(rng, (kp, words)), words + dcb)
    u = factor_row_words(rng, rows, kp)
    want = product_words(u, colw, words)
    for a in (colw, u, want):
        a.setflags(write=False)
    return dict(rows=rows, words=words, kp=kp, ldcb=words + dcb, ldo=words + do, colw=colw, u=u, want=want)


# bmf_confusion_rows: (rows, words, ldg - words, ldp - words); 16390 rows pass the 4096 x 4 waves of the grid
CONFUSION_CASES = [(r, w, 0, 0) for r in (1, 5) for w in (1, 63, 64, 65, 130)] + [(16390, 3, 0, 0), (5, 65, 3, 1), (5, 64, 0, 2)]


@functools.lru_cache(maxsize=None)
def confusion_case(rows, words, dg, dp) -> dict:
    rng = np.random.default_rng([20242, rows, words, dg, dp])
    G = padded(random_words(rng, (rows, words)), words + dg)
    P = padded(random_words(rng, (rows, words)), words + dp)
    tp, fp = confusion_rows(G, P, words)
    for a in (G, P):
        a.setflags(write=False)
    return dict(rows=rows, words=words, ldg=words + dg, ldp=words + dp, G=G, P=P, tp=tp, fp=fp)


# bmf_pack_rows_u8: (rows, cols, ldx - cols, ldw - words needed); 33000 x 65 is 66000 wave tasks for 8192 x 4 waves
PACK_CASES = [(5, c, 0, 0) for c in (1, 31, 32, 33, 63, 64, 65, 129)] + [(5, c, 7, 0) for c in (1, 33, 64, 65, 129)] + \
             [(5, 65, 0, 4), (3, 31, 7, 2), (33000, 65, 0, 0)]
PACK_BYTES = np.array([0, 0, 1, 2, 255], dtype=np.uint8)      # drawn uniformly: density 0.6, three kinds of 'set'
PACK_SENTINEL = np.uint32(0x5A5A5A5A)


@functools.lru_cache(maxsize=None)
def pack_case(rows, cols, dx, dw) -> dict:
    rng = np.random.default_rng([20243, rows, cols, dx, dw])
    X = padded(PACK_BYTES[rng.integers(0, len(PACK_BYTES), size=(rows, cols))], cols + dx, np.uint8(255))
    X[:, cols - 1] = 2 * (np.arange(rows) % 2)        # the last real column: clear in even rows, a byte of 2 in odd ones
    need = 2 * ((cols + 63) // 64)
    want = pack_rows(X, cols)
    X.setflags(write=False)
    return dict(rows=rows, cols=cols, ldx=cols + dx, ldw=need + dw, need=need, X=X, want=want)


# bmf_popcount: (rows, words, ldw - words); 3 x 180001 words pass the 2048 x 256 threads of the grid
POPCOUNT_CASES = [(1, 1, 0), (5, 3, 2), (7, 65, 1), (3, 180001, 0), (3, 180001, 3)]

SQDIFF_N = [0, 1, 255, 256, 257, 300001]          # 300001 passes the 1024 x 256 threads of the grid
REDUCE_N = [1, 64, 65, 4096, 65536, 65540]        # >= 65536 and a multiple of 4: the float4 kernel
REDUCE_COUNTS = [1, 3, 4, 5, 16, 17, 33]
