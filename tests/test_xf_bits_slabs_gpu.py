"""xf_bits_kernel (csrc/xf_bits.hip, the bf16 / fp16 bits GEMM behind bmf_xf_bits and bmf_xf_bits_f16) slab by slab on stream-K plans
whose slices are several stages long: the second prologue DMA, the look-ahead DMA into the ring buffer a finished stage left, the hand-over
of the next stage's X words, the B-fragment fetch across the stage barrier, and slices that end one 512-row tile and start the next.

The per-slab contract (tests/xf_plan_ref.py): piece (tile, s0, s1, slot) of the plan writes the sum over the stages [s0, s1) of the tile
into slab `slot` of the tile's rows; the piece that holds the tile's last stage zero-fills every slot behind its own up to `splits`.

The reference takes nothing from the panel builders: the panel is read back from the device, un-permuted with bmf_panel_pos and decoded
addend by addend; Fq = the sum of the addends in fp64 (for fp16 panels the column-scaled value, with colscale from scale[kp:]).  The
expected block of a piece is bits[tile rows, 128 s0 : 128 s1] @ Fq[128 s0 : 128 s1] in fp64, times 1 (bf16) or 2 colscale (fp16: the
kernel forms colscale * acc with the bits expanded to 2.0).  All values are integers on a power-of-two grid per column, so fp64 is exact.

Two classes of cells.
  exact    every row in the small-integer columns, and the four-per-stage, single-one, all-zero and padding rows in all columns: every
           product is exact in the 16-bit formats and every partial sum of a piece fits 24 bits (asserted on the host per piece: ones of the
           row in the piece x max sum_t |addend_t| in units of the column's grid < 2^24), so fp32 accumulation in any order is exact and the
           comparison is on fp32 bit patterns, no tolerance.  Cells nobody sums into (behind a tile's last contributor) are +0.0.
           (The last column holds 23-bit integers so that the third bf16 addend is not always zero: there the four-per-stage rows are in the
           bounded class, 24 such addends do not fit 24 bits.)
  bounded  dense and all-ones rows in the wide columns, where the order of the fp32 additions matters:
           |got - want| <= n 2^-23 sum|addends|, n = ones of the row in the piece x terms, the sum of absolute values from the fp64 reference
           of the same piece (the textbook bound of a length-n fp32 sum with either rounding or truncation per addition).

`out` is pre-filled with a marker no sum can take (-7.5: every sum of a negative column is an integer) and has guard floats in front of
it, behind it and between the slabs (the slack of slab_stride); X sits as a column block inside a wider marked matrix (ldw > red_words), the
panel rows are longer than the reduction (ldp > 32 red_words); all inputs must come back byte for byte and a second launch must give the same
bytes.  The shapes are for 256 compute units; on another device the case's property fails and so does the test."""
import contextlib
import functools
import time

import numpy as np
import pytest

import xf_plan_ref as R

pytestmark = pytest.mark.gpu

MARK = -7.5
GUARD = 16            # floats: keeps the 16-byte alignment the launch asks for
MARK_WORD = 0xF9F9F9F9
MARK_I16 = -1543
LEFT = 4              # words of the wider bit matrix in front of X (16 bytes: the alignment of the launch) ...
RIGHT = 4             # ... and behind it
PAD_ROWS = 37         # zero padding rows at the end of the matrix

DENSE, ONES, ZERO, SINGLE, FOUR, PADDING = range(6)


@pytest.fixture(scope="module")
def L():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def make_bits(rows_pad, stages):
    """x (rows_pad, 128 stages) uint8 cells and the class of every row.  Every 512-row tile holds, in this order: two all-ones rows, two
    all-zero rows, 128 rows with a single one (row i: position i of a stage, the stage walking through the reduction with the row and the
    tile), 128 rows with exactly four ones at random positions in every stage, dense random rows of density 1 / 4; the last PAD_ROWS rows of
    the matrix are zero padding."""
    red = R.STAGE * stages
    rng = np.random.default_rng(rows_pad * 1000 + stages)
    packed = rng.integers(0, 256, (rows_pad, red // 8), dtype=np.uint8) & rng.integers(0, 256, (rows_pad, red // 8), dtype=np.uint8)
    x = np.unpackbits(packed, axis=1, bitorder="little")
    cls = np.full(rows_pad, DENSE, dtype=np.uint8)
    i = np.arange(128)
    for t in range(rows_pad // R.TILE_ROWS):
        b = R.TILE_ROWS * t
        x[b:b + 2], cls[b:b + 2] = 1, ONES
        x[b + 2:b + 4], cls[b + 2:b + 4] = 0, ZERO
        x[b + 4:b + 260] = 0
        x[b + 4 + i, R.STAGE * ((5 * i + 3 * t) % stages) + i] = 1
        cls[b + 4:b + 132] = SINGLE
        four = x[b + 132:b + 260].reshape(128, stages, R.STAGE)
        assert four.base is not None                                          # a view: the ones land in x
        np.put_along_axis(four, np.argpartition(rng.random((128, stages, R.STAGE), dtype=np.float32), 4, axis=2)[:, :, :4], 1, axis=2)
        cls[b + 132:b + 260] = FOUR
    x[rows_pad - PAD_ROWS:], cls[rows_pad - PAD_ROWS:] = 0, PADDING
    per_stage = x.reshape(rows_pad, stages, R.STAGE).sum(axis=2)
    assert (per_stage[cls == FOUR] == 4).all() and (x[cls == SINGLE].sum(axis=1) == 1).all() and (per_stage[cls == ONES] == R.STAGE).all()
    assert not x[(cls == ZERO) | (cls == PADDING)].any() and (cls == DENSE).sum() >= rows_pad // 4
    assert abs(x[cls == DENSE].mean() - 0.25) < 0.01
    return x, cls


def make_factor(red, kp):
    """red x kp, integer-valued: columns [0, kp / 2) in [0, 64) with an all-zero column and a column arange % 7, columns [kp / 2, kp) in
    [0, 2^17) (two fp16 addends; two bf16 addends as well, because the builder rounds to nearest: the remainder of a 17-bit integer after
    its first addend has 8 bits and a sign), the last column in [0, 2^23) so that the third bf16 addend is in use too; whole columns times
    2^-30, 2^20 and -1 in either half (exact, moves the fp16 column scales apart, exercises the sign)"""
    rng = np.random.default_rng(red + kp)
    h = kp // 2
    F = np.empty((red, kp), dtype=np.float64)
    F[:, :h] = rng.integers(0, 64, (red, h))
    F[:, h:] = rng.integers(0, 2 ** 17, (red, kp - h))
    F[:, kp - 1] = rng.integers(0, 2 ** 23, red)
    F[:, 0] = 0
    F[:, 1] = np.arange(red) % 7
    for c, f in ((3, 2.0 ** -30), (4, -1.0), (5, 2.0 ** 20), (h + 1, 2.0 ** -30), (h + 2, 2.0 ** 20), (h + 3, -1.0)):
        F[:, c] *= f
    F32 = F.astype(np.float32)
    assert np.array_equal(F32.astype(np.float64), F)
    return F32


def read_addends(L, panel_host, kind, red):
    """(terms, red, kp) fp64: the addends a device panel holds, in reduction order"""
    pos = np.array([L.lib.bmf_panel_pos(c) for c in range(R.STAGE)])
    assert sorted(pos.tolist()) == list(range(R.STAGE))
    r = np.arange(red)
    idx = (r // R.STAGE) * R.STAGE + pos[r % R.STAGE]
    if kind == "f16":
        val = panel_host.view(np.float16).astype(np.float64)
    else:
        val = (panel_host.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return np.ascontiguousarray(val[:, :, idx].transpose(0, 2, 1))


def column_grid(add):
    """(kp,) the largest power of two that divides every addend of the column (1 for an all-zero column)"""
    mag = np.abs(add)
    top, low = mag.max(axis=(0, 1)), np.where(mag > 0, mag, np.inf).min(axis=(0, 1))
    zero = top == 0
    # every addend is a 16-bit float: a multiple of 2^-10 of its own power of two, so of unit = 2^(e_low - 11) with low = m 2^e_low
    unit = np.where(zero, 1.0, 2.0 ** (np.frexp(np.where(zero, 1.0, low))[1] - 12.0))
    assert (top / unit < 2.0 ** 62).all()
    ints = (mag / unit[None, None, :]).astype(np.int64)
    assert np.array_equal(ints.astype(np.float64) * unit[None, None, :], mag)
    every = np.bitwise_or.reduce(ints, axis=(0, 1))                             # its lowest set bit: the lowest set bit of any addend
    g = np.where(zero, 1.0, (every & -every).astype(np.float64) * unit)
    return g


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def exact_rows_mask(cls, kp):
    """(rows_pad, kp) bool: the exact class"""
    m = np.zeros((len(cls), kp), dtype=bool)
    m[:, :kp // 2] = True
    m[np.isin(cls, (ZERO, SINGLE, FOUR, PADDING))] = True
    m[cls == FOUR, kp - 1] = False                                            # the 23-bit column: 24 of its addends do not fit 24 bits
    return m


def one_blas_thread():
    """the products of a piece are small (512 x <= 768 x 128): on one BLAS thread they run several times faster than spread over a pool"""
    try:
        import threadpoolctl
    except ImportError:
        return contextlib.nullcontext()
    return threadpoolctl.threadpool_limits(limits=1, user_api="blas")


def reference(x, cls, add, outscale, segs, splits):
    """want (splits, rows_pad, kp) fp64, exact (same shape, bool), bound (same shape, fp64: the gate of the bounded class)"""
    with one_blas_thread():
        return reference_(x, cls, add, outscale, segs, splits)


def reference_(x, cls, add, outscale, segs, splits):
    terms, red, kp = add.shape
    rows_pad = x.shape[0]
    both = np.concatenate([add.sum(axis=0), np.abs(add).sum(axis=0)], axis=1)    # Fq | sum_t |addend_t|: one product per piece
    Fabs = both[:, kp:]
    grid = column_grid(add)
    rowmask = exact_rows_mask(cls, kp)
    want = np.zeros((splits, rows_pad, kp))
    bound = np.zeros((splits, rows_pad, kp))
    exact = np.ones((splits, rows_pad, kp), dtype=bool)                       # cells nobody sums into: +0.0, exactly
    seen = set()
    for s in segs:
        assert (s.tile, s.slot) not in seen and s.slot < splits
        seen.add((s.tile, s.slot))
        rows, cols = slice(R.TILE_ROWS * s.tile, R.TILE_ROWS * (s.tile + 1)), slice(R.STAGE * s.s0, R.STAGE * s.s1)
        xb = x[rows, cols].astype(np.float64)
        ones = xb.sum(axis=1)
        prod = xb @ both[cols]
        want[s.slot, rows] = prod[:, :kp]
        bound[s.slot, rows] = (ones * terms * 2.0 ** -23)[:, None] * prod[:, kp:]
        exact[s.slot, rows] = rowmask[rows]
        # before exactness is trusted: every partial sum of the piece, in any order, fits the 24 bits of an fp32 significand
        fits = ones[:, None] * (Fabs[cols].max(axis=0) / grid)[None, :] < 2.0 ** 24
        assert fits[rowmask[rows]].all(), s
    want *= outscale[None, None, :]
    want += 0.0                                                                # (no negative zeros)
    bound *= outscale[None, None, :]
    return want, exact, bound


def compare(got, want, exact, bound):
    """the exact class on bit patterns, the bounded class against its gate; returns the worst error / gate of the bounded class"""
    w32 = want.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64)[exact], want[exact])          # the expected values are fp32 numbers
    diff = (np.ascontiguousarray(got).view(np.int32) != w32.view(np.int32)) & exact
    if diff.any():
        bad = np.argwhere(diff)
        s, r, c = bad[0]
        raise AssertionError(f"{len(bad)} exact-class slab cells differ; first: slot {s} row {r} (tile {r // R.TILE_ROWS}, row {r % R.TILE_ROWS} of it) "
                             f"column {c}: got {got[s, r, c]!r} want {w32[s, r, c]!r}")
    loose = ~exact
    err = np.abs(got.astype(np.float64) - want)[loose]
    gate = bound[loose]
    assert np.isfinite(err).all()
    over = err > gate
    assert not over.any(), f"{over.sum()} bounded-class cells over their gate; worst error / gate {np.max(err[over] / np.maximum(gate[over], 1e-300)):.3g}"
    return float(np.max(err[gate > 0] / gate[gate > 0])) if (gate > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------------------------------------
INSTANCES = [("bf16", 32, 1), ("bf16", 32, 2), ("bf16", 32, 3), ("bf16", 64, 1), ("bf16", 64, 2), ("bf16", 64, 3), ("f16", 32, 2), ("f16", 64, 2)]
THREE = [("f16", 64, 2), ("bf16", 64, 3), ("bf16", 32, 1)]          # (bf16, 64, 3): the largest LDS ring, 144 KiB
PARAMS = [(c.name,) + inst for c in R.CASES for inst in (INSTANCES if c.name in ("cross2", "ring") else THREE)]


def build_panel(L, F32, kind, kp, terms, ldp):
    """the device panel (terms, kp, ldp) of F32 by the stand-alone builders, marker in the elements past the reduction; colscale or None"""
    import torch
    red = F32.shape[0]
    panel = torch.full((terms, kp, ldp), MARK_I16, dtype=torch.int16, device="cuda:0")
    Fd = dev(F32)
    scale = None
    if kind == "f16":
        assert terms == 2
        ws = torch.zeros(red // R.STAGE * kp, dtype=torch.float32, device="cuda:0")
        scale = torch.zeros(2 * kp, dtype=torch.float32, device="cuda:0")
        L.check(L.lib.bmf_make_panel_f16(L.ptr(Fd), red, kp, kp, L.ptr(panel), ldp, L.ptr(ws), L.ptr(scale), None))
    else:
        L.check(L.lib.bmf_make_panel(L.ptr(Fd), red, kp, kp, terms, L.ptr(panel), ldp, None))
    torch.cuda.synchronize()
    assert (panel[:, :, red:] == MARK_I16).all()
    return panel, scale


@pytest.mark.parametrize("name,kind,kp,terms", PARAMS, ids=[f"{p[0]}-{p[1]}-kp{p[2]}-t{p[3]}" for p in PARAMS])
def test_every_slab_of_a_multi_stage_plan(L, name, kind, kp, terms):
    import torch
    t_start = time.time()
    case = R.CASE[name]
    rows_pad, stages = case.rows_pad, case.stages
    red, red_words = R.STAGE * stages, 4 * stages
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = R.plan(rows_pad, stages, cus)
    segs = R.segments(plan)
    case.prop(plan, segs)                                                     # the plan this case is named for, on THIS device
    assert L.lib.bmf_xf_bits_slots(rows_pad, red_words, terms, kp) == plan.slots
    splits = plan.slots + (2 if (name, kind, kp) == ("cross2", "f16", 64) else 1)

    # inputs: X as a column block of a wider marked matrix, panel rows longer than the reduction
    x, cls = make_bits(rows_pad, stages)
    ldw, ldp = LEFT + red_words + RIGHT, red + 8
    words = np.full((rows_pad, ldw), MARK_WORD, dtype=np.uint32)
    words[:, LEFT:LEFT + red_words] = np.packbits(x, axis=1, bitorder="little").view(np.uint32)
    bits = dev(words.view(np.int32))
    F32 = make_factor(red, kp)
    panel, scale = build_panel(L, F32, kind, kp, terms, ldp)
    panel_host = panel.cpu().numpy()
    add = read_addends(L, panel_host[:, :, :red], kind, red)
    if kind == "f16":
        colscale = scale.cpu().numpy()[kp:].astype(np.float64)
        assert (np.frexp(colscale)[0] == 0.5).all()                           # powers of two
        outscale = 2.0 * colscale
    else:
        outscale = np.ones(kp)
    # the factor arrived as it was made (so the classes are what they are named for): exactly where the format holds it, and with every
    # addend in use in the wide columns
    Fq = add.sum(axis=0) * outscale[None, :]
    h = kp // 2
    assert np.array_equal(Fq[:, :h], F32[:, :h].astype(np.float64))
    if kind == "f16":
        assert np.array_equal(Fq[:, :kp - 1], F32[:, :kp - 1].astype(np.float64))   # (two fp16 addends hold 22 bits, the last column has 23)
    elif terms == 3:
        assert np.array_equal(Fq, F32.astype(np.float64))
    assert all(np.count_nonzero(add[t][:, h:]) > red * (kp - h) // 2 for t in range(min(terms, 2)))
    assert all(np.count_nonzero(add[t][:, kp - 1]) > red // 2 for t in range(terms))

    t_ref = time.time()
    want, exact, bound = reference(x, cls, add, outscale, segs, splits)
    t_ref = time.time() - t_ref
    tiles_with_tail = sum(1 for s in segs if s.is_last and s.slot + 1 < splits)
    assert tiles_with_tail == plan.tiles                                      # every tile has slots to zero-fill: the surplus one at least

    stride = rows_pad * kp + GUARD
    buf = torch.full((GUARD + splits * stride,), MARK, dtype=torch.float32, device="cuda:0")
    inputs = {"bits": bits, "panel": panel}
    if scale is not None:
        inputs["scale"] = scale
    before = {k_: v.cpu().numpy().tobytes() for k_, v in inputs.items()}

    def launch():
        a, o = bits.data_ptr() + 4 * LEFT, buf.data_ptr() + 4 * GUARD
        if kind == "f16":
            rc = L.lib.bmf_xf_bits_f16(a, rows_pad, ldw, red_words, panel.data_ptr(), ldp, scale.data_ptr() + 4 * kp, kp, o, stride, splits, None)
        else:
            rc = L.lib.bmf_xf_bits(a, rows_pad, ldw, red_words, panel.data_ptr(), ldp, terms, kp, o, stride, splits, None)
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.lib.bmf_last_error())
        for k_, v in inputs.items():
            assert v.cpu().numpy().tobytes() == before[k_], f"input {k_} was written"
        host = buf.cpu().numpy()
        assert (host[:GUARD] == MARK).all(), "guard in front of out"
        body = host[GUARD:].reshape(splits, stride)
        assert (body[:, rows_pad * kp:] == MARK).all(), "guards between and behind the slabs"
        return body[:, :rows_pad * kp].reshape(splits, rows_pad, kp)

    got = launch().copy()
    assert (got != MARK).all(), "a cell of the slabs was not written"
    worst = compare(got, want, exact, bound)
    assert not got[plan.slots:].any() and not got[:, cls == PADDING].any()
    buf.fill_(MARK)
    assert launch().tobytes() == got.tobytes(), "a second launch gave other bytes"

    print(f"\n[xf slabs] {name} {kind} kp {kp} terms {terms}: rows_pad {rows_pad} stages {stages} cus {cus} | upw {plan.units_per_wg} workgroups {plan.num_wgs} "
          f"slots {plan.slots} splits {splits} piece lengths {R.piece_lengths(segs)} | exact cells {int(exact.sum())} bounded cells {int((~exact).sum())} "
          f"worst bounded error / gate {worst:.4f} | reference {t_ref:.2f} s, case {time.time() - t_start:.2f} s")
