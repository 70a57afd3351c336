"""The stream-K plan of the int8 bits GEMM, from the library's host-only query (bmf_xf_bits_i8_plan with an explicit compute-unit
count: no device is touched): equal, field by field, to the plain restatement in tests/i8_plan_ref.py; the properties the kernel's slab
contract rests on, checked from the query alone; and hand-worked plans at the shapes the GPU tests and the fit loop run."""
import pytest

import i8_plan_ref as R

# (rows_pad, reduction length): the two headline launches, every shape of tests/test_xf_bits_i8_slabs_gpu.py (rows padded to 512 as the
# launcher demands), the largest shape of test_xf_bits_i8_is_exact, and a few at the edges of the rule
GPU_SHAPES = [(53248, 2560), (8192, 16896), (106496, 2560), (3072, 20992), (153600, 512), (1536, 3584), (512, 512), (10240, 6656)]
SHAPES = [(100352, 20480), (20480, 100352)] + GPU_SHAPES + [(3072, 20480), (512, 1024), (1024, 512), (131072, 512), (16384, 1024),
                                                            (4096, 4096), (512, 524288 - 512), (7680, 1536)]
CUS = (256, 304, 64, 8)


@pytest.fixture(scope="module")
def lib():
    from pybmf_amd import _lib as L
    prev = L.lib.bmf_xf_bits_i8_variant(-1)
    yield L.lib
    L.lib.bmf_xf_bits_i8_variant(prev)


def launches():
    """(variant, ncols, kp): every launch width on every kernel variant (the variants serve whole 64-column factors only)"""
    return [(0, 32, 32), (0, 32, 64), (1, 32, 64), (4, 32, 64)] + [(v, 64, 64) for v in (0, 1, 2, 4)]


@pytest.mark.parametrize("cus", CUS)
def test_query_equals_the_restatement(lib, cus):
    for variant, ncols, kp in launches():
        assert lib.bmf_xf_bits_i8_variant(variant) >= 0
        for rows_pad, red in SHAPES:
            got = R.query(lib, rows_pad, red // 32, ncols, kp, cus)
            want = R.plan(rows_pad, red // 32, ncols, cus, R.variant_of(ncols, kp, variant))
            assert got is not None, (lib.bmf_last_error(), rows_pad, red)
            for name in R.Plan._fields:
                assert getattr(got, name) == getattr(want, name), (name, variant, ncols, kp, rows_pad, red)
    lib.bmf_xf_bits_i8_variant(0)


@pytest.mark.parametrize("cus", CUS)
def test_plan_properties(lib, cus):
    for variant, ncols, kp in launches():
        assert lib.bmf_xf_bits_i8_variant(variant) >= 0
        for rows_pad, red in SHAPES:
            p = R.query(lib, rows_pad, red // 32, ncols, kp, cus)
            what = (variant, ncols, kp, rows_pad, red)
            stages = red // 128
            assert p.total == rows_pad // p.tile_rows * stages and p.halves in (1, 2) and p.tile_rows in (256, 512), what
            bounds = R.slice_bounds(p)
            # the slices tile [0, total) without gap or overlap, in whole groups of four stages
            assert len(bounds) == p.n_slices >= 1 and bounds[0][0] == 0 and bounds[-1][1] == p.total, what
            assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:])), what
            assert all(u1 > u0 and (u1 - u0) % 4 == 0 and u0 % 4 == 0 for u0, u1 in bounds), what
            assert p.u_big % 4 == 0 and p.u_small % 4 == 0 and p.u_big >= p.u_small >= 4 and 0 <= p.n_big <= p.n_slices, what
            # the slice map is injective onto 0 .. n_slices - 1
            mapped = [(b, s) for b, s in enumerate(p.perm) if s != R.NONE]
            assert sorted(s for _, s in mapped) == list(range(p.n_slices)), what
            # the grid: whole XCD rounds of every column half, and workgroup w = block slice (w / 8 / halves) * 8 + w % 8 reaches the last one
            last = max(b for b, _ in mapped)
            assert p.grid % (8 * p.halves) == 0 and 0 < p.grid <= 512 * p.halves, what
            assert ((last // 8) * p.halves + p.halves - 1) * 8 + last % 8 < p.grid, what
            # slab slots: the largest number of slices that meet one row tile
            pieces = R.tile_pieces(p, stages)
            assert p.slots == max(len(v) for v in pieces.values()), what
            assert all([s for s, _, _ in v] == list(range(v[0][0], v[0][0] + len(v))) for v in pieces.values()), what
            assert all(v[0][1] == 0 and v[-1][2] == stages and all(a[2] == b[1] for a, b in zip(v, v[1:])) for v in pieces.values()), what
            # two lengths: the big slices sit on the first gsz / 2 block slices (the first-dispatched workgroup of every CU), the small
            # ones on the other half
            if p.n_big > 0:
                gsz = min(2 * cus // p.halves, 512)
                assert p.u_big > p.u_small and p.n_big <= gsz // 2 and p.n_slices - p.n_big <= gsz // 2, what
                assert all((s < p.n_big) == (b < gsz // 2) for b, s in mapped) and last < gsz, what
    lib.bmf_xf_bits_i8_variant(0)


# 256 compute units, the default kernel: (rows, reduction, ncols) -> (n_big, u_big, u_small, n_slices, slots).  Worked by hand from the
# rule, e.g. 100352 x 20480 at 64 columns: 392 tiles x 160 stages = 15680 groups on gsz = 256 slices per half; g_big = int(0.66 * 2 *
# 15680 / 256 + 0.999) = int(81.849) = 81 -> u_big 324; 128 big slices take 10368 groups, the other 5312 go to 128 small ones of
# ceil(5312 / 128) = 42 groups -> u_small 168, 127 of them; a tile of 160 stages meets at most 2 slices of >= 168.
ANCHORS = [
    ((100352, 20480, 64), (128, 324, 168, 255, 2)),
    ((20480, 100352, 32), (256, 164, 84, 503, 11)),
    ((53248, 2560, 64), (128, 24, 12, 219, 3)),
    ((8192, 16896, 64), (128, 24, 12, 224, 11)),
    ((106496, 2560, 32), (256, 24, 12, 438, 3)),
    ((3072, 20992, 64), (0, 8, 8, 246, 21)),
    ((153600, 512, 64), (0, 12, 12, 200, 1)),
    ((1280, 3584, 64), (0, 4, 4, 35, 7)),
    ((256, 512, 32), (0, 4, 4, 1, 1)),
]
# the two anchors whose row count is a multiple of the 256-row tile but not of the row padding (512): no launch and no query takes
# them as they stand; padded, as a launch sees them, they are 6 tiles x 7 groups and 2 tiles x 1 group of equal one-group slices
PADDED_ANCHORS = [
    ((1536, 3584, 64), (0, 4, 4, 42, 7)),
    ((512, 512, 32), (0, 4, 4, 2, 1)),
]


def test_hand_worked_plans(lib):
    assert lib.bmf_xf_bits_i8_variant(0) >= 0
    for (rows, red, ncols), want in ANCHORS + PADDED_ANCHORS:
        r = R.plan(rows, red // 32, ncols, 256)
        assert (r.n_big, r.u_big, r.u_small, r.n_slices, r.slots) == want, (rows, red, ncols)
        p = R.query(lib, rows, red // 32, ncols, ncols, 256)
        if rows % 512:
            assert p is None and b"rows_pad" in lib.bmf_last_error(), (rows, red, ncols)   # refused as a launch would be
        else:
            assert (p.n_big, p.u_big, p.u_small, p.n_slices, p.slots) == want, (rows, red, ncols)
            assert p == r
