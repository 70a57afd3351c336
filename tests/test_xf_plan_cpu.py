"""The stream-K plan of the bf16 / fp16 bits GEMM without a GPU: the properties of the host model (tests/xf_plan_ref.py) that the
kernel's slab contract rests on, the model against the library's slot query (bmf_xf_bits_slots, which plans for 256 compute units when
no device answers), and the case table of tests/test_xf_bits_slabs_gpu.py re-derived on 256 compute units."""
import collections

import pytest

import xf_plan_ref as R

TILES = range(1, 8)
STAGES = list(range(1, 41)) + [100, 101, 193, 641]
CUS = (1, 4, 104, 256, 304)


@pytest.mark.parametrize("cus", CUS)
def test_model_properties(cus):
    for tiles in TILES:
        for stages in STAGES:
            p = R.plan(R.TILE_ROWS * tiles, stages, cus)
            what = (tiles, stages, cus)
            assert p.total == tiles * stages and 1 <= p.num_wgs <= min(cus, p.total), what
            assert (p.num_wgs - 1) * p.units_per_wg < p.total <= p.num_wgs * p.units_per_wg, what       # equal slices, no idle workgroup
            assert p.units_per_wg == 1 or (p.units_per_wg - 1) * cus < p.total, what                    # and no longer than they must be
            segs = R.segments(p)
            # every unit is covered exactly once
            units = sorted(s.tile * stages + st for s in segs for st in range(s.s0, s.s1))
            assert units == list(range(p.total)), what
            assert all(0 <= s.s0 < s.s1 <= stages and 0 <= s.tile < tiles and s.is_last == (s.s1 == stages) for s in segs), what
            # a workgroup's pieces are consecutive units: at most units_per_wg of them, each new piece at the start of the next tile
            for wg, v in R.by_wg(segs).items():
                assert sum(s.s1 - s.s0 for s in v) <= p.units_per_wg, what
                assert v[0].tile * stages + v[0].s0 == wg * p.units_per_wg, what
                assert all(a.is_last and b.s0 == 0 and b.tile == a.tile + 1 for a, b in zip(v, v[1:])), what
            # slots: inside the slab array, no two pieces on one (tile, slot), consecutive from 0 in stage order
            assert all(0 <= s.slot < p.slots for s in segs), what
            assert len({(s.tile, s.slot) for s in segs}) == len(segs), what
            per_tile = collections.defaultdict(list)
            for s in segs:
                per_tile[s.tile].append(s)
            assert sorted(per_tile) == list(range(tiles)), what
            for v in per_tile.values():
                v.sort(key=lambda s: s.s0)
                assert [s.slot for s in v] == list(range(len(v))), what
                assert v[0].s0 == 0 and v[-1].is_last and all(a.s1 == b.s0 for a, b in zip(v, v[1:])), what
                assert [s.is_last for s in v] == [False] * (len(v) - 1) + [True], what                  # one zero-filler per tile: the last slot
            assert p.slots == max(len(v) for v in per_tile.values()), what
            # the kernel's closed form of the slot: workgroup minus the workgroup that holds the tile's first unit
            assert all(s.slot == s.wg - (s.tile * stages) // p.units_per_wg for s in segs), what


def no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def test_library_slots_equal_the_model_on_256_compute_units():
    """Without a device the library plans for 256 compute units: its slot count over the sweep, for every panel form, and at the
    headline launch (100352 rows x 640 words)."""
    no_gpu()
    from pybmf_amd import _lib as L
    for tiles in TILES:
        for stages in STAGES:
            want = R.plan(R.TILE_ROWS * tiles, stages, 256).slots
            for terms in (1, 2, 3):
                for kp in (32, 64):
                    assert L.lib.bmf_xf_bits_slots(R.TILE_ROWS * tiles, 4 * stages, terms, kp) == want, (tiles, stages, terms, kp)
    for rows_pad, words in ((100352, 640), (20480, 3136)):
        want = R.plan(rows_pad, words // 4, 256)
        assert L.lib.bmf_xf_bits_slots(rows_pad, words, 2, 64) == want.slots, (rows_pad, words)
    # 196 tiles x 160 stages on 256 workgroups: 123 units each, 255 workgroups, a tile of 160 stages meets at most 3 of them
    h = R.plan(100352, 160, 256)
    assert (h.total, h.units_per_wg, h.num_wgs, h.slots) == (31360, 123, 255, 3)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case_table_on_256_compute_units(case):
    p = R.plan(case.rows_pad, case.stages, 256)
    segs = R.segments(p)
    assert (p.units_per_wg, p.num_wgs, p.slots, R.piece_lengths(segs)) == case.at256
    case.prop(p, segs)


def test_engine_rows_with_a_live_pipeline():
    """the two rows of test_medium_odd_shapes_many_row_tiles whose 16-bit launches have multi-stage slices on 256 compute units:
    2999 x 12901 -> 6 tiles x 104 stages (padded 3072 x 13312) and 26 tiles x 24 stages the other way"""
    a, b = R.plan(3072, 104, 256), R.plan(13312, 24, 256)
    assert (a.total, a.units_per_wg) == (624, 3) and (b.total, b.units_per_wg) == (624, 3)
    crossing = [sum(1 for v in R.by_wg(R.segments(p)).values() if len(v) > 1) for p in (a, b)]
    assert crossing == [4, 0]              # X V: four slices end one tile and start the next; X^T U: 24 = 8 slices of 3, none does
    # and the rows that were there before: one stage per slice
    for rows_pad, stages in ((5120, 24), (3072, 40), (9216, 9)):
        assert R.plan(rows_pad, stages, 256).units_per_wg == 1
