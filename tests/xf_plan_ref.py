"""The stream-K plan of the bf16 / fp16 bits GEMM (xf_bits_kernel in csrc/xf_bits.hip), written from the contract in the kernel's comment
and not from its arithmetic: "the (row tile, stage) space is linearised tile-major and cut into equal contiguous slices, one per
workgroup; a slice may end one tile and start the next; slot = how many workgroups started on that tile before this one".

A unit is (row tile, stage): a tile is 512 rows, a stage is 128 reduction indices, unit u = tile * stages + stage.  One persistent
workgroup per compute unit, never more workgroups than units; every workgroup takes units_per_wg = ceil(total / workgroups)
consecutive units, the last one what is left.  A slice is cut at every tile boundary it crosses into PIECES; a piece (tile, s0, s1)
is one trip of the kernel's slice loop: it restarts the LDS ring, sums the stages [s0, s1) of the tile and writes that sum into slab
`slot` of the tile's rows.  The piece that holds the tile's last stage zero-fills every slot behind its own up to `splits`.

tests/test_xf_plan_cpu.py checks the model's properties and its agreement with the library's bmf_xf_bits_slots;
tests/test_xf_bits_slabs_gpu.py takes every expected slab from segments().  CASES is the table both of them use."""
import collections

TILE_ROWS = 512
STAGE = 128
RING = 3          # LDS buffers of the kernel's stage ring

Plan = collections.namedtuple("Plan", "total units_per_wg num_wgs slots tiles stages cus")
Piece = collections.namedtuple("Piece", "wg tile s0 s1 slot is_last")


def _pieces(tiles, stages, upw, num_wgs):
    """every piece of every slice, in workgroup order; the slot is COUNTED (workgroups met on the tile so far), not computed"""
    total = tiles * stages
    started = [0] * tiles
    for wg in range(num_wgs):
        u, u_end = wg * upw, min((wg + 1) * upw, total)
        while u < u_end:
            tile = u // stages
            s0 = u - tile * stages
            s1 = min(stages, s0 + (u_end - u))
            yield Piece(wg, tile, s0, s1, started[tile], s1 == stages)
            started[tile] += 1
            u += s1 - s0


def plan(rows_pad, stages, cus):
    assert rows_pad > 0 and rows_pad % TILE_ROWS == 0 and stages >= 1 and cus >= 1
    tiles = rows_pad // TILE_ROWS
    total = tiles * stages
    wgs = min(cus, total)
    upw = -(-total // wgs)
    num_wgs = -(-total // upw)
    per_tile = collections.Counter(p.tile for p in _pieces(tiles, stages, upw, num_wgs))
    return Plan(total, upw, num_wgs, max(per_tile.values()), tiles, stages, cus)


def segments(p):
    """(wg, tile, s0, s1, slot, is_last) for every piece of every slice of plan p"""
    return list(_pieces(p.tiles, p.stages, p.units_per_wg, p.num_wgs))


def by_wg(segs):
    out = collections.defaultdict(list)
    for s in segs:
        out[s.wg].append(s)
    return out


def piece_lengths(segs):
    return sorted({s.s1 - s.s0 for s in segs})


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_xf_bits_slabs_gpu.py: what each one is named for, as an assertion on a plan.  The shapes are the smallest
# with the property on 256 compute units.
# ------------------------------------------------------------------------------------------------------------------------------
def prop_single(p, segs):
    """one stage per workgroup: slab s of a tile is its stage s"""
    assert p.units_per_wg == 1 and p.slots == p.stages and p.num_wgs == p.total
    assert all(s.s1 == s.s0 + 1 and s.slot == s.s0 for s in segs)


def prop_pairs(p, segs):
    """two-stage slices and none crosses a tile boundary"""
    assert p.units_per_wg == 2 and piece_lengths(segs) == [2]
    assert all(len(v) == 1 for v in by_wg(segs).values())


def prop_cross2(p, segs):
    """two-stage slices; one ends a tile and starts the next; the last workgroup has one unit left"""
    assert p.units_per_wg == 2 and piece_lengths(segs) == [1, 2]
    w = by_wg(segs)
    crossing = [v for v in w.values() if len(v) == 2]
    assert crossing and all(v[0].is_last and v[1].s0 == 0 and v[1].tile == v[0].tile + 1 and v[1].slot == 0 and v[0].slot > 0 for v in crossing)
    last = w[p.num_wgs - 1]
    assert len(last) == 1 and last[0].s1 - last[0].s0 == 1 and last[0].is_last


def prop_ring(p, segs):
    """four-stage slices: the look-ahead DMA and the first reuse of ring buffer 0, and a slice cut by a tile boundary in every way"""
    assert p.units_per_wg == 4 > RING and piece_lengths(segs) == [1, 2, 3, 4]
    cuts = {(v[0].s1 - v[0].s0, v[1].s1 - v[1].s0) for v in by_wg(segs).values() if len(v) == 2}
    assert cuts == {(1, 3), (2, 2), (3, 1)}


def prop_laps(p, segs):
    """six-stage slices: two full laps of the three-buffer ring, and a crossing slice"""
    assert p.units_per_wg == 2 * RING and piece_lengths(segs) == [1, 4, 5, 6]
    assert any(len(v) == 2 for v in by_wg(segs).values())


Case = collections.namedtuple("Case", "name rows_pad stages prop at256")
#            name      rows_pad stages property     (units_per_wg, num_wgs, slots, piece lengths) on 256 compute units
CASES = [Case("single", 1024, 8, prop_single, (1, 16, 8, [1])),
         Case("pairs", 1536, 100, prop_pairs, (2, 150, 50, [2])),
         Case("cross2", 1536, 101, prop_cross2, (2, 152, 51, [1, 2])),
         Case("ring", 2048, 193, prop_ring, (4, 193, 49, [1, 2, 3, 4])),
         Case("laps", 1024, 641, prop_laps, (6, 214, 108, [1, 4, 5, 6]))]
CASE = {c.name: c for c in CASES}
