"""The stream-K plan of the int8 bits GEMM (build_plan_i8 in csrc/xf_bits_i8.hip), restated in plain Python (not imported), and what a
test needs to know from a plan: where every slice starts and ends, which slices meet a row tile, which slab slot a slice writes.
tests/test_i8_plan_cpu.py checks the library's query (bmf_xf_bits_i8_plan) against this restatement field by field;
tests/test_xf_bits_i8_slabs_gpu.py takes the slice bounds from the QUERY and uses only the helpers below the restatement.

The rule.  A unit is (row tile, stage): stage = 128 reduction indices, `stages` per tile, total = tiles * stages, cut in whole groups of
four stages.  gsz = workgroups per column half that are resident at once (two per CU with the default kernel, at most 512).
  * groups >= 4 gsz (and gsz % 16 == 0, two workgroups per CU): two lengths.  The first workgroup of a CU takes 66 % of the CU's work:
    g_big = int(0.66 * 2 * groups / gsz + 0.999) groups per big slice, n_big = min(gsz / 2, ceil(groups / g_big)) of them; the rest is
    shared by the other gsz / 2 workgroups, g_small = ceil(rest / (gsz / 2)) groups each.
  * otherwise: equal slices of g = ceil(groups / min(gsz, groups)) groups.
  * slots = the largest number of slices that meet one row tile.
  * the slice map: the slices of a class, sorted (stably) by the stage they start at -- the small class `lead` = 50 % of u_big - u_small
    stages earlier -- are dealt to the 8 XCD runs b0 + x, b0 + x + 8, ... in turn; big slices onto block slices [0, gsz / 2), small ones onto
    [gsz / 2, gsz), equal slices onto [0, ceil(n_slices / 8) * 8).
  * grid = (last mapped block slice / 8 + 1) * 8 * halves."""
import collections

SHARE = 0.66          # of a CU's work to the first of its two workgroups
LEAD_PERCENT = 50     # of u_big - u_small
NONE = 0xFFFF

Plan = collections.namedtuple("Plan", "n_slices grid n_big u_big u_small slots halves tile_rows total perm")


def variant_of(ncols, kp, variant):
    """the kernel variant a launch over `ncols` columns of a kp-wide factor runs on (bmf_i8_use_wide)"""
    return variant if (ncols == 64 and kp == 64) else 0


def plan(rows_pad, red_words, ncols, cus, wide=0):
    """build_plan_i8(rows_pad, stages = red_words / 4, ncols, cus, wide), as a Plan"""
    stages = red_words // 4
    halves = 1 if (wide and wide != 4) else ncols // 32
    wg_per_cu = 1 if wide else 2
    tile_rows = 512 if wide in (3, 4) else 256
    tiles = rows_pad // tile_rows
    total = tiles * stages
    gsz = min(wg_per_cu * cus // halves, 512)
    groups = total // 4
    n_old = gsz // 2
    if wg_per_cu == 2 and gsz % 16 == 0 and groups >= 4 * gsz:
        g_big = int(SHARE * 2.0 * float(groups) / float(gsz) + 0.999)
        n_big = min(n_old, -(-groups // g_big))
        rest = groups - min(groups, n_big * g_big)
        g_small = max(1, -(-rest // (gsz - n_old)))
        u_big, u_small = 4 * g_big, 4 * g_small
        n_slices = n_big + -(-rest // g_small)
    else:
        gsz = min(gsz, groups)
        g = -(-groups // gsz)
        n_big, u_big, u_small = 0, 4 * g, 4 * g
        n_slices = -(-groups // g)
    big_end = n_big * u_big

    def start_of(s):
        return s * u_big if s < n_big else big_end + (s - n_big) * u_small

    def slice_of(u):
        return u // u_big if u < big_end else n_big + (u - big_end) // u_small

    slots = max([1] + [slice_of((t + 1) * stages - 1) - slice_of(t * stages) + 1 for t in range(tiles)])
    perm = [NONE] * 512

    def deal(l0, l1, b0, b1, lead):
        order = sorted(range(l0, l1), key=lambda s: (start_of(s) - lead) % stages)   # (sorted is stable, % is non-negative)
        j = 0
        for x in range(8):
            for b in range(b0 + x, b1, 8):
                if j < len(order):
                    perm[b] = order[j]
                    j += 1

    if n_big > 0:
        deal(0, n_big, 0, n_old, 0)
        deal(n_big, n_slices, n_old, gsz, (u_big - u_small) * LEAD_PERCENT // 100)
    else:
        deal(0, n_slices, 0, (n_slices + 7) // 8 * 8, 0)
    last = max([0] + [b for b in range(512) if perm[b] != NONE])
    grid = (last // 8 + 1) * 8 * halves
    return Plan(n_slices, grid, n_big, u_big, u_small, slots, halves, tile_rows, total, tuple(perm))


def query(lib, rows_pad, red_words, ncols, kp, cus):
    """bmf_xf_bits_i8_plan as a Plan (cus = 0: the current device's compute units), or None when the call is refused"""
    import ctypes as C
    f = (C.c_int32 * 8)(*([-7] * 8))
    total = C.c_int64(-7)
    perm = (C.c_uint16 * 512)(*([7] * 512))
    rc = lib.bmf_xf_bits_i8_plan(rows_pad, red_words, ncols, kp, cus, f, C.byref(total), perm)
    if rc != 0:
        assert rc == -1 and list(f) == [-7] * 8 and total.value == -7 and list(perm) == [7] * 512   # a refused call writes nothing
        return None
    return Plan(*list(f), total.value, tuple(perm))


# ------------------------------------------------------------------------------------------------------------------------------
# reading a plan (the library's or the restatement's): slice bounds, the slices of a tile, the slab slot of a slice
# ------------------------------------------------------------------------------------------------------------------------------
def slice_bounds(p):
    """[(u0, u1)] of the logical slices, the last one clipped by total"""
    out = []
    big_end = p.n_big * p.u_big
    for s in range(p.n_slices):
        u0 = s * p.u_big if s < p.n_big else big_end + (s - p.n_big) * p.u_small
        out.append((u0, min(u0 + (p.u_big if s < p.n_big else p.u_small), p.total)))
    return out


def tile_pieces(p, stages):
    """{tile: [(slice, stage0, stage1)]}: the slices that meet the tile, in order, each with the stage range of the tile it covers.  A
    slice writes its partial sum of the tile into slab slot (slice - the first slice of the tile)."""
    bounds = slice_bounds(p)
    out, s = {}, 0
    for t in range(p.total // stages):
        a, b = t * stages, (t + 1) * stages
        while bounds[s][1] <= a:
            s += 1
        meet, q = [], s
        while q < len(bounds) and bounds[q][0] < b:
            meet.append((q, max(bounds[q][0], a) - a, min(bounds[q][1], b) - a))
            q += 1
        out[t] = meet
    return out
