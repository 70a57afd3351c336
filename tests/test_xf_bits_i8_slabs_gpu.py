"""xf_bits_i8_kernel (csrc/xf_bits_i8.hip, the default int8 bits GEMM) slab by slab, bit for bit, on every kind of stream-K plan.

The per-slab contract: slice s of the plan writes, for every 256-row tile it meets, the sum over ITS stages of the tile into slab slot
s - (first slice of the tile); the slice that holds the tile's last stage zero-fills every slot behind its own up to `splits`; a slab
value is float32(float64(v) * float64(colscale)) with v the exact integer sum and colscale a power of two -- one rounding, so the
comparison is on bit patterns, with no tolerance.

The reference takes nothing from the quantiser: the integers Q = sum_l 256^l plane_l are read back from the device planes
(un-permuted with bmf_panel_pos_i8), colscale from scale[kp:].  Slices are whole groups of four stages = whole 512-index blocks of the
reduction, so the host computes the exact products per (row, 512-block, column) once (fp64 BLAS on integers below 2^32: exact) and
every slab is a difference of two entries of their running sum.  Slice bounds come from the library's plan query (bmf_xf_bits_i8_plan on
the current device); every case first asserts the plan property it is named for and FAILS when the device gives another plan.

`out` is pre-filled with a marker and has guard elements in front of it, behind it and between the slabs; all inputs must come back byte
for byte.  Every whole-factor case passes one slab more than the plan needs: the surplus slot is zero-filled like any other slot behind
a tile's last contributor (the header's "surplus slabs are written as zeros"; callers add up all `splits` slabs), so the marker survives
only in the guards and in the columns a column-block launch does not own.  The shapes in the tables are for 256 compute units; row
counts are padded to 512 as the launcher demands (1280 -> 1536: a last tile of padding rows only; 256 -> 512).
"""
import functools
import time

import numpy as np
import pytest

import i8_plan_ref as R

pytestmark = pytest.mark.gpu

MARK = -7
GUARD = 16            # floats: keeps the 16-byte alignment the launch asks for
MARK_WORD = 0xF9F9F9F9


@pytest.fixture(scope="module")
def L():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    assert _lib.lib.bmf_xf_bits_i8_variant(0) >= 0
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def pad512(x):
    return -(-x // 512) * 512


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def make_bits(rows, red):
    """(rows_pad, red / 8) uint8, little-endian bit order: random bits of density 1 / 8 (every tile and every 512-block holds ones),
    all-ones rows, all-zero rows, rows with a single one that walk through the positions of a 512-block, zero padding rows"""
    rows_pad = pad512(rows)
    rng = np.random.default_rng(rows * 7 + red)
    shape = (rows_pad, red // 8)
    bits = rng.integers(0, 256, shape, dtype=np.uint8) & rng.integers(0, 256, shape, dtype=np.uint8) & rng.integers(0, 256, shape, dtype=np.uint8)
    nb = red // 512
    ones = sorted({0, 257 % rows, 3 * rows // 4 + 3, rows - 1})
    zeros = sorted({1, 255, 256 % rows, rows - 2} - set(ones))
    bits[ones] = 255
    bits[zeros] = 0
    n1 = 512 if rows >= 2048 else 128            # single-one rows: every position of a block, or every fourth (+ 0..3) in a tiny matrix
    stride = 512 // n1
    r0 = min(300, rows // 4)
    assert r0 + n1 <= rows and not (set(range(r0, r0 + n1)) & (set(ones) | set(zeros)))
    i = np.arange(n1)
    idx = (i % nb) * 512 + i * stride + (i // (n1 // stride) if stride > 1 else 0)
    assert len(set((idx % 512).tolist())) == n1
    bits[r0:r0 + n1] = 0
    bits[r0 + i, idx // 8] = (1 << (idx % 8)).astype(np.uint8)
    bits[rows:] = 0
    return bits


def make_factor(red, kp, seed):
    """red x kp fp64: columns over 12 decades, a negative column, a half-zero column (as test_xf_bits_i8_is_exact)"""
    rs = np.random.RandomState(seed)
    F = np.abs(rs.standard_normal((red, kp))) * 10.0 ** rs.uniform(-3, 0, (red, kp))
    F *= (10.0 ** rs.uniform(-9, 3, kp))[None, :]
    F[:, 1] *= -1.0
    F[: red // 2, 2] = 0.0
    F[:, 35 % kp] *= -1.0
    return F


def panel_positions(L, n):
    pos = np.array([L.lib.bmf_panel_pos_i8(i) for i in range(512)])
    assert sorted(pos.tolist()) == list(range(512))
    r = np.arange(n)
    return (r // 512) * 512 + pos[r % 512]


def planes_to_int(L, planes, red):
    """Q[c][j] = sum_l 256^l plane_l[c][position of j]: (kp, red) int64 from host planes (limbs, kp, >= red)"""
    idx = panel_positions(L, red)
    q = np.zeros(planes.shape[1:2] + (red,), dtype=np.int64)
    for l in range(planes.shape[0]):
        q += planes[l][:, idx].astype(np.int64) << (8 * l)
    return q


def build_panel(L, F64, kp, limbs, ldp=None):
    """device planes (limbs, kp, ldp) int8 of F64 by the stand-alone builder, marker in the bytes past the reduction; its scale (2 kp)"""
    import torch
    red = F64.shape[0]
    ldp = red if ldp is None else ldp
    panel = torch.full((limbs, kp, ldp), MARK, dtype=torch.int8, device="cuda:0")
    scale = torch.zeros(2 * kp, dtype=torch.float32, device="cuda:0")
    ws = torch.zeros(red // 128 * kp, dtype=torch.float32, device="cuda:0")
    F64d, F32d = dev(F64), dev(F64.astype(np.float32))                        # (held until the launches have run)
    L.check(L.lib.bmf_make_panel_i8(L.ptr(F64d), L.ptr(F32d), red, kp, kp, limbs, L.ptr(panel), ldp, L.ptr(ws), L.ptr(scale), None))
    torch.cuda.synchronize()
    assert (panel[:, :, red:] == MARK).all()
    return panel, scale


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def block_sums(bits, Q):
    """S[r][b][c] = sum over the first b 512-blocks of sum_j X[r][j] Q[c][j]: (rows_pad, blocks + 1, kp) int64, exact"""
    rows_pad, nb, kp = bits.shape[0], bits.shape[1] // 64, Q.shape[0]
    assert np.abs(Q).max() * 512 < 2 ** 52
    S = np.zeros((rows_pad, nb + 1, kp), dtype=np.int64)
    Qf = Q.astype(np.float64)
    for r0 in range(0, rows_pad, 16384):
        r1 = min(r0 + 16384, rows_pad)
        for b in range(nb):
            xb = np.unpackbits(bits[r0:r1, 64 * b:64 * (b + 1)], axis=1, bitorder="little").astype(np.float64)
            S[r0:r1, b + 1] = np.rint(xb @ Qf[:, 512 * b:512 * (b + 1)].T).astype(np.int64)
    np.cumsum(S, axis=1, out=S)
    return S


def expected_slabs(S, plan, stages, colscale, col0, ncols, splits):
    """(splits, rows_pad, ncols) float32: every slab slot of every tile for the columns [col0, col0 + ncols) of one launch under `plan`"""
    rows_pad = S.shape[0]
    want = np.zeros((splits, rows_pad, ncols), dtype=np.float32)          # slots behind a tile's last contributor: +0.0
    cs = colscale[col0:col0 + ncols].astype(np.float64)[None, :]
    assert plan.tile_rows == 256 and plan.total == rows_pad // 256 * stages and plan.slots <= splits
    for t, pieces in R.tile_pieces(plan, stages).items():
        rows = slice(256 * t, 256 * (t + 1))
        assert len(pieces) <= plan.slots and pieces[0][1] == 0 and pieces[-1][2] == stages
        whole = np.zeros((256, ncols), dtype=np.int64)
        for s, s0, s1 in pieces:
            assert s0 % 4 == 0 and s1 % 4 == 0 and s1 > s0
            v = S[rows, s1 // 4, col0:col0 + ncols] - S[rows, s0 // 4, col0:col0 + ncols]
            want[s - pieces[0][0], rows] = (v.astype(np.float64) * cs).astype(np.float32)
            whole += v
        assert np.array_equal(whole, S[rows, -1, col0:col0 + ncols])          # whatever the cut, the integer slabs of a tile add up to its product
    return want


class Problem:
    """X bits (plain with leading dimension ldw, and tiled), the planes of a factor, and the reference sums; everything on the device
    once, with host copies to prove that a launch left its inputs alone"""

    def __init__(self, L, rows, red, kp, limbs, ldw=None, ldp=None, seed=5, planes=None):
        import torch
        self.L, self.rows, self.red, self.kp, self.limbs = L, rows, red, kp, limbs
        self.rows_pad, self.red_words, self.stages = pad512(rows), red // 32, red // 128
        self.ldw = self.red_words if ldw is None else ldw
        self.ldp = red if ldp is None else ldp
        t0 = time.time()
        bits = make_bits(rows, red)
        words = np.full((self.rows_pad, self.ldw), MARK_WORD, dtype=np.uint32)
        words[:, :self.red_words] = bits.view(np.uint32)
        self.bits = dev(words.view(np.int32))
        self.tiled = torch.full((self.rows_pad * self.red_words,), MARK, dtype=torch.int32, device="cuda:0")
        L.check(L.lib.bmf_tile_bits(L.ptr(self.bits), self.rows_pad, self.ldw, self.red_words, L.ptr(self.tiled), None))
        want_tiled = words[:, :self.red_words].reshape(self.rows_pad // 256, 256, self.red_words // 16, 16).transpose(0, 2, 1, 3)
        assert np.array_equal(self.tiled.cpu().numpy().view(np.uint32), want_tiled.ravel())
        if planes is None:
            self.panel, self.scale = build_panel(L, make_factor(red, kp, seed), kp, limbs, self.ldp)
        else:                                                                 # planes and colscale that something else built
            self.panel = torch.full((limbs, kp, self.ldp), MARK, dtype=torch.int8, device="cuda:0")
            self.panel[:, :, :red] = dev(planes[0])
            self.scale = dev(np.concatenate([np.zeros(kp, np.float32), planes[1]]))
        self.colscale = self.scale[kp:].cpu().numpy()
        fr, _ = np.frexp(self.colscale)
        assert (fr == 0.5).all()                                             # powers of two: the slab contract is bit-exact
        self.Q = planes_to_int(L, self.panel.cpu().numpy(), red)
        if planes is None:                                                    # the factor's columns arrived as they were made
            top = np.abs(self.Q).max(axis=1)
            assert (self.Q[1] <= 0).all() and (self.Q[0] >= 0).all() and not self.Q[2, :red // 2].any() and self.Q[2, red // 2:].any()
            assert (top >= (2 ** 21 if limbs == 3 else 2 ** 13)).all() and (top <= (8355711 if limbs == 3 else 32639)).all()
        self.S = block_sums(bits, self.Q)
        self.host_seconds = time.time() - t0
        assert not self.S[rows:].any()
        occupied = bits.reshape(self.rows_pad // 256, 256, red // 512, 64).any(axis=(1, 3))
        assert occupied[: -(-rows // 256)].all()                              # ones in every 512-block of every tile that holds real rows
        self.stop = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        self.inputs = {"bits": self.bits, "tiled": self.tiled, "panel": self.panel, "scale": self.scale, "stop": self.stop}
        self.before = {k_: v.cpu().numpy().tobytes() for k_, v in self.inputs.items()}

    def plan(self, ncols):
        p = R.query(self.L.lib, self.rows_pad, self.red_words, ncols, self.kp, 0)
        assert p is not None, self.L.lib.bmf_last_error()
        return p

    def new_out(self, splits):
        """a marked buffer of `splits` slabs, GUARD floats in front, behind and between the slabs"""
        import torch
        self.stride = self.rows_pad * self.kp + GUARD
        self.splits = splits
        return torch.full((GUARD + splits * self.stride,), MARK, dtype=torch.float32, device="cuda:0")

    def launch(self, buf, col0, ncols, tiled, stop=None, expect=0, splits=None, shift=None):
        import torch
        L, sh = self.L, shift or {}
        a = self.tiled if tiled else self.bits
        rc = L.lib.bmf_xf_bits_i8_cols(a.data_ptr() + sh.get("A", 0), self.rows_pad, self.ldw, self.red_words, self.panel.data_ptr() + sh.get("panel", 0), self.ldp,
                                       self.limbs, self.scale.data_ptr() + 4 * self.kp, self.kp, col0, ncols, buf.data_ptr() + 4 * GUARD + sh.get("out", 0),
                                       self.stride, self.splits if splits is None else splits, 1 if tiled else 0,
                                       self.stop.data_ptr() if stop is not None else None, None)
        torch.cuda.synchronize()
        assert rc == expect, (rc, L.lib.bmf_last_error())
        for k_, v in self.inputs.items():
            assert v.cpu().numpy().tobytes() == self.before[k_], f"input {k_} was written"
        host = buf.cpu().numpy()
        assert (host[:GUARD] == MARK).all(), "guard in front of out"
        body = host[GUARD:].reshape(self.splits, self.stride)
        assert (body[:, self.rows_pad * self.kp:] == MARK).all(), "guards between and behind the slabs"
        return body[:, :self.rows_pad * self.kp].reshape(self.splits, self.rows_pad, self.kp)

    def set_stop(self, v):
        self.stop.fill_(v)
        self.before["stop"] = self.stop.cpu().numpy().tobytes()


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


def check_launch(P, got, plan, col0, ncols, untouched=()):
    """every slot of every tile of the launched columns against the reference, bit patterns; `untouched`: column ranges that must
    still hold the marker"""
    want = expected_slabs(P.S, plan, P.stages, P.colscale, col0, ncols, P.splits)
    part = got[:, :, col0:col0 + ncols]
    if not same_bits(part, want):
        bad = np.argwhere(np.ascontiguousarray(part).view(np.int32) != want.view(np.int32))
        s, r, c = bad[0]
        raise AssertionError(f"{len(bad)} slab cells differ; first: slot {s} row {r} (tile {r // 256}) column {col0 + c}: got {part[s, r, c]!r} want {want[s, r, c]!r}")
    assert not part[:, P.rows:].any()                                       # padded rows: zero in every slot
    for a, b in untouched:
        assert (got[:, :, a:b] == MARK).all(), f"columns [{a}, {b}) were written"
    return want


# ------------------------------------------------------------------------------------------------------------------------------
# the plans: what each case is named for, asserted from the query on this device
# ------------------------------------------------------------------------------------------------------------------------------
def per_tile(plan, stages):
    return R.tile_pieces(plan, stages)


def prop_big_through_tiles(p, stages):
    """two lengths, and a big slice is longer than a tile: it runs through tile boundaries in the middle of the pipelined loop"""
    assert p.n_big > 0 and p.u_big > stages
    assert any(sum(1 for v in per_tile(p, stages).values() if any(s == big for s, _, _ in v)) >= 2 for big in range(p.n_big))


def prop_many_per_tile(p, stages):
    """two lengths, 6 to 11 slices per tile, and some tile holds big and small slices"""
    assert p.n_big > 0
    pt = per_tile(p, stages)
    assert all(6 <= len(v) <= 11 for v in pt.values()) and p.slots == 11
    assert any(v[0][0] < p.n_big <= v[-1][0] for v in pt.values())


def prop_two_lengths_512(p, stages):
    """a 32-column launch: one workgroup per slice, two lengths on the 512-slice grid"""
    assert p.n_big > 0 and p.halves == 1 and p.n_slices > 256 and p.u_big > p.u_small


def prop_equal_g2(p, stages):
    """equal slices of two groups that straddle tiles"""
    assert p.n_big == 0 and p.u_big == p.u_small == 8
    bounds = R.slice_bounds(p)
    assert any(u0 // stages != (u1 - 1) // stages for u0, u1 in bounds)


def prop_three_tiles(p, stages):
    """equal slices, each three whole tiles long"""
    assert p.n_big == 0 and p.u_small == 3 * stages and p.slots == 1


def prop_small_equal(p, stages):
    """equal slices of one group, several per tile"""
    assert p.n_big == 0 and p.u_small == 4 and p.n_slices == p.total // 4 and p.slots == stages // 4 > 1


def prop_one_group_per_tile(p, stages):
    """the smallest launch there is: rows are padded to 512 = two tiles, so two slices of the one group each tile has (a plan of ONE
    group in all needs 256 rows, which the launcher refuses)"""
    assert p.n_big == 0 and p.u_small == 4 == stages and p.n_slices == 2 and p.slots == 1 and p.total == 8


def prop_clipped(p, stages):
    """equal slices whose last one is clipped by the total"""
    assert p.n_big == 0 and p.n_slices * p.u_small != p.total
    u0, u1 = R.slice_bounds(p)[-1]
    assert 0 < u1 - u0 < p.u_small


#        rows    red    kp  limbs  property
CASES = [(53248, 2560, 64, 3, prop_big_through_tiles),
         (53248, 2560, 64, 2, prop_big_through_tiles),
         (8192, 16896, 64, 3, prop_many_per_tile),
         (8192, 16896, 64, 2, prop_many_per_tile),
         (106496, 2560, 32, 3, prop_two_lengths_512),
         (3072, 20992, 64, 3, prop_equal_g2),
         (153600, 512, 64, 3, prop_three_tiles),
         (1280, 3584, 64, 3, prop_small_equal),
         (1280, 3584, 64, 2, prop_small_equal),
         (256, 512, 32, 3, prop_one_group_per_tile),
         (256, 512, 32, 2, prop_one_group_per_tile),
         (10240, 6656, 64, 3, prop_clipped)]


def report(name, P, plan, slabs):
    print(f"\n[i8 slabs] {name}: rows_pad {P.rows_pad} red {P.red} kp {P.kp} limbs {P.limbs} | n_slices {plan.n_slices} grid {plan.grid} n_big {plan.n_big} "
          f"u_big {plan.u_big} u_small {plan.u_small} slots {plan.slots} total {plan.total} | slabs compared {slabs} | host reference {P.host_seconds:.2f} s")


@pytest.mark.parametrize("rows,red,kp,limbs,prop", CASES, ids=[f"{c[0]}x{c[1]}-kp{c[2]}-l{c[3]}" for c in CASES])
def test_every_slab_of_a_whole_factor_launch(L, rows, red, kp, limbs, prop):
    P = Problem(L, rows, red, kp, limbs)
    plan = P.plan(kp)
    prop(plan, P.stages)
    assert L.lib.bmf_xf_bits_i8_slots(P.rows_pad, P.red_words, kp) == plan.slots
    buf = P.new_out(plan.slots + 1)                 # one slot more than the plan needs: zero-filled like every slot behind the last contributor
    plain = P.launch(buf, 0, kp, tiled=False)
    check_launch(P, plain, plan, 0, kp)
    assert not plain[plan.slots:].any()
    buf.fill_(MARK)
    tiled = P.launch(buf, 0, kp, tiled=True)
    assert same_bits(tiled, plain)                  # the tiled bit matrix: bit-identical slabs
    report(prop.__name__[5:], P, plan, (P.rows_pad // 256) * P.splits)


@pytest.mark.parametrize("rows,red", [(53248, 2560), (1280, 3584)])
def test_column_blocks_of_a_64_wide_factor(L, rows, red):
    """(col0, ncols) = (0, 32) then (32, 32) into one marked buffer, as a row-sharded run launches: each half under the plan of a 32-column
    launch, the other half untouched; and the slot sums of the two forms agree"""
    P = Problem(L, rows, red, 64, 3)
    p32, p64 = P.plan(32), P.plan(64)
    assert p32.halves == 1 and p64.halves == 2
    buf = P.new_out(p32.slots + 1)
    got = P.launch(buf, 0, 32, tiled=True)
    w0 = check_launch(P, got, p32, 0, 32, untouched=[(32, 64)])
    got = P.launch(buf, 32, 32, tiled=True)
    check_launch(P, got, p32, 0, 32)
    w1 = check_launch(P, got, p32, 32, 32)
    halves = got.astype(np.float64).sum(axis=0)
    assert np.array_equal(halves, np.concatenate([w0, w1], axis=2).astype(np.float64).sum(axis=0))
    # the whole-factor launch cuts the same sums differently: its slabs, un-rounded, add up to the same integers
    splits32 = P.splits
    buf = P.new_out(p64.slots)
    whole = P.launch(buf, 0, 64, tiled=True)
    check_launch(P, whole, p64, 0, 64)
    exact = P.S[:, -1].astype(np.float64) * P.colscale.astype(np.float64)[None, :]
    for form, slabs, n in (("halves", halves, splits32), ("whole", whole.astype(np.float64).sum(axis=0), p64.slots)):
        assert np.abs(slabs - exact).max() <= n * 2.0 ** -24 * np.abs(exact).max(), form   # one fp32 rounding per slab
    report("column blocks", P, p32, (P.rows_pad // 256) * (splits32 + p64.slots))


def test_leading_dimensions(L):
    """ldw > red_words and ldp > 32 * red_words: the words and bytes between are marked and come back intact (Problem.launch)"""
    rows, red = 1280, 3584
    P = Problem(L, rows, red, 64, 3, ldw=red // 32 + 4, ldp=red + 16)
    plan = P.plan(64)
    buf = P.new_out(plan.slots)
    plain = P.launch(buf, 0, 64, tiled=False)
    check_launch(P, plain, plan, 0, 64)
    buf.fill_(MARK)
    assert same_bits(P.launch(buf, 0, 64, tiled=True), plain)
    Q = Problem(L, rows, red, 64, 3)                                         # the same problem, tight leading dimensions
    assert np.array_equal(Q.Q, P.Q) and same_bits(Q.launch(Q.new_out(plan.slots), 0, 64, tiled=False), plain)


def test_stop_flag(L):
    P = Problem(L, 1280, 3584, 64, 2)
    plan = P.plan(64)
    buf = P.new_out(plan.slots + 1)
    P.set_stop(1)
    for tiled in (False, True):
        got = P.launch(buf, 0, 64, tiled=tiled, stop=True)
        assert (got == MARK).all()                                            # nothing is written
    P.set_stop(0)
    got = P.launch(buf, 0, 64, tiled=False, stop=True)                      # the same buffers, the flag cleared: the slabs appear
    check_launch(P, got, plan, 0, 64)


def test_refused_launches_write_nothing(L):
    P = Problem(L, 1280, 3584, 64, 3)
    p64, p32 = P.plan(64), P.plan(32)
    assert p64.slots > 1 and p32.slots > 1
    buf = P.new_out(max(p64.slots, p32.slots))
    for kw, msg in ((dict(col0=16, ncols=32), b"column range"), (dict(col0=32, ncols=64), b"column range"), (dict(col0=0, ncols=48), b"column range"),
                    (dict(col0=64, ncols=32), b"column range"), (dict(col0=-32, ncols=32), b"column range"),
                    (dict(col0=0, ncols=64, splits=p64.slots - 1), b"slab slots"), (dict(col0=32, ncols=32, splits=p32.slots - 1), b"slab slots"),
                    (dict(col0=0, ncols=64, shift={"out": 4}), b"aligned"), (dict(col0=0, ncols=64, shift={"A": 4}), b"aligned"),
                    (dict(col0=0, ncols=64, shift={"panel": 1}), b"aligned")):
        got = P.launch(buf, kw["col0"], kw["ncols"], tiled=False, expect=-1, splits=kw.get("splits"), shift=kw.get("shift"))
        assert msg in L.lib.bmf_last_error(), (kw, L.lib.bmf_last_error())
        assert (got == MARK).all(), kw
    check_launch(P, P.launch(buf, 0, 64, tiled=False), p64, 0, 64)            # and the buffers still serve a good launch
