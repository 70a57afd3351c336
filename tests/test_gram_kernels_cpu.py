"""tests/gram_ref.py (the bit-for-bit restatements that tests/test_gram_kernels_gpu.py holds the Gram and F . G kernels to) proved on
the host: the fmaf emulation against exact rational arithmetic, the case tables against the restated launch arithmetic, the exact
inputs against their claim that every partial sum is representable, and the chains against the bound.  No GPU.

Mutations of gram_ref.py, each tried against this file and reverted: fma32 as float32(a64 * b64 + c64) fails
test_fma32_is_the_correctly_rounded_fma alone (the hand-made double-rounding triples); `per` as floor instead of ceil fails
test_partition_covers_every_row_pair_once and 46 more; dropping the odd row of a pair in slab_chain fails
test_exact_slabs_are_the_integer_grams, test_exact_cross_slabs_are_the_integer_products and the two bound tests."""
import fractions

import numpy as np
import pytest

import gram_ref as R

F32 = np.float32
GRAM_IDS = [c[0] for c in R.GRAM_CASES]

# what each case of R.GRAM_CASES is there for (tail / trips: of a full wave)
EXPECT = {
    "one_pair_three_idle_waves": dict(per=1, tail=1, trips=0, tail_only=True, clipped=False, idle_wave_in_busy_block=True, idle_blocks=0),
    "tail_loop_only": dict(per=1, tail=1, trips=0, tail_only=True, clipped=False, idle_wave_in_busy_block=True, idle_blocks=0),
    "per5_one_trip_tail1": dict(per=5, tail=1, trips=1, tail_only=False, clipped=False, idle_wave_in_busy_block=False, idle_blocks=0),
    "per6_one_trip_tail2": dict(per=6, tail=2, trips=1, tail_only=False, clipped=False, idle_wave_in_busy_block=False, idle_blocks=0),
    "per7_one_trip_tail3": dict(per=7, tail=3, trips=1, tail_only=False, clipped=False, idle_wave_in_busy_block=False, idle_blocks=0),
    "per9_two_trips_clipped_last_wave": dict(per=9, tail=1, trips=2, tail_only=False, clipped=True, idle_wave_in_busy_block=False,
                                             idle_blocks=0),
    "per4_partial_last_block": dict(per=4, tail=0, trips=1, tail_only=False, clipped=True, idle_wave_in_busy_block=True, idle_blocks=0),
    "48_idle_blocks": dict(per=1, tail=1, trips=0, tail_only=True, clipped=False, idle_wave_in_busy_block=False, idle_blocks=48),
    "per16_four_trips_no_tail": dict(per=16, tail=0, trips=4, tail_only=False, clipped=False, idle_wave_in_busy_block=False, idle_blocks=0),
    "per46_eleven_trips_tail2": dict(per=46, tail=2, trips=11, tail_only=False, clipped=True, idle_wave_in_busy_block=False, idle_blocks=0),
    "960_idle_blocks": dict(per=1, tail=1, trips=0, tail_only=True, clipped=False, idle_wave_in_busy_block=False, idle_blocks=960),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused multiply-add
# ---------------------------------------------------------------------------------------------------------------------------------------
def fma_triples():
    rs = np.random.RandomState(0)
    n = 3000
    a = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 21, n)).astype(F32)
    b = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 21, n)).astype(F32)
    p = a.astype(np.float64) * b.astype(np.float64)
    gap = rs.randint(20, 31, n) * rs.choice([-1, 1], n)            # the addend 2^20 .. 2^30 above or below the product
    c = (p * 2.0 ** gap * rs.choice([-1, 1], n) * rs.uniform(1, 2, n)).astype(F32)
    near = slice(0, 600)                                           # and a share at the product's own size, either sign: cancellation
    c[near] = (-p[near] * (1 + rs.standard_normal(600) * 2.0 ** rs.randint(-24, 1, 600))).astype(F32)
    # hand-made: a b + c a hair to either side of an fp32 tie, the hair below the last bit of the fp64 sum
    one, eps = F32(1), F32(2.0 ** -23)
    hand = []
    for big in (F32(2.0 ** 30), F32(2.0 ** 30 + 2.0 ** 7), F32(-(2.0 ** 30)), F32(-(2.0 ** 30 + 2.0 ** 7))):
        for s in (1, -1):
            hand.append((F32(s * 64) * (one + eps), one - eps, big))     # +-(64 - 2^-40): just inside the tie at big +- 64
            hand.append((F32(s * 64) * (one + eps), one + eps, big))     # +-(64 + 2^-16 + 2^-40): just outside
            hand.append((F32(s * 64), one, big))                          # the tie itself
    # exact ties with nothing lost, zeros and signed zeros
    hand += [(one + F32(2.0 ** -12), one + F32(2.0 ** -12), F32(0)), (F32(3), F32(2.0 ** -24), one), (F32(0), F32(5), F32(-0.0)),
             (F32(-0.0), F32(5), F32(0)), (F32(2), F32(3), F32(-6)), (F32(2.0 ** -70), F32(2.0 ** -70), F32(2.0 ** -149))]
    ha, hb, hc = (np.array(x, F32) for x in zip(*hand))
    return np.concatenate([a, ha]), np.concatenate([b, hb]), np.concatenate([c, hc]), n


def test_fma32_is_the_correctly_rounded_fma():
    a, b, c, n = fma_triples()
    got = R.fma32(a, b, c)
    Fr = fractions.Fraction
    want = np.array([R.round_fraction_f32(Fr(float(x)) * Fr(float(y)) + Fr(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert got.dtype == F32 and np.array_equal(got, want) and np.isfinite(got).all()
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    # the triples tell the emulation from the twice-rounded form: among the hand-made ones at least four differ
    assert (naive[n:] != want[n:]).sum() >= 4
    # scalars and broadcasting keep their shape
    assert R.fma32(F32(2), F32(3), F32(1)).shape == () and R.fma32(a[:4, None], b[None, :5], c[:4, None]).shape == (4, 5)


def test_round_fraction_is_round_to_nearest_even():
    Fr = fractions.Fraction
    for x, want in ((Fr(1) + Fr(1, 2 ** 24), 1.0), (Fr(1) + Fr(3, 2 ** 24), 1 + 2.0 ** -22), (Fr(1) + Fr(1, 2 ** 24) + Fr(1, 2 ** 80), 1 + 2.0 ** -23),
                    (Fr(-3, 2 ** 150), -(2.0 ** -148)), (Fr(1, 2 ** 150), 0.0), (Fr(2 ** 24 + 1), 2.0 ** 24), (Fr(1, 3), float(F32(1 / 3)))):
        assert float(R.round_fraction_f32(x)) == want, x


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch arithmetic and the case tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def all_launches():
    return [(r, b) for _, r, b in R.GRAM_CASES] + [(r, b) for r in R.CROSS_ROWS for b in R.CROSS_BLOCKS]


@pytest.mark.parametrize("rows_pad,blocks", all_launches())
def test_partition_covers_every_row_pair_once(rows_pad, blocks):
    pairs, per, ranges = R.partition(rows_pad, blocks)
    assert pairs == rows_pad // 2 and len(ranges) == 4 * blocks and (per - 1) * 4 * blocks < pairs <= per * 4 * blocks
    seen = np.zeros(pairs, np.int64)
    for gw, (p0, p1) in enumerate(ranges):
        assert p0 == gw * per and 0 <= p1 - p0 <= per and p1 <= max(pairs, p0)
        seen[p0:p1] += 1
    assert (seen == 1).all()
    # the rows of a slab are those of its four waves, and owner_block agrees
    for b in sorted({0, 1, blocks // 2, blocks - 1} & set(range(blocks))):
        r0, r1 = R.block_rows(b, rows_pad, blocks)
        own = [r for p0, p1 in ranges[4 * b:4 * b + 4] for r in range(2 * p0, 2 * p1)]
        assert own == list(range(r0, r1))
        assert all(R.owner_block(r, rows_pad, blocks) == b for r in own)


@pytest.mark.parametrize("name,rows_pad,blocks", R.GRAM_CASES, ids=GRAM_IDS)
def test_every_case_is_what_its_name_says(name, rows_pad, blocks):
    assert R.describe(rows_pad, blocks) == EXPECT[name]


def test_the_cases_reach_every_path():
    d = [R.describe(r, b) for _, r, b in R.GRAM_CASES]
    assert [c[1:] for c in R.GRAM_CASES] == [(2, 1), (6, 1), (80, 2), (96, 2), (112, 2), (134, 2), (130, 5), (128, 64), (384, 3), (2560, 7),
                                             (512, 1024)]
    assert {x["tail"] for x in d} == {0, 1, 2, 3}
    assert {x["tail"] for x in d if x["trips"] >= 1} == {0, 1, 2, 3}          # every tail length behind an unrolled trip
    assert any(x["tail_only"] for x in d) and any(x["trips"] >= 2 for x in d)
    assert any(x["trips"] >= 1 and x["tail"] == 0 for x in d)                # the tail loop not entered at all
    assert any(x["clipped"] for x in d) and any(x["idle_wave_in_busy_block"] for x in d)
    assert sorted(x["idle_blocks"] for x in d if x["idle_blocks"]) == [48, 960]
    # bmf_gram_cross: single pairs, clipped waves, idle waves and idle blocks all occur in the grid
    c = [R.describe(r, b) for r in R.CROSS_ROWS for b in R.CROSS_BLOCKS]
    assert any(x["clipped"] for x in c) and any(x["idle_wave_in_busy_block"] for x in c) and any(x["idle_blocks"] > 900 for x in c)
    assert any(x["per"] == 1 for x in c) and any(x["per"] >= 320 for x in c)
    assert R.FG_ROWS == [128, 384, 1664] and all(r % 128 == 0 for r in R.FG_ROWS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def assert_partials_representable(iA, eA, iB, eB, rows_pad, blocks):
    """every prefix of every wave chain, every wave sum and both steps of the slab sum: integers below 2^24 times 2^(e_i + e_j), with
    the exponent inside the normal range -- so each is an fp32 number and no rounding ever happens, in any order"""
    _, _, ranges = R.partition(rows_pad, blocks)
    worst = 0
    for b in range(blocks):
        sums = []
        for p0, p1 in ranges[4 * b:4 * b + 4]:
            rows = slice(2 * p0, 2 * p1)
            pre = np.cumsum(iA[rows, :, None] * iB[rows, None, :], axis=0)
            worst = max(worst, int(np.abs(pre).max()) if pre.size else 0)
            sums.append(pre[-1] if pre.size else np.zeros(pre.shape[1:], np.int64))
        if not any(p1 > p0 for p0, p1 in ranges[4 * b:4 * b + 4]):
            break                                                             # (idle from here on)
        for s in (sums[0] + sums[1], sums[2] + sums[3], sum(sums)):
            worst = max(worst, int(np.abs(s).max()))
    assert worst < 2 ** 24
    e = eA[:, None] + eB[None, :]
    assert e.min() >= -126 and e.max() + 24 <= 127


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name,rows_pad,blocks", R.GRAM_CASES, ids=GRAM_IDS)
def test_exact_factor_is_what_it_claims(name, rows_pad, blocks, kp):
    F, ints, e, tracers = R.exact_factor(rows_pad, kp, blocks)
    assert np.abs(ints).max() <= 7 and e.min() == -20 and e.max() == 10 and len(set(e)) >= 16
    assert not ints[:, R.ZERO_COL].any() and not F[:, R.ZERO_COL].any()
    _, _, ranges = R.partition(rows_pad, blocks)
    edges = {r for p0, p1 in ranges if p1 > p0 for r in (2 * p0, 2 * p1 - 1)}
    assert tracers and len({c for c, _ in tracers}) == len(tracers) and R.ZERO_COL not in {c for c, _ in tracers}
    for c, r in tracers:
        assert r in edges and np.flatnonzero(ints[:, c]).tolist() == [r]
    rows = [r for _, r in tracers]
    assert 0 in rows and rows_pad - 1 in rows                                  # the first row of all and the last (clipped) wave's last
    if blocks > 1 and rows_pad >= 16:
        assert {R.owner_block(r, rows_pad, blocks) for r in rows} >= {0, 1}    # both sides of the seam between slab 0 and slab 1
    assert_partials_representable(ints, e, ints, e, rows_pad, blocks)


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name,rows_pad,blocks", R.GRAM_CASES, ids=GRAM_IDS)
def test_exact_slabs_are_the_integer_grams(name, rows_pad, blocks, kp):
    F, want, ref64, mag, tracers = R.gram_reference("exact", rows_pad, blocks, kp)
    got = R.slab_chain(F, F, rows_pad, blocks, kp)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(want[:len(ref64)].astype(np.float64), ref64) and not bits(want[len(ref64):]).any()
    assert np.array_equal(bits(got), bits(got.transpose(0, 2, 1)))
    for c, r in tracers:                                                       # a tracer names the slab that owns its row
        assert np.flatnonzero(got[:, c, c]).tolist() == [R.owner_block(r, rows_pad, blocks)]
    # any other order gives the same bits: the rows of every wave backwards
    assert np.array_equal(bits(R.slab_chain(F[::-1], F[::-1], rows_pad, 1, kp).sum(0)), bits(got.astype(np.float64).sum(0).astype(F32)))


@pytest.mark.parametrize("same", [True, False], ids=["A_is_B", "A_not_B"])
@pytest.mark.parametrize("blocks", R.CROSS_BLOCKS)
@pytest.mark.parametrize("rows_pad", R.CROSS_ROWS)
def test_exact_cross_slabs_are_the_integer_products(rows_pad, blocks, same):
    A, iA, eA, tracers = R.exact_factor(rows_pad, R.BK, blocks, 5)
    B, iB, eB, _ = (A, iA, eA, tracers) if same else R.exact_factor(rows_pad, R.BK, blocks, 6)
    assert_partials_representable(iA, eA, iB, eB, rows_pad, blocks)
    _, _, want, ref64, _, _ = R.cross_reference("exact", rows_pad, blocks, same)
    got = R.slab_chain(A, B, rows_pad, blocks, R.BK)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(want[:len(ref64)].astype(np.float64), ref64)
    for c, r in tracers:
        assert np.flatnonzero(got[:, c, c]).tolist() == [R.owner_block(r, rows_pad, blocks)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows_pad", R.FG_ROWS)
def test_exact_fg_is_the_integer_product(rows_pad, accumulate):
    F, G, O, iF, iG, iO, d = R.exact_fg(rows_pad)
    order = [k for s in range(32) for k in (s, 32 + s)]
    pre = np.cumsum(iF[:, order, None] * iG[None, order, :], axis=1)           # every prefix of the chain, in the kernel's order
    assert np.abs(pre).max() + 7 < 2 ** 24 and not F[:, R.ZERO_COL].any() and not G[:, R.ZERO_COL].any()
    e = np.log2(np.abs(G[G != 0]) / np.abs(iG[G != 0]))
    assert e.min() >= -30 and e.max() <= 30
    _, _, _, want, ref64, _ = R.fg_reference("exact", rows_pad, accumulate)
    got = R.fg_chain(F, G, O if accumulate else None)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(want.astype(np.float64), ref64)
    assert np.array_equal(bits(R.fg_chain(F[:, ::-1].copy(), G[::-1].copy(), O if accumulate else None)), bits(want))   # any order


# ---------------------------------------------------------------------------------------------------------------------------------------
# mixed inputs: the chains against fp64
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mixed_factor_is_what_it_claims():
    for rows_pad, kp in ((2, 32), (130, 64), (2560, 64)):
        F = R.mixed_factor(rows_pad, kp)
        pad = min(37, rows_pad // 4)
        live = F[:rows_pad - pad]
        assert not F[rows_pad - pad:].any() and (live != 0).all() and np.isfinite(F).all()
        assert (live > 0).any() and (live < 0).any()
        if rows_pad > 100:
            top = np.abs(live).max(axis=0)
            assert top.max() / top.min() > 1e5                                  # columns many decades apart


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name,rows_pad,blocks", R.GRAM_CASES, ids=GRAM_IDS)
def test_mixed_slabs_lie_within_the_bound(name, rows_pad, blocks, kp):
    F, want, ref64, mag, _ = R.gram_reference("mixed", rows_pad, blocks, kp)
    nb = len(ref64)
    assert np.isfinite(want).all() and not bits(want[nb:]).any()
    assert (np.abs(want[:nb] - ref64) <= R.bound(R.slab_roundings(rows_pad, blocks), rows_pad, mag)).all()
    # the sum of the slabs against F^T F: the slab bounds add up (the fp64 sums are good to their length times 2^-53)
    F64 = F.astype(np.float64)
    total, tmag = F64.T @ F64, np.abs(F64).T @ np.abs(F64)
    assert (np.abs(want.astype(np.float64).sum(0) - total) <= R.bound(R.slab_roundings(rows_pad, blocks), rows_pad + blocks, tmag)).all()
    # a column at 1e-6 of the largest is held as tightly as the largest: the bound is per entry
    assert np.array_equal(bits(want), bits(want.transpose(0, 2, 1)))


@pytest.mark.parametrize("same", [True, False], ids=["A_is_B", "A_not_B"])
@pytest.mark.parametrize("rows_pad,blocks", [(2, 1), (134, 3), (512, 7), (2560, 1), (512, 1024)])
def test_mixed_cross_slabs_lie_within_the_bound(rows_pad, blocks, same):
    A, B, want, ref64, mag, _ = R.cross_reference("mixed", rows_pad, blocks, same)
    nb = len(ref64)
    assert np.isfinite(want).all() and not bits(want[nb:]).any()
    assert (np.abs(want[:nb] - ref64) <= R.bound(R.slab_roundings(rows_pad, blocks), rows_pad, mag)).all()
    assert same == np.array_equal(bits(want), bits(want.transpose(0, 2, 1)))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows_pad", R.FG_ROWS)
def test_mixed_fg_lies_within_the_bound(rows_pad, accumulate):
    F, G, O, want, ref64, mag = R.fg_reference("mixed", rows_pad, accumulate)
    assert np.isfinite(want).all()
    assert (np.abs(want - ref64) <= R.bound(64 + accumulate, 65, mag)).all()
    if accumulate:                                                             # the last rounding is there: fp32(out_old + acc)
        acc = R.fg_chain(F, G)
        assert np.array_equal(bits(want), bits((O + acc).astype(F32))) and (want != acc).any()
