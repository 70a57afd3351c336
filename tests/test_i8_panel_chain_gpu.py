"""The launches between the update epilogue and the int8 bits GEMM in the forms the iteration driver uses them (sweep() in csrc/api.hip),
each against a plain restatement, bit for bit:

  bmf_gram_partial_i8      the Gram launch with kp / 4 extra workgroups that derive (fused = 0) or CHECK (fused = 1) the column scales of
                           the digit planes (bmf_colscale_i8_block / bmf_colscale_i8_fused_block, csrc/common.h)
  bmf_make_panel_i8_cond   the conditional rebuild of the planes: nothing, the flagged columns byte by byte (at most 8), or everything
                           (make_panel_i8_kernel, csrc/xf_bits_i8.hip), with the Gram slab reduction riding in the same launch
  and the chain once: epilogue with a prediction that is off -> scale check -> rebuild -> GEMM (bmf_xf_bits_i8_cols).

Every output is pre-filled with a marker and has guard elements behind it; inputs must come back byte for byte."""
import numpy as np
import pytest

from test_palm_kernels_cpu import QMAX, digits_of
from test_xf_bits_i8_slabs_gpu import MARK, Problem, check_launch, dev, panel_positions, planes_to_int

pytestmark = pytest.mark.gpu

GUARD = 5
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    assert _lib.lib.bmf_xf_bits_i8_variant(0) >= 0
    return _lib


def marked(n, dtype):
    import torch
    return torch.full((n + GUARD,), MARK, dtype=dtype, device="cuda:0")


def with_guard(a, dtype):
    t = marked(a.size, dtype)
    t[:a.size] = dev(np.ascontiguousarray(a).ravel()).to(dtype)
    return t


def sync():
    import torch
    torch.cuda.synchronize()


def raw(t):
    return t.cpu().numpy().tobytes()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------------
# restatements (float32 where the device computes in float32)
# ------------------------------------------------------------------------------------------------------------------------------
def exact_exponent(m):
    """e_c of a column maximum m (float32): 23 bits, 22 when the maximum would land above what three balanced digits hold"""
    m = np.asarray(m, dtype=F32)
    with np.errstate(invalid="ignore"):
        live = (m > 0) & (m <= F32(3.0e38))
    fr, ex = np.frexp(np.where(live, m, F32(1.0)))
    return np.where(live, np.clip(np.where(fr > F32(0.99599), 22, 23) - ex, -100, 100), 0).astype(np.int64)


def pow2(e):
    return np.ldexp(F32(1.0), np.asarray(e).astype(np.int32)).astype(F32)


def scales_ref(blockmax, limbs):
    """bmf_colscale_i8_block: (2 kp) float32"""
    e = exact_exponent(blockmax.max(axis=0))
    return np.concatenate([pow2(e), pow2((8 if limbs == 2 else 0) - e)])


def fused_ref(blockmax, used, limbs):
    """bmf_colscale_i8_fused_block: the four kp-blocks of `scale` after the launch, float32, and the flags as booleans"""
    m = blockmax.max(axis=0).astype(F32)
    used = np.asarray(used, dtype=F32)
    fresh = pow2(exact_exponent(m))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = (m * used).astype(F32)
        ok = (used > 0) & (used <= F32(3.0e38)) & ((m == 0) | ((v <= F32(8355711.0)) & (v >= F32(2097152.0))))
        colscale = (F32(256.0 if limbs == 2 else 1.0) / np.where(ok, used, fresh)).astype(F32)
    return np.concatenate([fresh, colscale, fresh, np.where(ok, F32(0), F32(1))]).astype(F32), ~ok


def quantise_ref(F64, scale, limbs):
    """the planes of make_panel_i8_kernel as digits (limbs, rows, kp): q = rint(clip(F64 scale)) to even, two limbs: floor((q + 128) / 256)"""
    q = np.rint(np.clip(F64 * scale.astype(np.float64)[None, :], -QMAX, QMAX)).astype(np.int64)
    if limbs == 2:
        return digits_of((q + 128) >> 8)[:2], q
    return digits_of(q), q


def unpermute(planes, rows_pad):
    """host planes (limbs, kp, >= rows_pad) int8 -> digits (limbs, rows_pad, kp) in row order"""
    return planes[:, :, panel_positions_cached(rows_pad)].transpose(0, 2, 1).astype(np.int64)


_POS = {}


def panel_positions_cached(rows_pad):
    if rows_pad not in _POS:
        from pybmf_amd import _lib
        _POS[rows_pad] = panel_positions(_lib, rows_pad)
    return _POS[rows_pad]


def reduce_ref(slabs):
    """sum_b slabs[b] in fp64 the way reduce_slabs_kernel and the riding blocks add: 16 groups of ceil(count / 16) consecutive slabs, each
    summed in slab order from 0.0, then the 16 group sums in group order from 0.0"""
    count = slabs.shape[0]
    per = -(-count // 16)
    t = np.zeros(slabs.shape[1])
    for g in range(16):
        acc = np.zeros(slabs.shape[1])
        for b in range(g * per, min(g * per + per, count)):
            acc = acc + slabs[b].astype(np.float64)
        t = t + acc
    return t


# ------------------------------------------------------------------------------------------------------------------------------
# the scale check
# ------------------------------------------------------------------------------------------------------------------------------
def column_states(kp, nblk, seed):
    """blockmax (nblk, kp) and the scale the planes were built with, `used` (kp): one column per state of the check, the rest random"""
    rs = np.random.RandomState(seed)
    top = F32(8355711.0 / 1024.0)                       # times 2^10: exactly the largest number three balanced digits hold
    frac = F32(0.99599)
    states = [
        ("inside", F32(1.5), F32(2.0 ** 22), False),
        ("exactly 8355711", top, F32(2.0 ** 10), False),
        ("exactly 2^21", F32(0.125), F32(2.0 ** 24), False),
        ("one ulp above 8355711", np.nextafter(top, F32(np.inf)), F32(2.0 ** 10), True),
        ("one ulp below 2^21", np.nextafter(F32(0.125), F32(0)), F32(2.0 ** 24), True),
        ("all-zero column", F32(0), F32(2.0 ** 20), False),
        ("used = 0", F32(1), F32(0), True),
        ("used = inf", F32(1), F32(np.inf), True),
        ("used = nan", F32(1), F32(np.nan), True),
        ("all-zero column, used = 0", F32(0), F32(0), True),
        ("fraction just above 0.99599", np.nextafter(frac, F32(1)) * F32(32), F32(2.0 ** 17), False),
        ("fraction exactly float32(0.99599)", frac * F32(2.0 ** -7), F32(2.0 ** 29), False),
        ("used < 0", F32(1.5), F32(-(2.0 ** 22)), True),
        ("used not a power of two", F32(1), F32(3 * 2.0 ** 20), False),
        ("maximum above 3e38", F32(3.2e38), F32(2.0 ** -100), True),
        ("exponent clipped at 100", F32(2.0 ** -120), F32(2.0 ** 100), True),
    ]
    assert len(states) <= kp
    m = np.zeros(kp, F32)
    used = np.zeros(kp, F32)
    flagged = np.zeros(kp, bool)
    for c in range(kp):
        if c < len(states):
            _, m[c], used[c], flagged[c] = states[c]
        else:                                            # a live column whose prediction is off by -3 .. +2 bits
            m[c] = F32(rs.uniform(0.3, 3.0) * 10.0 ** rs.uniform(-6, 6))
            used[c] = pow2(exact_exponent(m[c]) + (c % 6) - 3)
    blockmax = (m[None, :] * rs.rand(nblk, kp).astype(F32)).astype(F32)
    blockmax[(np.arange(kp) * 5) % nblk, np.arange(kp)] = m
    assert np.array_equal(blockmax.max(axis=0), m)
    return blockmax, used, flagged, [s[0] for s in states]


@pytest.mark.parametrize("rows_pad", [512, 1536])
@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("kp", [32, 64])
def test_fused_scale_check(L, kp, limbs, rows_pad):
    import torch
    nblk, blocks = rows_pad // 128, 5
    blockmax, used, flagged, names = column_states(kp, nblk, 400 + kp + limbs)
    want, flags = fused_ref(blockmax, used, limbs)
    for c, name in enumerate(names):
        assert flags[c] == flagged[c], name                                  # the states are what they are named
    fresh = want[:kp]
    assert fresh[10] * blockmax.max(axis=0)[10] < 2.0 ** 22 <= fresh[11] * blockmax.max(axis=0)[11]   # the 22-bit and the 23-bit scale
    assert fresh[5] == 1.0 and flags[16:].any() and not flags[16:].all()
    rs = np.random.RandomState(7)
    F = dev((rs.standard_normal((rows_pad, kp)) * 10.0 ** rs.uniform(-3, 3, (rows_pad, kp))).astype(F32))
    bm = dev(blockmax)
    stop = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    scale = marked(4 * kp, torch.float32)
    scale[:kp] = dev(used)
    slabs, slabs_ref = marked(blocks * kp * kp, torch.float32), marked(blocks * kp * kp, torch.float32)
    before = raw(F), raw(bm)
    # the flag set: the scale workgroups write nothing
    stop.fill_(1)
    start = raw(scale)
    L.check(L.lib.bmf_gram_partial_i8(L.ptr(F), rows_pad, kp, kp, L.ptr(slabs), blocks, L.ptr(bm), limbs, L.ptr(scale), 1, L.ptr(stop), None))
    sync()
    assert raw(scale) == start
    stop.fill_(0)
    slabs.fill_(MARK)
    L.check(L.lib.bmf_gram_partial_i8(L.ptr(F), rows_pad, kp, kp, L.ptr(slabs), blocks, L.ptr(bm), limbs, L.ptr(scale), 1, L.ptr(stop), None))
    L.check(L.lib.bmf_gram_partial(L.ptr(F), rows_pad, kp, kp, L.ptr(slabs_ref), blocks, None))
    sync()
    got = scale.cpu().numpy()
    assert (got[4 * kp:] == MARK).all()
    for b, what in enumerate(("next prediction", "colscale", "exact scale", "flags")):
        g, w = got[b * kp:(b + 1) * kp], want[b * kp:(b + 1) * kp]
        assert same_bits(g, w), (what, [(names[c] if c < len(names) else c, g[c], w[c]) for c in np.flatnonzero(g.view(np.int32) != w.view(np.int32))])
    assert raw(slabs) == raw(slabs_ref) and (slabs.cpu().numpy()[-GUARD:] == MARK).all()      # the Gram slabs: those of bmf_gram_partial
    assert (raw(F), raw(bm)) == before


@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("kp", [32, 64])
def test_unfused_scales_are_the_builders(L, kp, limbs):
    import torch
    rows_pad = 1536
    rs = np.random.RandomState(11 + kp)
    F64 = rs.standard_normal((rows_pad, kp)) * 10.0 ** rs.uniform(-3, 0, (rows_pad, kp)) * (10.0 ** rs.uniform(-9, 3, kp))[None, :]
    F64[:, 4] = 0.0
    Fs = F64.astype(F32)
    F64d, Fd = dev(F64), dev(Fs)
    panel = torch.zeros((limbs, kp, rows_pad), dtype=torch.int8, device="cuda:0")
    ws = torch.zeros(rows_pad // 128 * kp, dtype=torch.float32, device="cuda:0")
    built = marked(2 * kp, torch.float32)
    L.check(L.lib.bmf_make_panel_i8(L.ptr(F64d), L.ptr(Fd), rows_pad, kp, kp, limbs, L.ptr(panel), rows_pad, L.ptr(ws), L.ptr(built), None))
    blockmax = np.abs(Fs).reshape(rows_pad // 128, 128, kp).max(axis=1)
    sync()
    assert np.array_equal(ws.cpu().numpy().reshape(-1, kp), blockmax)
    scale, slabs = marked(2 * kp, torch.float32), marked(3 * kp * kp, torch.float32)
    bm = dev(blockmax)
    L.check(L.lib.bmf_gram_partial_i8(L.ptr(Fd), rows_pad, kp, kp, L.ptr(slabs), 3, L.ptr(bm), limbs, L.ptr(scale), 0, None, None))
    sync()
    assert raw(scale) == raw(built) and same_bits(scale.cpu().numpy()[:2 * kp], scales_ref(blockmax, limbs))
    assert (scale.cpu().numpy()[2 * kp:] == MARK).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the conditional rebuild
# ------------------------------------------------------------------------------------------------------------------------------
def clamp_and_tie_factor(rows_pad, kp, ldf, seed):
    """F64 (rows_pad, ldf) and a shadow whose only job is the column maximum: entries t / scale with t from a pool of values at and
    beyond the clamp, exact .5 ties, the ties of the two-limb rounding (128 mod 256), zeros, and random values in between; junk in the
    columns kp .. ldf - 1"""
    rs = np.random.RandomState(seed)
    maxima = (2.0 ** ((np.arange(kp) % 9) - 4) * np.where(np.arange(kp) % 2, 1.0, 1.9921875)).astype(F32)   # 1.9921875 = 0.99609375 * 2: the 22-bit branch
    shadow = np.zeros((rows_pad, kp), F32)
    shadow[(np.arange(kp) * 37) % rows_pad, np.arange(kp)] = maxima
    scale = pow2(exact_exponent(maxima))
    pool = np.array([8355711.0, 8355711.5, 8355712.0, 9.0e6, 2.0 ** 24, 8355710.5, 8355709.5, 0.5, 1.5, 2.5, 127.5, 128.5, 32767.5, 32768.5, 0.0,
                     128.0, 384.0, 127.0, 129.0, 32896.0, 8355584.0, 8355583.5, 4194304.0, 0.49999999, 0.50000001])
    t = np.where(rs.rand(rows_pad, kp) < 0.5, rs.choice(pool, (rows_pad, kp)) * rs.choice([-1.0, 1.0], (rows_pad, kp)),
                 np.where(rs.rand(rows_pad, kp) < 0.5, rs.uniform(-8.4e6, 8.4e6, (rows_pad, kp)), np.rint(rs.uniform(-70000, 70000, (rows_pad, kp)))))
    F64 = rs.uniform(1.0, 2.0, (rows_pad, ldf)) * 1e3
    F64[:, :kp] = t / scale.astype(np.float64)[None, :]
    return F64, shadow, scale


def build(L, F64, shadow, rows_pad, ldf, kp, limbs):
    """the stand-alone builder: host planes (limbs, kp, rows_pad) and its 2 kp scales"""
    import torch
    panel = torch.full((limbs, kp, rows_pad), MARK, dtype=torch.int8, device="cuda:0")
    ws = torch.zeros(rows_pad // 128 * kp, dtype=torch.float32, device="cuda:0")
    scale = torch.zeros(2 * kp, dtype=torch.float32, device="cuda:0")
    sh = np.zeros((rows_pad, ldf), F32)
    sh[:, :kp] = shadow
    F64d, shd = dev(F64), dev(sh)                                             # (held until the launches have run)
    L.check(L.lib.bmf_make_panel_i8(L.ptr(F64d), L.ptr(shd), rows_pad, ldf, kp, limbs, L.ptr(panel), rows_pad, L.ptr(ws), L.ptr(scale), None))
    sync()
    return panel.cpu().numpy(), scale.cpu().numpy()


@pytest.mark.parametrize("rows_pad", [512, 2048])
@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("kp", [32, 64])
def test_conditional_rebuild(L, kp, limbs, rows_pad):
    import torch
    ldf, ldp = kp + 2, rows_pad + 16
    F64, shadow, scale = clamp_and_tie_factor(rows_pad, kp, ldf, 900 + kp + limbs)
    new, new_scale = build(L, F64, shadow, rows_pad, ldf, kp, limbs)
    assert same_bits(new_scale, scales_ref(shadow.reshape(rows_pad // 128, 128, kp).max(axis=1), limbs)) and same_bits(new_scale[:kp], scale)
    digits, q = quantise_ref(F64[:, :kp], scale, limbs)
    bad = np.argwhere((unpermute(new, rows_pad) != digits).any(axis=0))
    assert (np.abs(q) == QMAX).mean() > 0.05 and not len(bad), (len(bad), [(r, c, F64[r, c] * float(scale[c])) for r, c in bad[:5]])   # the builder itself, clamp and ties
    rs = np.random.RandomState(3)
    Fo = np.zeros((rows_pad, ldf))
    Fo[:, :kp] = rs.standard_normal((rows_pad, kp)) * 10.0 ** rs.uniform(-2, 2, kp)[None, :]
    old, _ = build(L, Fo, Fo[:, :kp].astype(F32), rows_pad, ldf, kp, limbs)
    assert (old != new).mean() > 0.25
    F64d, scaled = dev(F64), dev(scale)
    colscale_want = (F32(256.0 if limbs == 2 else 1.0) / scale).astype(F32)
    for cols in ([], [0], [kp - 1], [0, kp - 1], [0, 3, 4, 17, 18, 21, kp - 1], [0, 3, 4, 17, 18, 21, 30, kp - 1],
                 [0, 3, 4, 17, 18, 21, 29, 30, kp - 1], list(range(kp))):
        fl = np.zeros(kp, F32)
        fl[cols] = [1.0, -2.5, 1e-30][len(cols) % 3]                          # any non-zero word flags a column
        flags = dev(fl)
        start = np.full((limbs, kp, ldp), MARK, np.int8)
        start[:, :, :rows_pad] = old
        panel = with_guard(start, torch.int8)
        colscale = marked(kp, torch.float32)
        before = raw(F64d), raw(scaled), raw(flags)
        L.check(L.lib.bmf_make_panel_i8_cond(L.ptr(F64d), rows_pad, ldf, kp, limbs, L.ptr(panel), ldp, L.ptr(scaled), L.ptr(flags), L.ptr(colscale),
                                             None, 0, 0, None, None, None, None))
        sync()
        want = start.copy()
        if len(cols) > 8:
            want[:, :, :rows_pad] = new
        else:
            want[:, cols, :rows_pad] = new[:, cols]
        got = panel.cpu().numpy()
        assert (got[-GUARD:] == MARK).all()
        got = got[:-GUARD].reshape(limbs, kp, ldp)
        bad = np.argwhere(got != want)
        assert not len(bad), (cols, len(bad), bad[:4].tolist())
        cs = colscale.cpu().numpy()
        assert same_bits(cs[:kp], colscale_want) if len(cols) > 8 else (cs[:kp] == MARK).all(), cols
        assert (cs[kp:] == MARK).all() and (raw(F64d), raw(scaled), raw(flags)) == before


@pytest.mark.parametrize("kp", [32, 64])
def test_slab_reduction_rides_in_the_rebuild_launch(L, kp):
    import torch
    rows_pad, limbs, rn = 512, 3, kp * kp
    F64, shadow, scale = clamp_and_tie_factor(rows_pad, kp, kp, 77)
    new, _ = build(L, F64, shadow, rows_pad, kp, kp, limbs)
    old, _ = build(L, F64[::-1].copy(), shadow[::-1].copy(), rows_pad, kp, kp, limbs)
    F64d, scaled = dev(F64), dev(scale)
    stop = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    rs = np.random.RandomState(kp)
    for rcount in (1, 3, 15, 16, 17, 67):
        slabs_h = (rs.standard_normal((rcount, rn)) * 10.0 ** rs.uniform(-6, 6, (rcount, rn))).astype(F32)
        slabs = dev(slabs_h)
        want64 = reduce_ref(slabs_h)
        ref32, ref64 = marked(rn, torch.float32), marked(rn, torch.float64)
        L.check(L.lib.bmf_reduce_slabs(L.ptr(slabs), rn, rcount, rn, L.ptr(ref32), L.ptr(ref64), None))
        sync()
        assert raw(ref64[:rn]) == want64.tobytes() and raw(ref32[:rn]) == want64.astype(F32).tobytes()
        for cols, give32, give64, stopped in (([], True, True, 0), ([], True, False, 0), ([], False, True, 0), ([0, kp - 1], True, True, 0),
                                              (list(range(kp)), True, True, 0), ([0, kp - 1], True, True, 1)):
            fl = np.zeros(kp, F32)
            fl[cols] = 1.0
            flags = dev(fl)
            panel = with_guard(old, torch.int8)
            colscale = marked(kp, torch.float32)
            out32, out64 = marked(rn, torch.float32), marked(rn, torch.float64)
            stop.fill_(stopped)
            before = raw(slabs)
            L.check(L.lib.bmf_make_panel_i8_cond(L.ptr(F64d), rows_pad, kp, kp, limbs, L.ptr(panel), rows_pad, L.ptr(scaled), L.ptr(flags), L.ptr(colscale),
                                                 L.ptr(slabs), rcount, rn, L.ptr(out32) if give32 else None, L.ptr(out64) if give64 else None, L.ptr(stop), None))
            sync()
            what = (rcount, cols, give32, give64, stopped)
            want = old.copy()
            if not stopped:
                want[:, cols] = new[:, cols]
            assert raw(panel[:old.size]) == want.tobytes() and (panel.cpu().numpy()[-GUARD:] == MARK).all(), what
            if stopped:       # the documented behaviour: the fp64 sum is zeroed, nothing else is written
                assert raw(out64[:rn]) == np.zeros(rn).tobytes() and (out32 == MARK).all() and (out64[rn:] == MARK).all(), what
                continue
            assert raw(out32) == (raw(ref32) if give32 else raw(marked(rn, torch.float32))), what
            assert raw(out64) == (raw(ref64) if give64 else raw(marked(rn, torch.float64))), what
            assert raw(slabs) == before


def test_refused_calls(L):
    import torch
    kp, rows_pad = 32, 512
    f = torch.zeros(rows_pad * kp, dtype=torch.float32, device="cuda:0")
    d = torch.zeros(rows_pad * kp, dtype=torch.float64, device="cuda:0")
    p = marked(3 * kp * rows_pad, torch.int8)
    sc = marked(4 * kp, torch.float32)
    start = raw(p), raw(sc)
    g, c = L.lib.bmf_gram_partial_i8, L.lib.bmf_make_panel_i8_cond
    assert g(L.ptr(f), rows_pad, kp, kp, L.ptr(f), 4, None, 3, L.ptr(sc), 1, None, None) == -1 and b"bmf_gram_partial_i8: null pointer" in L.lib.bmf_last_error()
    assert g(L.ptr(f), rows_pad, kp, kp, L.ptr(f), 4, L.ptr(f), 3, None, 1, None, None) == -1
    assert g(L.ptr(f), rows_pad, kp, kp, L.ptr(f), 4, L.ptr(f), 4, L.ptr(sc), 1, None, None) == -1
    assert g(L.ptr(f), rows_pad, kp, kp, L.ptr(f), 4, L.ptr(f), 3, L.ptr(sc), 2, None, None) == -1
    assert g(L.ptr(f), rows_pad, kp, kp, L.ptr(f), 0, L.ptr(f), 3, L.ptr(sc), 1, None, None) == -1
    assert g(L.ptr(f), 576, kp, kp, L.ptr(f), 4, L.ptr(f), 3, L.ptr(sc), 1, None, None) == -1          # rows_pad % 128
    ok = (L.ptr(d), rows_pad, kp, kp, 3, L.ptr(p), rows_pad, L.ptr(sc), L.ptr(sc), L.ptr(sc))
    assert c(*ok[:8], None, L.ptr(sc), None, 0, 0, None, None, None, None) == -1 and b"bmf_make_panel_i8_cond: null pointer" in L.lib.bmf_last_error()
    assert c(*ok[:9], None, None, 0, 0, None, None, None, None) == -1
    assert c(L.ptr(d), 768, kp, kp, 3, L.ptr(p), 768, L.ptr(sc), L.ptr(sc), L.ptr(sc), None, 0, 0, None, None, None, None) == -1
    assert c(L.ptr(d), rows_pad, kp, kp, 4, L.ptr(p), rows_pad, L.ptr(sc), L.ptr(sc), L.ptr(sc), None, 0, 0, None, None, None, None) == -1
    assert c(L.ptr(d), rows_pad, kp, kp, 3, L.ptr(p), rows_pad - 16, L.ptr(sc), L.ptr(sc), L.ptr(sc), None, 0, 0, None, None, None, None) == -1
    assert c(*ok, L.ptr(f), 0, kp * kp, L.ptr(f), None, None, None) == -1                               # rcount
    assert c(*ok, L.ptr(f), 3, kp * kp + 8, L.ptr(f), None, None, None) == -1                           # rn % 16
    assert c(*ok, L.ptr(f), 3, kp * kp, None, None, None, None) == -1                                   # no output
    sync()
    assert (raw(p), raw(sc)) == start


# ------------------------------------------------------------------------------------------------------------------------------
# the chain, once
# ------------------------------------------------------------------------------------------------------------------------------
def test_epilogue_scale_check_rebuild_gemm(L):
    """bmf_mu_epilogue builds the planes with a predicted scale that is off for three columns (3: three bits too large, 7: one bit low,
    11: two bits low); the scale check keeps 7 and flags 3 and 11; the rebuild rewrites those two; the GEMM runs on the result."""
    import torch
    from test_mu_epilogue_cpu import PENALTY, general_inputs, mu_step_ref
    from test_mu_epilogue_gpu import launch
    rows, red, kp, k, limbs = 1280, 3584, 32, 20, 3
    a = general_inputs(dict(form="planes3", mode=PENALTY, k=k, kp=kp, rows_pad=red, rows=3500, layout="plain", splits=1, reg=1.5, seed=91))
    e = exact_exponent(mu_step_ref(a)["blockmax"].max(axis=0)).astype(np.float64)      # the exact scales of the step's result ...
    e[3] += 3
    e[7] -= 1
    e[11] -= 2                                                                         # ... but for three columns
    a["plane_scale"] = (2.0 ** e).astype(F32)
    got = launch(a)
    F64, blockmax, predicted = got["F64"], got["blockmax"], a["plane_scale"]
    assert not F64[3500:].any() and not F64[:, k:].any()
    want4, flagged = fused_ref(blockmax, predicted, limbs)
    assert np.flatnonzero(flagged).tolist() == [3, 11]
    Fd, F64d, bm = dev(got["F"]), dev(F64), dev(blockmax)
    scale = marked(4 * kp, torch.float32)
    scale[:kp] = dev(predicted)
    slabs = marked(4 * kp * kp, torch.float32)
    planes = with_guard(got["planes"], torch.int8)
    colscale_out = marked(kp, torch.float32)
    gram32, gram64 = marked(kp * kp, torch.float32), marked(kp * kp, torch.float64)
    L.check(L.lib.bmf_gram_partial_i8(L.ptr(Fd), red, kp, kp, L.ptr(slabs), 4, L.ptr(bm), limbs, L.ptr(scale), 1, None, None))
    L.check(L.lib.bmf_make_panel_i8_cond(L.ptr(F64d), red, kp, kp, limbs, L.ptr(planes), red, scale.data_ptr() + 4 * 2 * kp, scale.data_ptr() + 4 * 3 * kp,
                                         L.ptr(colscale_out), L.ptr(slabs), 4, kp * kp, L.ptr(gram32), L.ptr(gram64), None, None))
    sync()
    sc = scale.cpu().numpy()
    assert same_bits(sc[:4 * kp], want4) and (colscale_out == MARK).all()
    in_force = np.where(flagged, want4[2 * kp:3 * kp], predicted)            # the exact scale where flagged, the prediction where kept
    assert same_bits(sc[kp:2 * kp], (F32(1) / in_force).astype(F32))
    host = planes.cpu().numpy()[:-GUARD].reshape(limbs, kp, red)
    digits, q = quantise_ref(F64, in_force, limbs)
    assert np.array_equal(unpermute(host, red), digits)
    assert np.abs(q[:, 3]).max() <= QMAX and np.abs(q[:, 3]).max() >= 2 ** 22 and 2 ** 21 <= np.abs(q[:, 7]).max() < 2 ** 22 <= np.abs(q[:, 11]).max()
    changed = (host != got["planes"]).any(axis=(0, 2))
    assert np.flatnonzero(changed).tolist() == [3, 11]
    G = F64.astype(F32).astype(np.float64)
    np.testing.assert_allclose(gram64.cpu().numpy()[:kp * kp].reshape(kp, kp), G.T @ G, rtol=1e-5, atol=0)
    # the GEMM on those planes: every slab against the integers they should hold
    P = Problem(L, rows, red, kp, limbs, planes=(host, sc[kp:2 * kp].copy()))
    assert np.array_equal(P.Q, q.T) and np.array_equal(planes_to_int(L, host, red), q.T)
    plan = P.plan(kp)
    check_launch(P, P.launch(P.new_out(plan.slots + 1), 0, kp, tiled=False), plan, 0, kp)
