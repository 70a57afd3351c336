"""bmf_mu_epilogue (csrc/epilogue.hip: mu_epilogue_kernel<T, NT> and mu_epilogue_i8_kernel<NT, MODE, LIMBS>) called directly, element by
element, against the stand-in of tests/test_mu_epilogue_cpu.py: general steps held inside the enclosure of the fp32 product, exact
inputs within the rounding of the element-wise part, the clamps, the threshold, and everything else one launch writes checked against
the device's own F64 (byte for byte, or with the derived tolerances for the two fp64 sums).

Every output buffer is pre-filled with a marker and has guard slots behind it that must keep the marker; the inputs of a launch must
come back byte for byte.  The fp32 shadow F is an INPUT of the update without `den` (it is the operand of the F G product there): that
form gets float32(F64) with zero padding, every other one the marker.
"""
import ctypes as C
import fractions

import numpy as np
import pytest

from test_mu_epilogue_cpu import (EPS, FORMS, PENALTY, PREPARE, QMAX, WNMF, bf16_addends, block_num, case_id, colbits_to_bool, derived_outputs,
                                  general_cases, general_inputs, mu_step_ref, planes_to_digits, rowbits_to_bool)

pytestmark = pytest.mark.gpu

MARK = -7
GUARD = 5


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def marked(n, dtype):
    import torch
    return torch.full((n,), MARK, dtype=dtype, device="cuda:0")


def with_guard(a, dtype):
    """a flat device buffer holding `a` with GUARD marked slots behind it"""
    t = marked(a.size + GUARD, dtype)
    t[:a.size] = dev(np.ascontiguousarray(a).ravel()).to(dtype)
    return t


def launch(a, stop=None, ldcb=None, ldp=None, expect=0, raw=None, null=(), shift=None):
    """One bmf_mu_epilogue call on the host arrays of `a` (the dict mu_step_ref takes, with the launch form in terms, limbs, blockmax).
    Returns the outputs as host arrays in their logical shapes; the guards, the unused parts of colbits, panel and planes, the outputs
    not asked for and the inputs are checked here.  raw: struct fields overwritten after the valid ones are filled in; null: pointer
    fields passed as NULL; shift: bytes added to a pointer field.  expect = -1: the call must refuse and leave every buffer as it was."""
    import torch
    from pybmf_amd import _lib as L
    rows_pad, kp = a["rows_pad"], a["kp"]
    terms, limbs = a.get("terms", 0), a.get("limbs", 0)
    want_bm = bool(a.get("blockmax")) or limbs > 0
    n, nb = rows_pad * kp, rows_pad // 128
    ldcb = rows_pad // 32 + 3 if ldcb is None else ldcb
    ldp = rows_pad + 32 if ldp is None else ldp
    reads_shadow = a["mode"] != PREPARE and a.get("den") is None
    bufs = {"F64": with_guard(a["F64"], torch.float64), "F": with_guard(a["F"], torch.float32) if reads_shadow else marked(n + GUARD, torch.float32),
            "rowbits": marked(rows_pad + GUARD, torch.int64), "colbits": marked(kp * max(ldcb, 1) + GUARD, torch.int32),
            "partials": marked(2 * nb + GUARD, torch.float64), "blockmax": marked(nb * kp + GUARD, torch.float32),
            "panel": marked(3 * kp * ldp + GUARD, torch.int16), "planes": marked(3 * kp * ldp + GUARD, torch.int8)}
    ins = {}
    for name, dt in (("num", np.float32), ("G", np.float32), ("den", np.float32), ("plane_scale", np.float32)):
        if a.get(name) is not None:
            ins[name] = dev(np.asarray(a[name], dtype=dt))
    if stop is not None:
        ins["stop"] = dev(np.array([stop], dtype=np.int32))
    before = {k_: v.cpu().numpy().tobytes() for k_, v in {**bufs, **ins}.items()}
    p = L.EpilogueArgs()
    p.F64, p.F, p.rows_pad, p.rows, p.k, p.kp = bufs["F64"].data_ptr(), bufs["F"].data_ptr(), rows_pad, a["rows"], a["k"], kp
    p.num, p.slab_stride, p.splits = (ins["num"].data_ptr() if "num" in ins else None), a["slab_stride"], a["splits"]
    p.num_block_stride = a.get("num_block_stride", 0)
    p.G = ins["G"].data_ptr() if "G" in ins else None
    p.den = ins["den"].data_ptr() if "den" in ins else None
    p.reg, p.mode, p.thr, p.terms = a["reg"], a["mode"], a["thr"], terms
    p.panel, p.ldp = bufs["panel"].data_ptr(), ldp
    p.rowbits, p.colbits, p.ldcb, p.partials = bufs["rowbits"].data_ptr(), bufs["colbits"].data_ptr(), ldcb, bufs["partials"].data_ptr()
    p.stop = ins["stop"].data_ptr() if stop is not None else None
    p.blockmax = bufs["blockmax"].data_ptr() if want_bm else None
    if limbs:
        p.planes, p.plane_scale, p.limbs = bufs["planes"].data_ptr(), ins["plane_scale"].data_ptr(), limbs
    for name, v in (raw or {}).items():
        setattr(p, name, v)
    for name, nbytes in (shift or {}).items():
        setattr(p, name, getattr(p, name) + nbytes)
    for name in null:
        setattr(p, name, None)
    rc = L.lib.bmf_mu_epilogue(C.byref(p), None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lib.bmf_last_error())
    host = {k_: v.cpu().numpy() for k_, v in bufs.items()}
    for k_, v in ins.items():
        assert v.cpu().numpy().tobytes() == before[k_], f"input {k_} was written"
    if expect != 0 or (stop is not None and stop != 0):
        for k_, v in host.items():
            assert v.tobytes() == before[k_], f"{k_} was written by a launch that must write nothing"
        return None
    for k_, v in host.items():
        assert (v[-GUARD:] == MARK).all(), f"guard behind {k_}"
    if a["mode"] == PREPARE:
        assert host["F64"].tobytes() == before["F64"], "F64 was written in PREPARE mode"
    cb = host["colbits"][:-GUARD].reshape(kp, ldcb)
    assert (cb[:, rows_pad // 32:] == MARK).all(), "colbits beyond rows_pad / 32"
    out = {"F64": host["F64"][:n].reshape(rows_pad, kp), "F": host["F"][:n].reshape(rows_pad, kp), "rowbits": host["rowbits"][:rows_pad],
           "colbits": cb[:, :rows_pad // 32], "partials": host["partials"][:2 * nb].reshape(nb, 2)}
    if want_bm:
        out["blockmax"] = host["blockmax"][:nb * kp].reshape(nb, kp)
    else:
        assert (host["blockmax"] == MARK).all(), "blockmax was written without being asked for"
    for name, count in (("panel", terms), ("planes", limbs)):
        pl = host[name][:-GUARD].reshape(3, kp, ldp)
        assert (pl[count:] == MARK).all() and (pl[:, :, rows_pad:] == MARK).all(), f"{name}: written beyond what was asked for"
        if count:
            out[name] = pl[:count, :, :rows_pad]
    return out


def panel_positions(rows_pad):
    """position of row r inside a panel column: 128-row blocks, inside each the order bmf_panel_pos"""
    from pybmf_amd import _lib as L
    pos = np.array([L.lib.bmf_panel_pos(int(c)) for c in range(128)])
    assert sorted(pos.tolist()) == list(range(128))
    r = np.arange(rows_pad)
    return (r // 128) * 128 + pos[r % 128]


def check_everything_else(a, got, num32):
    """What the launch writes besides F64, against the device's own F64.  The inputs carry junk in the padding of F64 and num: a sum
    taken before the padding is zeroed, or a new factor that keeps it, misses the tolerances (and the zeros) here."""
    rows_pad, kp = a["rows_pad"], a["kp"]
    want = derived_outputs(a, got["F64"], num32)
    ok = want["ok"]
    assert got["F"].tobytes() == want["F"].tobytes()                                   # the shadow, bit for bit, zero in the padding
    assert not got["F"][~ok].any() and (a["mode"] == PREPARE or not got["F64"][~ok].any())
    rb, cb = rowbits_to_bool(got["rowbits"], kp), colbits_to_bool(got["colbits"], rows_pad)
    assert np.array_equal(rb, want["bits"]) and np.array_equal(cb, want["bits"]) and not rb[~ok].any() and not cb[~ok].any()
    err0 = np.abs(got["partials"][:, 0] - want["partials"][:, 0])
    assert (err0 <= want["ptol0"]).all(), (err0, want["ptol0"])
    np.testing.assert_allclose(got["partials"][:, 1], want["partials"][:, 1], rtol=1e-12, atol=0)
    if "blockmax" in got:
        assert got["blockmax"].tobytes() == want["blockmax"].tobytes()
    if "planes" in got:
        limbs = got["planes"].shape[0]
        d = planes_to_digits(got["planes"], rows_pad)
        assert np.array_equal(d, want["digits"] if limbs == 3 else want["digits2"]) and not d[:, ~ok].any()
    if "panel" in got:
        terms = got["panel"].shape[0]
        p = got["panel"].view(np.uint16)[:, :, panel_positions(rows_pad)].transpose(0, 2, 1)
        # byte for byte, with one freedom: the first addend may be rounded from the fp64 entry or from its shadow (bf16_addends)
        want1, want2 = bf16_addends(got["F"], terms, want["fn"]), bf16_addends(got["F"], terms)
        print(f"panel: {(want1 != want2).any(axis=0).sum()} entries on a tie, {(p != want2).any(axis=0).sum()} of them rounded from fp64")
        bad = np.argwhere((p != want1).any(axis=0) & (p != want2).any(axis=0))[:4]
        assert not len(bad), [(got["F"][r, c_].view(np.uint32), p[:, r, c_].tolist(), want2[:, r, c_].tolist()) for r, c_ in bad]
        if terms == 3:
            val = (p.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(axis=0)
            assert np.array_equal(val, got["F"].astype(np.float64))
    return want


def check_enclosure(ref, got, what=""):
    """every entry: lo - tol <= F64 <= hi + tol; prints how much of the tolerance was used"""
    below, above = ref["lo"] - got["F64"], got["F64"] - ref["hi"]
    with np.errstate(invalid="ignore", divide="ignore"):
        used = np.nanmax(np.where(ref["tol"] > 0, np.maximum(below, above) / ref["tol"], np.where(np.maximum(below, above) > 0, np.inf, 0.0)))
    print(f"{what}: worst (distance outside [lo, hi]) / tol = {max(used, 0.0):.3g}")
    bad = (below > ref["tol"]) | (above > ref["tol"])
    assert not bad.any(), (np.argwhere(bad)[:5], below.max(), above.max())


def region_masks(rows_pad, rows, k, kp):
    r, c = np.arange(rows_pad)[:, None], np.arange(kp)[None, :]
    ok = (r < rows) & (c < k)
    return ok, (ok & (r < 128), (ok & (r == rows - 1)) | (ok & (c == k - 1)), ~ok)


# ---- general steps: the interval check, and everything else the launch writes --------------------------------------------------------------
@pytest.mark.parametrize("c", general_cases(), ids=case_id)
def test_general_steps_stay_inside_the_enclosure(c):
    a = general_inputs(c)
    ref = mu_step_ref(a)
    got = launch(a)
    check_enclosure(ref, got, case_id(c))
    check_everything_else(a, got, ref["num32"])
    # a second launch on equal inputs gives the same bytes everywhere, and the optional outputs do not change the step
    again = launch(a)
    assert set(again) == set(got)
    for name in got:
        assert again[name].tobytes() == got[name].tobytes(), name
    other = dict(a, terms=0, limbs=0, blockmax=False, plane_scale=None) if c["form"] != "plain" else dict(a, terms=2, blockmax=True)
    assert launch(other)["F64"].tobytes() == got["F64"].tobytes()


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------
NEAR_ONE = (20, 30, 40, 52)


def exact_inputs(mode, reg, form, k, kp):
    """G diagonal with power-of-two entries, F and num dyadic: every F G entry is one exact product.  Blocks 0..3 hold 1 - 2^-n in every
    valid entry, n = 20, 30, 40, 52, with num = float32(F) g: the ratio is exactly 1 when reg = 0."""
    rs = np.random.RandomState(k + mode)
    rows_pad, rows = 1024, 1000
    ok, _ = region_masks(rows_pad, rows, k, kp)
    terms, limbs, blockmax, _ = FORMS[form]
    F64 = rs.randint(1, 1537, (rows_pad, kp)) / 1024.0
    for b, nn in enumerate(NEAR_ONE):
        F64[128 * b:128 * (b + 1)] = 1.0 - 2.0 ** -nn
    F = np.where(ok, F64, 0.0).astype(np.float32)
    g = np.zeros(kp)
    g[:k] = 2.0 ** rs.randint(-2, 4, k)
    num = rs.randint(0, 513, (rows_pad, kp)) / 64.0
    num[:512] = F[:512].astype(np.float64) * g[None, :]
    num[~ok] = 7.0
    return dict(F64=F64, F=F, rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1, slab_stride=rows_pad * kp, num_block_stride=0,
                num=num.astype(np.float32).reshape(1, -1), G=np.diag(g).astype(np.float32), den=None, reg=reg, mode=mode, thr=0.5,
                plane_scale=np.full(kp, 2.0 ** 22, np.float32) if limbs else None, terms=terms, limbs=limbs, blockmax=blockmax)


@pytest.mark.parametrize("k,kp", [(20, 32), (37, 64)])
@pytest.mark.parametrize("form", ["bf16-3", "planes3"])
@pytest.mark.parametrize("mode,reg", [(PENALTY, 0.0), (PENALTY, 1.5), (PENALTY, 1e10), (WNMF, 0.0)])
def test_exact_inputs_and_entries_next_to_one(mode, reg, form, k, kp):
    a = exact_inputs(mode, reg, form, k, kp)
    ref = mu_step_ref(a)
    got = launch(a)
    err = np.abs(got["F64"] - ref["F64"])
    print(f"worst |F64 - stand-in| / tol = {np.nanmax(err[ref['tol'] > 0] / ref['tol'][ref['tol'] > 0]):.3g}")
    assert (err <= ref["tol"]).all(), (np.argwhere(err > ref["tol"])[:5], err.max())          # no enclosure: the product is exact
    want = check_everything_else(a, got, ref["num32"])
    ok = want["ok"]
    if reg == 0.0:          # the ratio is exactly 1: entries that no fp32 holds come through the update unchanged
        assert np.array_equal(got["F64"][:512][ok[:512]], a["F64"][:512][ok[:512]])
        assert (got["F"][128:512][ok[128:512]] == 1.0).all() and not want["bits"][:512][~ok[:512]].any() and want["bits"][:512][ok[:512]].all()
    # the regulariser sum of the blocks next to 1, against exact arithmetic on the device's own entries: what fp64 is there for
    for b, nn in enumerate(NEAR_ONE):
        fn = got["F64"][128 * b:128 * (b + 1)][ok[128 * b:128 * (b + 1)]]
        exact = sum(((x * x - x) ** 2 for x in map(fractions.Fraction, fn.tolist())), fractions.Fraction(0))
        assert abs(got["partials"][b, 0] - float(exact)) <= want["ptol0"][b], (nn, got["partials"][b, 0], float(exact))
        if reg == 0.0:      # (an fp32 evaluation sees 1 in the blocks of n >= 30 and gives 0)
            assert got["partials"][b, 0] > 0
            assert float(exact) == pytest.approx(fn.size * 2.0 ** (-2 * nn), rel=2.0 ** -(nn - 2))


# ---- the clamps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kp", [(20, 32), (37, 64)])
@pytest.mark.parametrize("form", ["plain", "den", "planes3"])
@pytest.mark.parametrize("mode", [PENALTY, WNMF])
def test_clamps(mode, form, k, kp):
    """den == 0 with f = 0 (a zero row, reg = 0) and with f != 0 (G = 0); fn == 0 from a zero numerator and from underflow (f = 5e-324,
    ratio 0.25): eps in PENALTY mode, 0 in WNMF -- each in a full tile, in the last valid row and column, and in the padding."""
    rs = np.random.RandomState(k)
    rows_pad, rows = 512, 400
    n = rows_pad * kp
    ok, regions = region_masks(rows_pad, rows, k, kp)
    terms, limbs, blockmax, with_den = FORMS[form]
    kind = (np.arange(n) % 5).reshape(rows_pad, kp)                  # 2: zero numerator, 3: f = 5e-324, else an ordinary entry
    zrows = np.zeros((rows_pad, kp), bool)
    zrows[[5, rows - 2, rows_pad - 2]] = True
    for hit in (kind == 2, kind == 3):
        assert all((hit & ~zrows & reg_).any() for reg_ in regions)
    assert (zrows & regions[0]).any() and (zrows & regions[1]).any() and (zrows & regions[2]).any()
    F64 = rs.rand(rows_pad, kp) + 0.1
    F64[kind == 3] = 5e-324
    F64[zrows] = 0.0
    F = np.where(ok, F64, 0.0).astype(np.float32)
    H = rs.rand(40, k) * 0.5
    G = np.zeros((kp, kp), np.float32)
    G[:k, :k] = (H.T @ H).astype(np.float32)
    fg = (F.astype(np.float64) @ G.astype(np.float64)).astype(np.float32)
    for zero_den in (False, True):
        if zero_den:
            fg = np.zeros_like(fg)
        num = (rs.rand(rows_pad, kp) * 3 + 0.1).astype(np.float32)
        num[kind == 2] = 0.0
        num[kind == 3] = (0.25 * fg)[kind == 3]
        a = dict(F64=F64, F=F, rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1, slab_stride=n, num_block_stride=0, num=num.reshape(1, -1),
                 G=None if with_den else (np.zeros_like(G) if zero_den else G), den=fg if with_den else None, reg=0.0, mode=mode, thr=0.5,
                 plane_scale=np.full(kp, 2.0 ** 20, np.float32) if limbs else None, terms=terms, limbs=limbs, blockmax=blockmax)
        ref = mu_step_ref(a)
        got = launch(a)
        check_enclosure(ref, got, f"clamps zero_den={zero_den}")
        check_everything_else(a, got, ref["num32"])
        floor_ = EPS if mode == PENALTY else 0.0
        for hit in (zrows, kind == 2, kind == 3):
            assert (got["F64"][hit & ok] == floor_).all()
        plain = ok & ~zrows & (kind != 2) & (kind != 3)
        if zero_den:     # den == 0 -> eps under an ordinary entry: f (num / eps), two correctly rounded operations
            assert np.array_equal(got["F64"][plain], F64[plain] * (num[plain].astype(np.float64) / EPS)) and (got["F64"][plain] > 1e12).all()
        else:
            assert (got["F64"][plain] > 1e-6).all() and (got["F64"][plain] < 1e3).all()


# ---- the threshold ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kp", [(20, 32), (37, 64)])
@pytest.mark.parametrize("form", ["prepare", "prepare-planes", "den-penalty", "den-wnmf", "ring-planes"])
def test_threshold_is_strict_and_taken_on_fp64(form, k, kp):
    """fn = f exactly (PREPARE, or an update with nume == den): the test places entries at float64(float32(thr)) and one fp64 step either
    side.  The step above rounds onto thr in the shadow and still sets the bit."""
    rows_pad, rows = 512, 400
    n = rows_pad * kp
    thr = np.float32(0.3)
    t = np.float64(thr)
    up, down = np.nextafter(t, np.inf), np.nextafter(t, -np.inf)
    assert np.float32(up) == thr and np.float32(down) == thr
    values = np.array([t, up, down, 0.1, 0.9, 0.25, 1.5])            # an odd count: cycled, each reaches every column
    F64 = values[np.arange(n) % len(values)].reshape(rows_pad, kp)
    ok, regions = region_masks(rows_pad, rows, k, kp)
    for v in values[:3]:
        assert all(((F64 == v) & reg_).any() for reg_ in regions)
    F = np.where(ok, F64, 0.0).astype(np.float32)
    rs = np.random.RandomState(k)
    a = dict(F64=F64, F=F, rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1, slab_stride=n, num_block_stride=0, num=None, G=None, den=None, reg=0.0,
             mode=PREPARE, thr=float(thr), plane_scale=None, terms=0, limbs=0, blockmax=False)
    if form.endswith("planes"):
        a.update(limbs=3, plane_scale=np.full(kp, 2.0 ** 22, np.float32))
    if form.startswith("den"):
        num = (rs.rand(rows_pad, kp) + 0.5).astype(np.float32)
        a.update(mode=PENALTY if form == "den-penalty" else WNMF, num=num.reshape(1, -1), den=num.copy())
    if form == "ring-planes":       # G = 1: F G is the shadow, and so is num
        G = np.zeros((kp, kp), np.float32)
        G[:k, :k] = np.eye(k)
        a.update(mode=WNMF, num=F.reshape(1, -1).copy(), G=G)
    got = launch(a)
    ref = mu_step_ref(a)
    assert np.array_equal(np.where(ok, got["F64"], 0.0), np.where(ok, F64, 0.0))
    want = check_everything_else(a, got, ref["num32"])
    rb, cb = rowbits_to_bool(got["rowbits"], kp), colbits_to_bool(got["colbits"], rows_pad)
    at, above, below = (ok & (F64 == v) for v in (t, up, down))
    assert at.sum() > 3 and above.sum() > 3 and below.sum() > 3
    assert not rb[at].any() and rb[above].all() and not rb[below].any() and np.array_equal(rb, cb)
    assert (got["F"][above] == thr).all() and np.array_equal(rb, want["bits"])


# ---- PREPARE ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kp", [(20, 32), (37, 64)])
@pytest.mark.parametrize("form", ["bf16-2", "blockmax", "planes2", "planes3"])
def test_prepare_mode(form, k, kp):
    """F64 is not written (launch() holds it byte for byte, the junk in its padding included); the shadow -- handed over as markers -- is
    rewritten with zero padding; bits, partials, panel and planes follow; without num the second partial is 0."""
    c = dict(form=form, mode=PREPARE, k=k, kp=kp, rows_pad=512, rows=390, layout="plain", splits=3, reg=1.5, seed=77)
    a = general_inputs(c)
    ok, _ = region_masks(512, 390, k, kp)
    assert a["F64"][~ok].all()
    for with_num in (False, True):
        b = a if with_num else dict(a, num=None)
        ref = mu_step_ref(b)
        got = launch(b)
        assert np.array_equal(got["F64"], a["F64"])
        want = check_everything_else(b, got, ref["num32"])
        assert np.array_equal(got["F"], np.where(ok, a["F64"], 0.0).astype(np.float32))
        assert (want["partials"][:, 0] > 0).all()
        if with_num:
            assert (got["partials"][:, 1] > 0).all()
        else:
            assert not got["partials"][:, 1].any()


# ---- a predicted plane scale that is off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("mode", [PREPARE, PENALTY])
def test_plane_scale_off_by_design(mode, limbs):
    """One column's scale is too large: q clamps at +-QMAX and the digits are those of the clamped value.  Another is one bit low.
    blockmax reports the true maximum in both, which is what lets the caller see that the prediction was off."""
    c = dict(form="planes%d" % limbs, mode=mode, k=20, kp=32, rows_pad=512, rows=500, layout="plain", splits=1, reg=1.5, seed=78)
    a = general_inputs(c)
    new = mu_step_ref(a)["F64"]
    e = 22 - np.floor(np.log2(np.maximum(new.max(axis=0), 1e-30)))        # max 2^e in [2^22, 2^23)
    e[20:] = 0
    e[3] += 3
    e[7] -= 1
    a["plane_scale"] = (2.0 ** e).astype(np.float32)
    ref = mu_step_ref(a)
    got = launch(a)
    if mode != PREPARE:
        check_enclosure(ref, got, "plane scale")
    want = check_everything_else(a, got, ref["num32"])
    q = want["q"]
    assert (q[:, 3] == QMAX).mean() > 0.3 and q[:, 7].max() < 2 ** 22 and q[:, 7].max() >= 2 ** 21 - 1 and 2 ** 22 <= q[:, 5].max() < 2 ** 23
    d = planes_to_digits(got["planes"], 512)
    clamped = q[:, 3] == QMAX
    assert (d[:, clamped, 3] == 127).all()
    assert np.array_equal(got["blockmax"].max(axis=0), want["fn"].astype(np.float32).max(axis=0))
    assert got["blockmax"].max(axis=0)[3] * a["plane_scale"][3] > 2 * QMAX


# ---- refusals and the stop flag --------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_stop_flag():
    from pybmf_amd import _lib as L
    base = dict(form="bf16-2", mode=PENALTY, k=20, kp=32, rows_pad=512, rows=300, layout="plain", splits=3, reg=1.5, seed=9)
    a = general_inputs(base)
    i8 = general_inputs(dict(base, form="planes3"))
    n = 512 * 32
    refused = lambda args, **kw: launch(args, expect=-1, **kw) is None      # noqa: E731
    assert launch(a) is not None and launch(i8) is not None                  # the launches the refusals below are one step away from
    assert L.lib.bmf_mu_epilogue(None, None) == -1                           # null args
    for name in ("F", "F64", "panel", "rowbits", "colbits", "partials"):     # null pointer
        assert refused(a, null=(name,))
    assert refused(a, raw=dict(rows_pad=500)) and refused(a, raw=dict(rows_pad=0))          # rows_pad
    assert refused(a, raw=dict(rows=0)) and refused(a, raw=dict(rows=513))                  # rows
    assert refused(a, raw=dict(kp=48)) and refused(a, raw=dict(k=0)) and refused(a, raw=dict(k=33))
    assert refused(a, raw=dict(mode=3)) and refused(a, raw=dict(mode=-1))
    assert refused(a, null=("num",)) and refused(a, null=("G",))             # update modes need num and G (or den)
    assert refused(a, raw=dict(splits=0)) and refused(a, raw=dict(slab_stride=n - 1))       # slab description
    assert refused(a, raw=dict(terms=4)) and refused(a, raw=dict(terms=-1))
    assert refused(a, ldp=508) and refused(a, ldp=514)                       # ldp < rows_pad, ldp % 4
    assert refused(a, ldcb=512 // 32 - 1)
    assert refused(a, shift=dict(panel=4)) and refused(a, shift=dict(F=4))   # alignment of panel (8) and F (16)
    # planes
    assert refused(i8, raw=dict(terms=1)) and refused(i8, raw=dict(limbs=4)) and refused(i8, raw=dict(limbs=1))
    assert refused(i8, null=("plane_scale",)) and refused(i8, null=("blockmax",))
    assert refused(general_inputs(dict(base, form="planes3", rows_pad=640, rows=600)))      # rows_pad % 512
    assert refused(i8, ldp=520) and refused(i8, shift=dict(planes=8))        # ldp % 16, alignment of planes
    d = general_inputs(dict(base, form="den", splits=1))
    assert launch(d) is not None
    assert refused(dict(d, limbs=3, plane_scale=np.ones(32, np.float32)))    # planes with den
    # the blocked numerator: one slab, blocks that do not overlap
    b = general_inputs(dict(base, form="planes3", layout="blocked", splits=1, kp=64, k=40))
    assert launch(b) is not None
    assert refused(dict(b, num=np.concatenate([b["num"], b["num"]])), raw=dict(splits=2, slab_stride=b["num"].shape[1]))
    assert refused(b, raw=dict(num_block_stride=512 * 32 - 1)) and refused(b, raw=dict(num_block_stride=-512 * 32))
    assert refused(dict(b, terms=2, limbs=0, plane_scale=None), raw=dict(num_block_stride=512 * 32 - 1))
    tight = dict(b, num_block_stride=512 * 32, num=block_num(np.ones((512, 64), np.float32), 512 * 32)[None, :])
    assert launch(tight) is not None                                         # (the smallest stride is accepted)
    # stop != 0 writes nothing, in either kernel; stop = 0 is the plain launch
    assert launch(a, stop=1) is None and launch(i8, stop=1) is None and launch(d, stop=-2) is None and launch(b, stop=7) is None
    for args in (a, i8):
        plain, flagged = launch(args), launch(args, stop=0)
        assert set(plain) == set(flagged) and all(plain[name].tobytes() == flagged[name].tobytes() for name in plain)
