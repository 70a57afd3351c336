"""bmf_palm_epilogue and the small kernels beside it (csrc/palm.hip) called directly, element by element, against the stand-in of
tests/test_palm_kernels_cpu.py: exact inputs at the kinks of the prox, general steps held inside the enclosure of the fp32 product,
and everything else one launch writes checked against the device's own F64 (exact, or 1e-12 for the two fp64 sums).

Every output buffer is pre-filled with a marker and has guard slots behind it that must keep the marker; the inputs of a launch must
come back byte for byte.  The fp32 shadow F is an INPUT of the form without inertial term and without `den` (it is the operand of
the F G product there): that form gets float32(F64), every other one the marker.
"""
import ctypes as C

import numpy as np
import pytest

from test_palm_kernels_cpu import (ELBMF, FROBENIUS, PRIMP, SPECTRAL, case_id, colbits_to_bool, derived_outputs, general_cases, general_inputs,
                                   palm_step_ref, planes_to_digits, rowbits_to_bool, step_size, sum_slabs32)

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


def launch(a, planes=False, blockmax=False, dotpart=False, stop=None, ldcb=None, ldp=None, expect=0, reads_shadow=None):
    """One bmf_palm_epilogue call on the host arrays of `a` (the dict palm_step_ref takes).  Returns the outputs as host arrays in
    their logical shapes; the guards, the unused columns of colbits and planes, and the inputs are checked here.  expect = -1: the
    call must refuse and leave every buffer as it was."""
    import torch
    from pybmf_amd import _lib as L
    rows_pad, kp, splits = a["rows_pad"], a["kp"], a["splits"]
    n, nb = rows_pad * kp, max(rows_pad // 128, 1)
    ldcb = -(-rows_pad // 32) + 3 if ldcb is None else ldcb
    ldp = rows_pad + 32 if ldp is None else ldp
    if reads_shadow is None:
        reads_shadow = a["beta"] == 0 and a["den"] is None
    bufs = {"F64": with_guard(a["F64"], torch.float64), "Fprev64": with_guard(a["Fprev64"], torch.float64),
            "F": with_guard(a["F"], torch.float32) if reads_shadow else marked(n + GUARD, torch.float32),
            "rowbits": marked(rows_pad + GUARD, torch.int64), "colbits": marked(kp * max(ldcb, 1) + GUARD, torch.int32),
            "partials": marked(nb + GUARD, torch.float64), "blockmax": marked(nb * kp + GUARD, torch.float32),
            "planes": marked(3 * kp * ldp + GUARD, torch.int8), "dotpart": marked(nb + GUARD, torch.float64)}
    ins = {"num": dev(a["num"]), "norms": dev(np.asarray(a["norms"], dtype=np.float64))}
    for name, dt in (("G", np.float32), ("den", np.float32), ("plane_scale", np.float32)):
        if a.get(name) is not None:
            ins[name] = dev(np.asarray(a[name], dtype=dt))
    if stop is not None:
        ins["stop"] = dev(np.array([stop], dtype=np.int32))
    before = {k_: v.cpu().numpy().tobytes() for k_, v in {**bufs, **ins}.items()}
    p = L.PalmArgs()
    p.F64, p.Fprev64, p.F = bufs["F64"].data_ptr(), bufs["Fprev64"].data_ptr(), bufs["F"].data_ptr()
    p.rows_pad, p.rows, p.k, p.kp, p.splits = rows_pad, a["rows"], a["k"], kp, splits
    p.num, p.slab_stride = ins["num"].data_ptr(), a["slab_stride"]
    p.G = ins["G"].data_ptr() if "G" in ins else None
    p.norms, p.norm_kind, p.variant, p.beta = ins["norms"].data_ptr(), a["norm_kind"], a["variant"], a["beta"]
    p.l1, p.l2, p.gap_l1, p.gap_l2, p.advance_prev, p.thr = a["l1"], a["l2"], a["gap_l1"], a["gap_l2"], a["advance_prev"], a["thr"]
    p.rowbits, p.colbits, p.ldcb, p.partials = bufs["rowbits"].data_ptr(), bufs["colbits"].data_ptr(), ldcb, bufs["partials"].data_ptr()
    p.blockmax = bufs["blockmax"].data_ptr() if blockmax or planes else None
    p.stop = ins["stop"].data_ptr() if stop is not None else None
    p.den = ins["den"].data_ptr() if "den" in ins else None
    if planes:
        p.planes, p.ldp, p.plane_scale = bufs["planes"].data_ptr(), ldp, ins["plane_scale"].data_ptr()
    p.dotpart = bufs["dotpart"].data_ptr() if dotpart else None
    rc = L.lib.bmf_palm_epilogue(C.byref(p), None)
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
    cb = host["colbits"][:-GUARD].reshape(kp, ldcb)
    assert (cb[:, rows_pad // 32:] == MARK).all(), "colbits beyond rows_pad / 32"
    out = {"F64": host["F64"][:n].reshape(rows_pad, kp), "Fprev64": host["Fprev64"][:n].reshape(rows_pad, kp), "F": host["F"][:n].reshape(rows_pad, kp),
           "rowbits": host["rowbits"][:rows_pad], "colbits": cb[:, :rows_pad // 32], "partials": host["partials"][:nb]}
    for name, asked in (("blockmax", blockmax or planes), ("dotpart", dotpart), ("planes", planes)):
        if not asked:
            assert (host[name] == MARK).all(), f"{name} was written without being asked for"
    if blockmax or planes:
        out["blockmax"] = host["blockmax"][:nb * kp].reshape(nb, kp)
    if dotpart:
        out["dotpart"] = host["dotpart"][:nb]
    if planes:
        pl = host["planes"][:-GUARD].reshape(3, kp, ldp)
        assert (pl[:, :, rows_pad:] == MARK).all(), "planes beyond rows_pad"
        out["planes"] = pl[:, :, :rows_pad]
    return out


def check_everything_else(a, got, num32):
    """What the launch writes besides F64, against the device's own F64.

    partials and the padding: the inputs carry junk in the padding of F64, Fprev64 and num, so a gap taken from the step's value
    BEFORE the padding is zeroed, or a new factor that keeps that value, would count it and miss the 1e-12 here (and the zeros
    above).  That is the fault this guards against.  Once the padding is zeroed its distance to {0, 1} is 0 and it adds nothing
    to the gap, so the kernel's `if (ok)` around the gap cannot be observed from outside: outputs are identical without it."""
    rows_pad, kp = a["rows_pad"], a["kp"]
    want = derived_outputs(a, got["F64"], a["F64"], num32)
    ok = want["ok"]
    assert got["F"].tobytes() == want["F"].tobytes()                                   # the shadow, bit for bit
    assert not got["F64"][~ok].any() and not got["F"][~ok].any()                       # padding rows and columns: zero
    assert got["Fprev64"].tobytes() == want["Fprev64"].tobytes()                       # advanced (padding zeroed) or left alone, byte for byte
    rb, cb = rowbits_to_bool(got["rowbits"], kp), colbits_to_bool(got["colbits"], rows_pad)
    assert np.array_equal(rb, want["bits"]) and np.array_equal(cb, want["bits"]) and not rb[~ok].any() and not cb[~ok].any()
    np.testing.assert_allclose(got["partials"], want["partials"], rtol=1e-12, atol=0)
    if "blockmax" in got:
        assert got["blockmax"].tobytes() == want["blockmax"].tobytes()
    if "planes" in got:
        d = planes_to_digits(got["planes"], rows_pad)
        assert np.array_equal(d[0] + 256 * d[1] + 65536 * d[2], want["q"]) and np.array_equal(d, want["digits"])
        assert not d[:, ~ok].any()
    if "dotpart" in got:
        np.testing.assert_allclose(got["dotpart"], want["dotpart"], rtol=1e-12, atol=1e-300)


# ---- kinks: exact inputs --------------------------------------------------------------------------------------------------------------
def kink_values(kai, extra=()):
    v = [0.0, 5e-324, -5e-324, kai, -kai, np.nextafter(kai, np.inf), np.nextafter(kai, -np.inf),
         0.5, np.nextafter(0.5, 1), np.nextafter(0.5, 0), 1.0, 1 + kai, 1 - kai, 1.5, -3.0, 7.0,
         # first prox of PRIMP below 0.5, above 0.5, above 1 (from either side of 1)
         0.3, 0.45, 0.6, 0.97, 1.4]
    v += list(extra)
    if len(v) % 2 == 0:       # an odd count: with kp a power of two, cycling through the values then reaches every column with every value
        v.append(0.75)
    return np.array(v, dtype=np.float64)


def kink_factor(values, rows_pad, rows, k, kp):
    """values cycled through the whole padded factor; each one must sit in a full tile, in the last valid row or column, and in the padding"""
    F = values[np.arange(rows_pad * kp) % len(values)].reshape(rows_pad, kp)
    r, c = np.arange(rows_pad)[:, None], np.arange(kp)[None, :]
    ok = (r < rows) & (c < k)
    regions = (ok & (r < 128), (ok & (r == rows - 1)) | (ok & (c == k - 1)), ~ok)
    for v in values:
        hit = F.view(np.int64) == np.float64(v).view(np.int64)
        assert all((hit & reg).any() for reg in regions), v
    return F


KINK_FORMS = ["ring", "ring_beta", "den", "den_beta"]


@pytest.mark.parametrize("k,kp", [(20, 32), (37, 64)])
@pytest.mark.parametrize("variant", [ELBMF, PRIMP])
@pytest.mark.parametrize("form", KINK_FORMS)
def test_kinks_with_exact_inputs(form, variant, k, kp):
    """grad = 0 (G = 0 and num = 0, or den = num) and beta = 0 or Fprev = F: x = f exactly, the test decides the branch."""
    rows_pad, rows = 256, 200
    beta = 0.5 if form.endswith("beta") else 0.0
    # (norms, norm_kind, l1, l2): eta = 1 and 0.5 from two different norms read both ways, and the 1e-4 floor of L
    round_norms = np.array([0.5, 1.0]) if beta else np.array([1 / 1.1, 2 / 1.1])
    for norms, kind, l1, l2, eta_want in ((round_norms, SPECTRAL, 0.0625, 0.25, 1.0), (round_norms, FROBENIUS, 0.0625, 0.25, 0.5),
                                          (np.zeros(2), SPECTRAL, 1e-5, 3e-5, None)):
        eta, L = step_size(norms, kind, beta)
        assert eta_want is None or eta == eta_want
        assert eta_want is not None or L == 1e-4
        kai, lam = l1 * eta, l2 * eta
        F = kink_factor(kink_values(kai), rows_pad, rows, k, kp)
        n = rows_pad * kp
        rs = np.random.RandomState(k)
        a = dict(F64=F, Fprev64=F.copy() if beta else rs.rand(rows_pad, kp), F=F.astype(np.float32), rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1,
                 num=np.zeros((1, n), np.float32), slab_stride=n, G=np.zeros((kp, kp), np.float32), norms=norms, norm_kind=kind, variant=variant, beta=beta,
                 l1=l1, l2=l2, gap_l1=0.3, gap_l2=1.7, advance_prev=1, thr=0.5, den=None, plane_scale=None)
        if form.startswith("den"):
            a["num"] = (rs.rand(1, n) * 3).astype(np.float32)
            a["den"], a["G"] = a["num"].reshape(rows_pad, kp).copy(), None
        ref = palm_step_ref(a)
        assert np.array_equal(ref["x"], F) and np.array_equal(ref["x_lo"], F) and (ref["kai"], ref["lam"]) == (kai, lam)
        got = launch(a, blockmax=True, dotpart=not form.startswith("den"))
        err = np.abs(got["F64"] - ref["F64"])
        assert (err <= ref["tol"]).all(), (form, variant, kind, np.argwhere(err > ref["tol"])[:5], err.max())
        check_everything_else(a, got, ref["num32"])


@pytest.mark.parametrize("form", ["ring", "den"])
@pytest.mark.parametrize("k,kp", [(20, 32), (37, 64)])
def test_threshold_is_strict(form, k, kp):
    """l1 = l2 = 0: the step is the identity on f >= 0, so the test places entries at the threshold and one step above it."""
    rows_pad, rows = 256, 200
    thr = np.float32(0.3)
    t = np.float64(thr)
    up, down = np.nextafter(t, np.inf), np.nextafter(t, -np.inf)
    F = kink_factor(kink_values(0.0, extra=(t, up, down)), rows_pad, rows, k, kp)
    n = rows_pad * kp
    for variant in (ELBMF, PRIMP):
        a = dict(F64=F, Fprev64=F.copy(), F=F.astype(np.float32), rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1, num=np.zeros((1, n), np.float32),
                 slab_stride=n, G=np.zeros((kp, kp), np.float32), norms=np.array([0.5, 1.0]), norm_kind=SPECTRAL, variant=variant, beta=0.0, l1=0.0, l2=0.0,
                 gap_l1=1.0, gap_l2=0.0, advance_prev=0, thr=float(thr), den=None, plane_scale=None)
        if form == "den":
            a["den"], a["G"] = np.zeros((rows_pad, kp), np.float32), None
        got = launch(a)
        ok = (np.arange(rows_pad)[:, None] < rows) & (np.arange(kp)[None, :] < k)
        want = np.where(ok, np.maximum(F, 0.0) if variant == ELBMF else np.clip(F, 0.0, 1.0), 0.0)
        assert np.array_equal(got["F64"], want)
        rb, cb = rowbits_to_bool(got["rowbits"], kp), colbits_to_bool(got["colbits"], rows_pad)
        at, above, below = (ok & (F == v) for v in (t, up, down))
        assert at.sum() > 3 and above.sum() > 3 and below.sum() > 3
        assert not rb[at].any() and rb[above].all() and not rb[below].any() and np.array_equal(rb, cb)
        check_everything_else(a, got, np.zeros((rows_pad, kp), np.float32))


# ---- general steps: the interval check, and everything else the launch writes --------------------------------------------------------------
@pytest.mark.parametrize("c", general_cases(), ids=case_id)
def test_general_steps_stay_inside_the_enclosure(c):
    a = general_inputs(c)
    ref = palm_step_ref(a)
    ring = c["form"] == "ring"
    planes = ring and a["plane_scale"] is not None
    got = launch(a, planes=planes, blockmax=ring, dotpart=ring)
    # every entry: lo - tol <= F64 <= hi + tol, (lo, hi) = the image of [x_lo, x_hi] under the step map; where neither fall of the map
    # (at 0 and at 1) lies inside the interval these are step(x_lo) and step(x_hi)
    below, above = ref["lo"] - ref["tol"] - got["F64"], got["F64"] - ref["hi"] - ref["tol"]
    assert (below <= 0).all() and (above <= 0).all(), (np.argwhere((below > 0) | (above > 0))[:5], below.max(), above.max())
    check_everything_else(a, got, ref["num32"])
    # the optional outputs do not change the step, and a second launch on equal inputs gives the same bytes everywhere
    plain = launch(a)
    assert plain["F64"].tobytes() == got["F64"].tobytes()
    again = launch(a, planes=planes, blockmax=ring, dotpart=ring)
    assert set(again) == set(got)
    for name in got:
        assert again[name].tobytes() == got[name].tobytes(), name


# ---- refusals and the stop flag --------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_stop_flag():
    base = dict(form="ring", beta=0.0, k=20, kp=32, rows_pad=512, rows=300, splits=3, variant=ELBMF, advance_prev=1, seed=9)
    a = general_inputs(base)
    assert launch(a, planes=True, dotpart=True) is not None                           # the launch the refusals below are one step away from
    assert launch(dict(a, rows_pad=500), expect=-1, reads_shadow=True) is None         # rows_pad % 128
    assert launch(dict(a, k=33), expect=-1) is None                                   # k > kp
    assert launch(dict(a, beta=1.0), expect=-1, reads_shadow=True) is None             # beta = 1
    assert launch(a, ldcb=512 // 32 - 1, expect=-1) is None                           # ldcb too small
    assert launch(a, planes=True, ldp=496, expect=-1) is None                          # (ldp < rows_pad)
    d = general_inputs(dict(base, form="den", splits=1))
    two = dict(d, splits=2, num=np.concatenate([d["num"], d["num"]]))
    assert launch(two, expect=-1) is None                                             # den with splits = 2
    assert launch(dict(d, plane_scale=np.ones(32, np.float32)), planes=True, expect=-1) is None     # planes with den
    assert launch(d, dotpart=True, expect=-1) is None                                 # (dotpart with den)
    e = general_inputs(dict(base, rows_pad=640, rows=600))
    assert launch(dict(e, plane_scale=np.ones(32, np.float32)), planes=True, expect=-1) is None     # planes with rows_pad = 640
    # stop != 0 writes nothing, in either form; stop = 0 is the plain launch
    assert launch(a, planes=True, dotpart=True, stop=1) is None
    assert launch(dict(a, beta=0.15), planes=True, dotpart=True, stop=-2) is None
    assert launch(d, stop=1) is None
    assert launch(a, stop=0)["F64"].tobytes() == launch(a)["F64"].tobytes()


# ---- the small kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4096 * 256 + 77])      # one pass, and more elements than the capped grid has threads
def test_extrapolate(n):
    import torch
    from pybmf_amd._lib import check, lib, ptr
    rs = np.random.RandomState(n % 1000)
    f, p = rs.rand(n) * 2 - 0.5, rs.rand(n) * 2 - 0.5
    f[:4], p[:4] = (0.0, 1.0, 5e-324, -3.0), (0.0, 1.0, 1.0, -3.0)
    fd, pd = dev(f), dev(p)
    for beta in (0.0, 0.15, 0.9):
        out = marked(n + GUARD, torch.float32)
        check(lib.bmf_palm_extrapolate(ptr(fd), ptr(pd), beta, n, ptr(out), None), "bmf_palm_extrapolate")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n:] == MARK).all()
        want = (f + beta * (f - p)).astype(np.float32)
        if beta == 0:
            assert got[:n].tobytes() == f.astype(np.float32).tobytes()
        ulp = np.spacing(np.abs(want))       # one fp32 ulp: the fused multiply-add may round the fp64 value the other way
        assert (np.abs(got[:n].astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        assert (got[:n] != want).mean() < 1e-3
    assert fd.cpu().numpy().tobytes() == f.tobytes() and pd.cpu().numpy().tobytes() == p.tobytes()
    assert lib.bmf_palm_extrapolate(ptr(fd), ptr(pd), 1.0, n, ptr(out), None) == -1 and (out.cpu().numpy()[n:] == MARK).all()


@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("splits", [1, 3])
def test_dot_slabs(splits, blocks):
    import torch
    from pybmf_amd._lib import check, lib, ptr
    rs = np.random.RandomState(10 * splits + blocks)
    n, stride = 5003, 5003 + 61
    F = rs.rand(n) + 0.1
    slabs = np.full((splits, stride), 1e6, np.float32)
    slabs[:, :n] = rs.rand(splits, n) * 3
    Fd, sd = dev(F), dev(slabs)
    part = marked(blocks + GUARD, torch.float64)
    check(lib.bmf_dot_slabs(ptr(Fd), ptr(sd), stride, splits, n, ptr(part), blocks, None), "bmf_dot_slabs")
    torch.cuda.synchronize()
    got = part.cpu().numpy()
    assert (got[blocks:] == MARK).all()
    terms = F * sum_slabs32(slabs, n).astype(np.float64)          # the slab sum in fp32, the product and the sum in fp64
    e = np.arange(n)
    want = np.array([terms[(e // 256) % blocks == b].sum() for b in range(blocks)])    # block b: the 256-element chunks b, b + blocks, ...
    np.testing.assert_allclose(got[:blocks], want, rtol=1e-12)
    assert got[:blocks].sum() == pytest.approx(terms.sum(), rel=1e-12)
    assert lib.bmf_dot_slabs(ptr(Fd), ptr(sd), n - 1, splits, n, ptr(part), blocks, None) == -1     # stride < n


@pytest.mark.parametrize("nd,kk,nu,nv", [(1024, 64 * 64, 1500, 300), (5, 32 * 32 + 3, 3, 1), (300, 1, 1024, 2000)])
def test_palm_scalars(nd, kk, nu, nv):
    import torch
    from pybmf_amd._lib import check, lib, ptr
    rs = np.random.RandomState(nd)
    dot, gu, gv, pu, pv = (rs.rand(s) + 0.01 for s in (nd, kk, kk, nu, nv))
    want = [dot.sum(), (gu * gv).sum(), pu.sum(), pv.sum()]
    d = [dev(np.concatenate([x, np.full(9, 1e9)])) for x in (dot, gu, gv, pu, pv)]      # what lies behind each input is not summed
    counts = dev(np.array([11, 22, 33, 44], dtype=np.int64))
    out = marked(6 + GUARD, torch.float64)
    args = (ptr(d[0]), nd, ptr(d[1]), ptr(d[2]), kk, ptr(d[3]), nu, ptr(d[4]), nv)
    check(lib.bmf_palm_scalars(*args, ptr(counts), ptr(out), None), "bmf_palm_scalars")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:4], want, rtol=1e-12)
    assert got[4] == 11.0 and got[5] == 22.0 and (got[6:] == MARK).all()
    assert counts.cpu().numpy().tolist() == [0, 0, 33, 44]
    # counts = NULL is accepted: the four sums again, words 4 and 5 left alone
    out = marked(6 + GUARD, torch.float64)
    check(lib.bmf_palm_scalars(*args, None, ptr(out), None), "bmf_palm_scalars")
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert again[:4].tobytes() == got[:4].tobytes() and (again[4:] == MARK).all()
    assert lib.bmf_palm_scalars(ptr(d[0]), 0, ptr(d[1]), ptr(d[2]), kk, ptr(d[3]), nu, ptr(d[4]), nv, None, ptr(out), None) == -1
