"""The PALM step kernels without a GPU: `palm_step_ref`, an fp64 NumPy restatement of ONE bmf_palm_epilogue call (csrc/palm.hip,
include/bmf_hip.h; PyBMF/models/ELBMF.py:177-208, PRIMP.py:51-88) with every output the launch writes, pinned here against what the
reference produced (tests/golden/g14_palm.*), and the plain helpers tests/test_palm_kernels_gpu.py compares the device with.

What is fp32 on the device is fp32 here: `num` is summed over its slabs in ascending order in np.float32, the extrapolated point is
rounded to fp32 before the Fe G product.  The product itself is accumulated in fp32 by the matrix cores in an order this file does
not restate; the stand-in computes it in fp64 and returns an enclosure [x_lo, x_hi] of x = fe - eta grad instead, of half-width
    b = eta ((kp + 2) 2^-24 (|fe32| @ |G|) + 2^-24 |num|)
-- the standard bound for a dot product of length kp accumulated in fp32 in any order, plus the final rounding.  With `den`, or
with G = 0, nothing is accumulated and b = 0.

The step maps are NOT monotone in x when kai > 0: the reference's prox has no dead zone, so x - kai sign(x) drops by 2 kai at x = 0
and x - kai sign(x - 1) drops by 2 kai at x = 1 (only the jump at 0.5 goes up).  Between those kinks each stage is affine and
increasing, so the image of an interval is enclosed by the values at its end points and at the kinks inside it with their two
neighbours: `step_enclosure`.  Where no kink at 0 or 1 lies inside, that is [step(x_lo), step(x_hi)].
"""
import json
import os

import numpy as np
import pytest

import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ELBMF, PRIMP = 1, 2               # BMF_PALM_*
SPECTRAL, FROBENIUS = 0, 1        # BMF_NORM_*
U24, U53 = 2.0 ** -24, 2.0 ** -53
QMAX = 8355711.0                  # the clamp of the digit planes: 127 + 127 * 256 + 127 * 65536


# ---- the element-wise maps ------------------------------------------------------------------------------------------------------
def step_map(x, kai, lam, variant):
    """ELBMF: prox, negatives to 0 (ELBMF.py:199-210).  PRIMP: proxelbmfnn then _proxelbmfnn (PRIMP.py:51-64, 84-87)."""
    x = np.asarray(x, dtype=np.float64)
    if variant == ELBMF:
        return orc.elbmf_prox(x, kai, lam)
    y = np.maximum(orc.primp_prox(x, kai, lam), 0.0)
    return np.minimum(orc.primp_prox(y, kai, lam), 1.0)


def _stage_enclosure(stage, lo, hi):
    """Hull of stage(x) over lo <= x <= hi for a map that is non-decreasing between the kinks 0, 0.5 and 1.  (A candidate outside the
    interval is clipped onto an end point, which is a candidate already.)"""
    pts = [lo, hi]
    for t in (0.0, 0.5, 1.0):
        for c in (np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)):
            pts.append(np.clip(c, lo, hi))
    vals = np.stack([stage(p) for p in pts])
    return vals.min(axis=0), vals.max(axis=0)


def step_enclosure(x_lo, x_hi, kai, lam, variant):
    """(lo, hi) with lo <= step_map(x) <= hi for every x in [x_lo, x_hi]; both are values the map takes on the interval (ELBMF) or
    the hull of the second stage over the hull of the first (PRIMP)."""
    x_lo, x_hi = np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64)
    if variant == ELBMF:
        return _stage_enclosure(lambda x: orc.elbmf_prox(x, kai, lam), x_lo, x_hi)
    y_lo, y_hi = _stage_enclosure(lambda x: np.maximum(orc.primp_prox(x, kai, lam), 0.0), x_lo, x_hi)
    return _stage_enclosure(lambda y: np.minimum(orc.primp_prox(y, kai, lam), 1.0), y_lo, y_hi)


def step_tol(x, kai, lam):
    """What a fused multiply-add may differ by from NumPy's two roundings, and nothing more: the two branches at a kink differ by
    2 kai + lam, far above it."""
    return 8 * U53 * (np.abs(x) + kai + lam + 1)


def step_size(norms, norm_kind, beta):
    """(eta, L) as the kernel computes them from bmf_sym_norms' output (ELBMF.py:184-185, PRIMP.py:73-80)."""
    L = max(float(norms[0 if norm_kind == SPECTRAL else 1]), 1e-4)
    return (1.0 / (1.1 * L) if beta == 0 else 2.0 * (1.0 - beta) / (1.0 + 2.0 * beta) / L), L


# ---- everything a launch derives from the new factor ------------------------------------------------------------------------------
def digits_of(q):
    """Balanced base-256 digits of integers |q| <= QMAX: (3, ...) in -128..127, q = d0 + 256 d1 + 65536 d2."""
    q = np.asarray(q, dtype=np.int64)
    d0 = ((q + 128) & 255) - 128
    q1 = (q - d0) >> 8
    d1 = ((q1 + 128) & 255) - 128
    return np.stack([d0, d1, (q1 - d1) >> 8])


def derived_outputs(a, F64_new, F64_old, num32):
    """What one launch writes besides F64, from the new fp64 factor (the stand-in's own, or the device's): a dict of
    F, Fprev64, bits (Boolean rows_pad x kp: rowbits and colbits are two layouts of it), partials, blockmax, q and digits (planes),
    dotpart."""
    rows_pad, rows, k, kp = a["rows_pad"], a["rows"], a["k"], a["kp"]
    nb = rows_pad // 128
    ok = (np.arange(rows_pad)[:, None] < rows) & (np.arange(kp)[None, :] < k)
    F32 = F64_new.astype(np.float32)
    out = {"F": F32, "ok": ok}
    out["Fprev64"] = np.where(ok, F64_old, 0.0) if a["advance_prev"] else a["Fprev64"].copy()
    out["bits"] = ok & (F64_new > np.float64(np.float32(a["thr"])))
    out["partials"] = np.array([orc.elbmf_integrality_gap(F64_new[128 * b:128 * (b + 1)][ok[128 * b:128 * (b + 1)]], a["gap_l1"], a["gap_l2"])
                                for b in range(nb)])
    out["blockmax"] = np.abs(F32).reshape(nb, 128, kp).max(axis=1)
    if a.get("plane_scale") is not None:
        scale = np.asarray(a["plane_scale"], dtype=np.float32).astype(np.float64)
        out["q"] = np.rint(np.clip(F64_new * scale[None, :], -QMAX, QMAX)).astype(np.int64)
        out["digits"] = digits_of(out["q"])
    out["dotpart"] = (F64_old * num32.astype(np.float64)).reshape(nb, 128 * kp).sum(axis=1)
    return out


def sum_slabs32(num, n):
    """sum over the slabs in ascending order in fp32, as the kernels add them"""
    s = np.zeros(n, dtype=np.float32)
    for sp in range(num.shape[0]):
        s = s + np.asarray(num[sp, :n], dtype=np.float32)
    return s


def palm_step_ref(a, exact=False):
    """One bmf_palm_epilogue call on host arrays.  `a`: the fields of bmf_palm_args -- F64, Fprev64 (rows_pad x kp fp64), F (the fp32
    shadow: read by the beta = 0 form without `den`, where it must be float32(F64)), rows_pad, rows, k, kp, splits, num
    ([splits][slab_stride] fp32), G (kp x kp fp32, or None with den), norms, norm_kind, variant, beta, l1, l2, gap_l1, gap_l2,
    advance_prev, thr, den (rows_pad x kp fp32 or None), plane_scale (kp fp32 or None).
    exact: G and num taken as fp64 and nothing rounded to fp32 (the pinning against the reference's fp64 steps).
    Returns a dict: F64, x, x_lo, x_hi, lo, hi (the enclosure of the new factor), tol, eta, kai, lam, num32, and derived_outputs()."""
    rows_pad, kp = a["rows_pad"], a["kp"]
    F64, P64 = np.asarray(a["F64"], dtype=np.float64), np.asarray(a["Fprev64"], dtype=np.float64)
    assert F64.shape == P64.shape == (rows_pad, kp)
    beta, den = float(a["beta"]), a.get("den")
    eta, L = step_size(a["norms"], a["norm_kind"], beta)
    kai, lam = a["l1"] * eta, a["l2"] * eta
    fe = F64 if beta == 0 else F64 + beta * (F64 - P64)
    n = rows_pad * kp
    num = np.asarray(a["num"])
    if exact:
        num32 = num[:, :n].astype(np.float64).sum(axis=0).reshape(rows_pad, kp)
    else:
        num32 = sum_slabs32(num, n).reshape(rows_pad, kp)
    if den is not None:
        fg, b = np.asarray(den, dtype=np.float32).astype(np.float64), 0.0
    else:
        if beta == 0 and not exact:   # the form without the inertial term multiplies the shadow it was given
            assert np.array_equal(np.asarray(a["F"], dtype=np.float32), F64.astype(np.float32), equal_nan=True), "F must be float32(F64) on entry"
        fe32 = fe if exact else fe.astype(np.float32).astype(np.float64)
        G = np.asarray(a["G"]).astype(np.float64)
        fg = fe32 @ G
        b = eta * ((kp + 2) * U24 * (np.abs(fe32) @ np.abs(G)) + U24 * np.abs(num32.astype(np.float64))) if G.any() and not exact else 0.0
    x = fe - eta * (fg - num32.astype(np.float64))
    ok = (np.arange(rows_pad)[:, None] < a["rows"]) & (np.arange(kp)[None, :] < a["k"])
    F64_new = np.where(ok, step_map(x, kai, lam, a["variant"]), 0.0)
    lo, hi = step_enclosure(x - b, x + b, kai, lam, a["variant"])
    out = dict(F64=F64_new, x=x, x_lo=x - b, x_hi=x + b, lo=np.where(ok, lo, 0.0), hi=np.where(ok, hi, 0.0),
               tol=step_tol(x, kai, lam), eta=eta, kai=kai, lam=lam, num32=num32)
    out.update(derived_outputs(a, F64_new, F64, num32))
    return out


# ---- the layouts of the bit words and of the digit planes ----------------------------------------------------------------------------
def rowbits_to_bool(words, kp):
    """rowbits: one 64-bit word per row, bit j = column j.  Bits kp..63 must be clear."""
    w = np.ascontiguousarray(words).view(np.uint64)
    assert not (w >> np.uint64(kp)).any() if kp < 64 else True
    return ((w[:, None] >> np.arange(kp, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def colbits_to_bool(words, rows_pad):
    """colbits: [kp][ldcb] 32-bit words, bit r % 32 of word r / 32 = row r.  Returns rows_pad x kp."""
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :rows_pad].T.astype(bool)


def plane_positions(rows_pad):
    """byte position of row r inside a plane column: 512-row groups, inside each the order bmf_panel_pos_i8"""
    from pybmf_amd import _lib as L
    pos = np.array([L.lib.bmf_panel_pos_i8(int(c)) for c in range(512)])
    assert sorted(pos.tolist()) == list(range(512))
    r = np.arange(rows_pad)
    return (r // 512) * 512 + pos[r % 512]


def planes_to_digits(planes, rows_pad):
    """planes [3][kp][ldp] int8 -> digits (3, rows_pad, kp) in row order"""
    return np.asarray(planes)[:, :, plane_positions(rows_pad)].transpose(0, 2, 1).astype(np.int64)


# ---- inputs of the general steps: the grid tests/test_palm_kernels_gpu.py runs, verified here to keep the interval check sharp --------
ROW_CASES = [(128, 1), (128, 127), (128, 128), (512, 1), (512, 127), (512, 128), (512, 129), (512, 500), (512, 512),
             (640, 1), (640, 127), (640, 128), (640, 129), (640, 500), (640, 640)]
K_CASES = [(1, 32), (31, 32), (32, 32), (33, 64), (63, 64), (64, 64)]
FORMS = [("ring", 0.0), ("ring", 0.15), ("ring", 0.9), ("den", 0.0), ("den", 0.15)]


def general_cases():
    """Every (k, form) pair once (30 cases), the row shapes, slab counts, variants and advance_prev cycled through them: 7 is coprime
    to the 15 row shapes, so the first 15 cases already reach each of them (test_general_cases_cover_the_grid).  Then two cases with
    36 blocks, where the ring form permutes its blocks (32 of them, and a plain tail of 4), and one with 68, where the block map reaches a
    round index above 0: 33 in all."""
    cases, i = [], 0
    for form, beta in FORMS:
        for k, kp in K_CASES:
            rows_pad, rows = ROW_CASES[(7 * i + 3) % len(ROW_CASES)]
            cases.append(dict(form=form, beta=beta, k=k, kp=kp, rows_pad=rows_pad, rows=rows, splits=1 if form == "den" else (1, 3)[(i // 2) % 2],
                              variant=(ELBMF, PRIMP)[i % 2], advance_prev=0 if i % 3 == 1 else 1, seed=4100 + i))
            i += 1
    cases.append(dict(form="ring", beta=0.0, k=40, kp=64, rows_pad=4608, rows=4500, splits=3, variant=ELBMF, advance_prev=1, seed=4198))
    cases.append(dict(form="ring", beta=0.15, k=20, kp=32, rows_pad=4608, rows=4481, splits=1, variant=PRIMP, advance_prev=0, seed=4199))
    cases.append(dict(form="ring", beta=0.15, k=33, kp=64, rows_pad=8704, rows=8650, splits=3, variant=ELBMF, advance_prev=1, seed=4200))
    return cases


def case_id(c):
    return "{form}-b{beta}-k{k}-kp{kp}-{rows}of{rows_pad}-s{splits}-v{variant}-a{advance_prev}".format(**c)


def general_inputs(c):
    """Random positive factors, a real Gram, `num` in slabs of mixed sign, scaled so that x straddles 0, 0.5 and 1; junk in the padding
    of F64, Fprev64 and num (the launch must not let it through), zeros in the padding of G (a Gram of k columns has them)."""
    rs = np.random.RandomState(c["seed"])
    rows_pad, rows, k, kp, beta = c["rows_pad"], c["rows"], c["k"], c["kp"], c["beta"]
    n = rows_pad * kp
    F64 = rs.rand(rows_pad, kp) * 1.2
    P64 = F64 + 0.1 * rs.standard_normal((rows_pad, kp))
    H = rs.rand(300, k) * 0.6
    G = np.zeros((kp, kp), np.float32)
    G[:k, :k] = (H.T @ H).astype(np.float32)
    norms = np.array([np.linalg.norm(G.astype(np.float64), 2), np.linalg.norm(G.astype(np.float64))])
    kind = SPECTRAL if c["variant"] == ELBMF else FROBENIUS
    eta, L = step_size(norms, kind, beta)
    # x = fe - eta (fe - target) G moves a row by about (its mean distance to the target) * eta L: a target level per row, scaled so
    # that the move is the same for every step size
    target = 0.6 + (rs.uniform(-2.0, 3.2, (rows_pad, 1)) + 0.3 * rs.standard_normal((rows_pad, kp)) - 0.6) / (eta * L)
    target[:, k:] = 0.0
    total = (target @ G.astype(np.float64)).astype(np.float32)
    total[:, k:] = rs.rand(rows_pad, kp - k)
    total[rows:] += rs.rand(rows_pad - rows, kp).astype(np.float32)
    stride = n + 96
    num = np.full((c["splits"], stride), 3.0, np.float32)
    if c["splits"] == 1:
        num[0, :n] = total.ravel()
    else:
        r = rs.rand(n).astype(np.float32)
        num[0, :n], num[1, :n], num[2, :n] = r * total.ravel(), 2 * (1 - r) * total.ravel(), -(1 - r) * total.ravel()
    a = dict(F64=F64, Fprev64=P64, F=F64.astype(np.float32), rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=c["splits"], num=num,
             slab_stride=stride, G=G, norms=norms, norm_kind=kind, variant=c["variant"],
             beta=beta, l1=0.02 * norms[0], l2=0.05 * norms[0], gap_l1=0.3, gap_l2=1.7, advance_prev=c["advance_prev"], thr=0.5, den=None,
             plane_scale=None)
    if c["form"] == "den":   # the masked gradient: den - num, one array each, G unused
        fe = F64 + beta * (F64 - P64)
        a["den"] = (fe @ G.astype(np.float64)).astype(np.float32) + rs.rand(rows_pad, kp).astype(np.float32) * 0.01
        a["G"] = None
    elif rows_pad % 512 == 0:   # the planes: power-of-two column scales, two of them driving the larger values into the clamp
        e = 16 + (np.arange(kp) * 5) % 7
        e[0], e[k - 1] = 24, 23
        a["plane_scale"] = (2.0 ** e).astype(np.float32)
    return a


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g14():
    z = np.load(os.path.join(GOLDEN, "g14_palm.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "g14_palm.json")))
    n = int(z["shape"][1])
    return z, meta, np.unpackbits(z["X"], axis=1)[:, :n].astype(np.float64)


def exact_args(X, F, Fprev, other, l1, l2, beta, variant, advance_prev):
    """The arguments of one step of factor F against `other` with num and G in fp64, padded to the kernel's shapes."""
    rows, k = F.shape
    rows_pad, kp = -(-rows // 128) * 128, 32
    pad = lambda M, shape: np.pad(M, [(0, s - d) for s, d in zip(shape, M.shape)])   # noqa: E731
    G = other.T @ other
    return dict(F64=pad(F, (rows_pad, kp)), Fprev64=pad(Fprev, (rows_pad, kp)), F=None, rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1,
                num=pad(X @ other, (rows_pad, kp)).reshape(1, -1), slab_stride=rows_pad * kp, G=pad(G, (kp, kp)),
                norms=np.array([np.linalg.norm(G, 2), np.linalg.norm(G)]), norm_kind=SPECTRAL if variant == ELBMF else FROBENIUS, variant=variant,
                beta=beta, l1=l1, l2=l2, gap_l1=0.0, gap_l2=0.0, advance_prev=advance_prev, thr=0.5, den=None, plane_scale=None)


# ---- pinning ----------------------------------------------------------------------------------------------------------------------------
def test_prox_reproduces_the_reference(g14):
    z, meta, _ = g14
    for i, (kai, lam) in enumerate(meta["prox_params"]):
        np.testing.assert_allclose(step_map(z["prox_in"], kai, lam, ELBMF), z[f"prox_out_{i}"], rtol=0, atol=1e-15)
        # PRIMP's first stage is the same expression
        np.testing.assert_allclose(np.maximum(orc.primp_prox(z["prox_in"], kai, lam), 0.0), z[f"prox_out_{i}"], rtol=0, atol=1e-15)


def test_whole_steps_reproduce_the_reference(g14):
    z, meta, X = g14
    m, n = X.shape
    k = z["U0"].shape[1]
    for i, p in enumerate(meta["steps"]):
        a = exact_args(X, z["U0"], z["U_prev"], z["V0"], p["reg_l1"], p["reg_l2"], p["beta"], ELBMF, 1)
        r = palm_step_ref(a, exact=True)
        np.testing.assert_allclose(r["F64"][:m, :k], z[f"step{i}_U"], rtol=1e-10)
        assert np.array_equal(r["Fprev64"][:m, :k], z["U0"]) and not r["F64"][m:].any() and not r["F64"][:, k:].any()
        a = exact_args(X.T, z["V0"], z["V0"], z[f"step{i}_U"], p["reg_l1"], p["reg_l2"], p["beta"], ELBMF, 1)
        np.testing.assert_allclose(palm_step_ref(a, exact=True)["F64"][:n, :k], z[f"step{i}_V"], rtol=1e-10)
    for i, p in enumerate(meta["primp_steps"]):   # the same function, the other variant: Frobenius step size, anchor left alone
        a = exact_args(X, z["U0"], z["U_prev"], z["V0"], p["l1reg"], p["l2reg"] * p["tau"], p["beta"], PRIMP, 0)
        r = palm_step_ref(a, exact=True)
        np.testing.assert_allclose(r["F64"][:m, :k], z[f"pstep{i}_U"], rtol=1e-10)
        assert np.array_equal(r["Fprev64"], a["Fprev64"])


def test_fp32_parts_are_restated_as_fp32():
    a = general_inputs(dict(form="ring", beta=0.15, k=5, kp=32, rows_pad=128, rows=100, splits=3, variant=ELBMF, advance_prev=1, seed=1))
    a["num"][:, 0] = (1e8, 1.0, -1e8)       # ascending in fp32: (1e8 + 1) - 1e8 = 0, any other order or fp64 gives 1
    r = palm_step_ref(a)
    assert r["num32"].dtype == np.float32 and r["num32"][0, 0] == 0.0
    # the enclosure holds an fp32 accumulation of the product in either direction
    fe32 = (a["F64"] + a["beta"] * (a["F64"] - a["Fprev64"])).astype(np.float32)
    for order in (range(32), range(31, -1, -1)):
        acc = np.zeros((128, 32), np.float32)
        for s in order:
            acc = acc + fe32[:, s:s + 1] * a["G"][s:s + 1, :]
        x = (a["F64"] + a["beta"] * (a["F64"] - a["Fprev64"])) - r["eta"] * (acc.astype(np.float64) - r["num32"].astype(np.float64))
        assert (r["x_lo"] <= x).all() and (x <= r["x_hi"]).all()
    assert (r["x_hi"] - r["x_lo"])[:100, :5].max() < 1e-4 * np.abs(r["x"]).max()   # (the cell that holds 1e8 apart)
    # no accumulation, no width: den given, or G = 0
    a["G"] = np.zeros_like(a["G"])
    r = palm_step_ref(a)
    assert np.array_equal(r["x_lo"], r["x"]) and np.array_equal(r["x_hi"], r["x"])
    b = general_inputs(dict(form="den", beta=0.0, k=5, kp=32, rows_pad=128, rows=100, splits=1, variant=PRIMP, advance_prev=0, seed=2))
    r = palm_step_ref(b)
    assert np.array_equal(r["x_lo"], r["x"]) and np.array_equal(r["x_hi"], r["x"])
    assert np.array_equal(r["x"], b["F64"] - r["eta"] * (b["den"].astype(np.float64) - b["num"][0, :128 * 32].reshape(128, 32).astype(np.float64)))
    # the form without the inertial term reads the shadow: a stale one is refused
    c = general_inputs(dict(form="ring", beta=0.0, k=5, kp=32, rows_pad=128, rows=100, splits=1, variant=ELBMF, advance_prev=1, seed=3))
    c["F"] = c["F"] + 1
    with pytest.raises(AssertionError):
        palm_step_ref(c)


# ---- the shape of the step maps -------------------------------------------------------------------------------------------------------------
PARAMS = [(0.0, 0.0), (0.0, 0.3), (0.01, 0.0), (0.02, 0.3), (0.0625, 0.25), (0.4, 2.0)]


def dense_grid():
    kinks = [0.0, 0.5, 1.0]
    near = [np.nextafter(t, d) for t in kinks for d in (-np.inf, np.inf)] + [5e-324, -5e-324]
    return np.unique(np.concatenate([np.linspace(-0.7, 1.9, 20801), kinks, near]))


def test_step_maps_are_monotone_between_the_kinks_and_drop_at_0_and_1():
    x = dense_grid()
    for kai, lam in PARAMS:
        for variant in (ELBMF, PRIMP):
            y = step_map(x, kai, lam, variant)
            if kai == 0:      # soft threshold switched off: non-decreasing everywhere, the jump at 0.5 included
                assert (np.diff(y) >= 0).all(), (kai, lam, variant)
        # with kai > 0, ELBMF's map is non-decreasing on each piece ...  (The piecewise shape is asserted for ELBMF only.  PRIMP is two
        # such stages composed, and the interval check does not rest on its shape: step_enclosure takes the hull stage by stage, and
        # test_step_enclosure_holds_every_value_on_a_dense_grid holds that hull against every value of both maps.)
        y = step_map(x, kai, lam, ELBMF)
        for piece in (x < 0, (x > 0) & (x <= 0.5), (x > 0.5) & (x < 1), x > 1):
            assert (np.diff(y[piece]) >= 0).all(), (kai, lam)
        if kai > 0:           # ... and falls at 0 and at 1, by 2 kai / (1 + lam) between the neighbours (the clamp at 0 hides one half)
            at = lambda t: step_map(np.array([np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)]), kai, lam, ELBMF)   # noqa: E731
            assert at(0.0)[0] == pytest.approx(kai / (1 + lam), rel=1e-12) and at(0.0)[1] == 0 and at(0.0)[2] == 0
            assert at(1.0)[0] - at(1.0)[2] == pytest.approx(2 * kai / (1 + lam), rel=1e-12) and at(1.0)[1] == pytest.approx(1.0, abs=1e-15)
            assert at(0.5)[2] - at(0.5)[1] == pytest.approx((2 * kai + lam) / (1 + lam), rel=1e-12)


def test_step_enclosure_holds_every_value_on_a_dense_grid():
    x = dense_grid()
    rs = np.random.RandomState(77)
    i0 = rs.randint(0, len(x) - 1, 4000)
    i1 = np.minimum(i0 + rs.randint(0, 60, 4000) * (rs.rand(4000) < 0.8), len(x) - 1).astype(int)
    for kai, lam in PARAMS:
        for variant in (ELBMF, PRIMP):
            y = step_map(x, kai, lam, variant)
            lo, hi = step_enclosure(x[i0], x[i1], kai, lam, variant)
            cs_min = np.array([y[a:b + 1].min() for a, b in zip(i0, i1)])
            cs_max = np.array([y[a:b + 1].max() for a, b in zip(i0, i1)])
            assert (lo <= cs_min).all() and (cs_max <= hi).all(), (kai, lam, variant)
            one = i0 == i1   # a point interval is the value itself
            assert np.array_equal(lo[one], y[i0[one]]) and np.array_equal(hi[one], y[i0[one]])
            if variant == ELBMF:    # attained: the hull is of values the map takes on the interval
                assert np.array_equal(lo, cs_min) and np.array_equal(hi, cs_max)
            # away from the falls at 0 and 1 it is the pair the end points give
            plain = ~(((x[i0] <= 0) & (x[i1] >= 0)) | ((x[i0] <= 1) & (x[i1] >= 1)))
            if variant == ELBMF:
                assert np.array_equal(lo[plain], y[i0][plain]) and np.array_equal(hi[plain], y[i1][plain])


# ---- the derived outputs and the layouts ---------------------------------------------------------------------------------------------------
def test_digits_carry():
    q = np.array([0, 1, -1, 127, 128, -128, -129, 255, 256, 32639, 32640, 32767, 32768, -32768, -32769, 65535, 65536, 8355711, -8355711])
    d = digits_of(q)
    assert d.min() >= -128 and d.max() <= 127 and np.array_equal(d[0] + 256 * d[1] + 65536 * d[2], q)
    assert d[:, 4].tolist() == [-128, 1, 0] and d[:, 12].tolist() == [0, -128, 1] and d[:, -2].tolist() == [127, 127, 127]
    rs = np.random.RandomState(5)
    q = rs.randint(-8355711, 8355712, 100000)
    d = digits_of(q)
    assert d.min() >= -128 and d.max() <= 127 and np.array_equal(d[0] + 256 * d[1] + 65536 * d[2], q)


def test_bit_layouts():
    rs = np.random.RandomState(6)
    for kp in (32, 64):
        B = rs.rand(256, kp) < 0.4
        words = (B.astype(np.uint64) << np.arange(kp, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)
        assert np.array_equal(rowbits_to_bool(words.view(np.int64), kp), B)
        cols = np.zeros((kp, 10), np.uint32)     # ldcb = 10 > 256 / 32
        for r, j in zip(*np.nonzero(B)):
            cols[j, r // 32] |= np.uint32(1) << np.uint32(r % 32)
        assert np.array_equal(colbits_to_bool(cols.view(np.int32), 256), B)
    with pytest.raises(AssertionError):
        rowbits_to_bool(np.array([1 << 40], dtype=np.uint64), 32)


def test_derived_outputs_on_a_hand_made_block():
    kp, rows_pad = 32, 128
    F = np.zeros((rows_pad, kp))
    F[0, :4] = (0.25, 0.75, 1.5, 0.5)
    F[3, 1] = 0.6
    F[2, 5] = 9.0        # a padded column and
    F[7, 0] = 9.0        # a padded row: neither counts
    old = np.full((rows_pad, kp), 2.0)
    a = dict(rows_pad=rows_pad, rows=5, k=4, kp=kp, advance_prev=1, thr=0.5, gap_l1=1.0, gap_l2=2.0, Fprev64=np.ones((rows_pad, kp)),
             plane_scale=np.full(kp, 4.0, np.float32))
    d = derived_outputs(a, F, old, np.ones((rows_pad, kp), np.float32))
    assert d["bits"].sum() == 3 and d["bits"][0, 1] and d["bits"][0, 2] and d["bits"][3, 1] and not d["bits"][0, 3]
    dist = np.array([0.25, 0.25, 0.5, 0.5, 0.4])
    assert d["partials"][0] == pytest.approx((dist + 2 * dist ** 2).sum(), rel=1e-14)
    assert d["Fprev64"].sum() == 2.0 * 5 * 4 and d["Fprev64"][5:].sum() == 0
    assert d["blockmax"][0, 0] == 9.0 and d["blockmax"][0, 2] == 1.5 and d["q"][0, :4].tolist() == [1, 3, 6, 2]
    assert d["dotpart"][0] == 2.0 * rows_pad * kp
    a["advance_prev"] = 0
    assert np.array_equal(derived_outputs(a, F, old, np.ones((rows_pad, kp), np.float32))["Fprev64"], a["Fprev64"])


# ---- the inputs of the general steps keep the interval check sharp ---------------------------------------------------------------------------
def test_general_cases_cover_the_grid():
    cases = general_cases()
    assert {(c["rows_pad"], c["rows"]) for c in cases} >= set(ROW_CASES)
    assert {(c["form"], c["beta"], c["k"], c["kp"]) for c in cases} >= {(f, b, k, kp) for f, b in FORMS for k, kp in K_CASES}
    ring = [c for c in cases if c["form"] == "ring"]
    for kp in (32, 64):
        for hasbeta in (False, True):      # the four ring instantiations, each with both slab counts, variants and advance_prev
            sub = [c for c in ring if c["kp"] == kp and (c["beta"] != 0) == hasbeta]
            assert {c["splits"] for c in sub} == {1, 3} and {c["variant"] for c in sub} == {ELBMF, PRIMP} and {c["advance_prev"] for c in sub} == {0, 1}
        sub = [c for c in cases if c["form"] == "den" and c["kp"] == kp]   # the first form at this NT
        assert {c["beta"] for c in sub} == {0.0, 0.15} and {c["variant"] for c in sub} == {ELBMF, PRIMP} and {c["advance_prev"] for c in sub} == {0, 1}
    assert any(c["rows_pad"] % 512 == 0 and c["form"] == "ring" and c["kp"] == kp and (c["beta"] != 0) == hb for c in cases
               for kp in (32, 64) for hb in (False, True))
    assert len({case_id(c) for c in cases}) == len(cases) == 33
    ring_blocks = {c["rows_pad"] // 128 for c in cases if c["form"] == "ring"}      # the permuted block map: one round and a tail; two rounds
    assert any(32 <= nb < 64 and nb % 32 for nb in ring_blocks) and any(nb >= 64 and nb % 32 for nb in ring_blocks)


@pytest.mark.parametrize("c", general_cases(), ids=case_id)
def test_general_inputs_give_narrow_intervals_that_straddle_the_kinks(c):
    a = general_inputs(c)
    r = palm_step_ref(a)
    ok = r["ok"]
    width = (r["hi"] - r["lo"])[ok]
    assert (width < 1e-5).mean() >= 0.9, (width < 1e-5).mean()
    assert (r["lo"] <= r["F64"]).all() and (r["F64"] <= r["hi"]).all()
    x = r["x"][ok]
    if x.size >= 500:
        for lo, hi in ((-np.inf, 0), (0, 0.5), (0.5, 1), (1, np.inf)):
            assert ((x > lo) & (x < hi)).mean() > 0.03, (lo, hi, ((x > lo) & (x < hi)).mean())
        assert np.abs(r["F64"] - a["F64"])[ok].mean() > 0.05      # the step changes the factor: old and new are told apart
    if a["plane_scale"] is not None and x.size >= 500:
        assert (np.abs(r["q"]) == QMAX).any() and (np.abs(r["q"][ok]) < QMAX).mean() > 0.5
        assert (np.abs(r["digits"][2]) > 1).any() and (r["digits"][1] < 0).any()
