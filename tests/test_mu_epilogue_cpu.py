"""The MU update epilogue without a GPU: `mu_step_ref`, an fp64 NumPy restatement of ONE bmf_mu_epilogue call (csrc/epilogue.hip,
include/bmf_hip.h; PyBMF/models/BinaryMFPenalty.py:136-163, WNMF.py:96-109) with every output the launch writes, pinned here against
the oracle's factor updates, and the plain helpers tests/test_mu_epilogue_gpu.py compares the device with.

What is fp32 on the device is fp32 here: `num` is summed over its slabs in ascending order in np.float32 (read through either layout:
plain [splits][rows_pad][kp], or 32-column blocks [kp/32][rows_pad][32] `num_block_stride` apart), `den` is taken as given, the
shadow is float32(F64).  The F G product is accumulated in fp32 by the matrix cores in an order this file does not restate; the
stand-in computes it in fp64 from the fp32 shadow and returns an enclosure [lo, hi] of the new factor instead, from the half-width
    b = (kp + 2) 2^-24 (|F32| @ |G|)
of the product -- the standard bound for a dot product of length kp accumulated in fp32 in any order, plus the final rounding; the
rule the PALM stand-in uses for the same MFMA.  With `den`, or with G = 0, nothing is accumulated and b = 0.

For non-negative f, num, G and reg the new entry f (nume / den) is decreasing in den (and every rounding on the way is monotone), so
the enclosure is [step(den + b), step(den - b)], both clamps applied (den == 0 -> eps; PENALTY: fn == 0 -> eps).
"""
import numpy as np
import pytest

import oracle as orc
from test_palm_kernels_cpu import QMAX, U24, U53, colbits_to_bool, digits_of, planes_to_digits, rowbits_to_bool, sum_slabs32  # noqa: F401

PREPARE, PENALTY, WNMF = 0, 1, 2     # BMF_MODE_*
EPS = orc.EPS
MUTANTS = ("three", "regf", "cube", "slabs", "layout")


# ---- the numerator through either layout ---------------------------------------------------------------------------------------------
def block_num(total, stride, fill=0.0, tail=0):
    """rows_pad x kp -> the blocked layout as one flat slab: block j (columns 32 j .. 32 j + 31, [rows_pad][32]) at j * stride, `fill` in
    the gaps between the blocks and in `tail` elements behind the last one"""
    rows_pad, kp = total.shape
    assert stride >= rows_pad * 32 and kp % 32 == 0
    flat = np.full((kp // 32 - 1) * stride + rows_pad * 32 + tail, fill, dtype=total.dtype)
    for j in range(kp // 32):
        flat[j * stride:j * stride + rows_pad * 32] = total[:, 32 * j:32 * j + 32].ravel()
    return flat


def unblock_num(flat, rows_pad, kp, stride):
    return np.concatenate([flat[j * stride:j * stride + rows_pad * 32].reshape(rows_pad, 32) for j in range(kp // 32)], axis=1)


def read_num32(a, exact=False, mutant=None):
    """The numerator one launch sees: rows_pad x kp, fp32 (fp64 with exact).  `num` is [splits][>= slab_stride] or None."""
    rows_pad, kp = a["rows_pad"], a["kp"]
    n = rows_pad * kp
    if a.get("num") is None:
        return np.zeros((rows_pad, kp), np.float64 if exact else np.float32)
    num = np.asarray(a["num"])
    assert num.ndim == 2 and num.shape[0] == a["splits"]
    stride = a.get("num_block_stride", 0)
    if stride and mutant != "layout":
        assert a["splits"] == 1
        out = unblock_num(num[0], rows_pad, kp, stride)
        return out.astype(np.float64) if exact else out + np.float32(0)      # 0 + x, as the kernel starts its sum
    if exact:
        return num[:, :n].astype(np.float64).sum(axis=0).reshape(rows_pad, kp)
    return sum_slabs32(num[:-1] if mutant == "slabs" else num, n).reshape(rows_pad, kp)


# ---- everything a launch derives from the new factor -----------------------------------------------------------------------------------
def bf16_addends(F32, terms, F64=None):
    """The panel's addends: (terms, ...) uint16 bf16 bits, each the round-to-nearest-even bf16 of what the earlier ones left (fp32).
    F64: the first addend is rounded from the fp64 entry instead of from its fp32 shadow.  The two differ only where the shadow lies
    exactly halfway between two bf16 values and the fp64 entry does not: one rounding then goes to the side the fp64 entry is on, two
    roundings go to even.  Both are a nearest bf16 of the shadow, and the remainders are exact either way."""
    rem = np.asarray(F32, dtype=np.float32).copy()
    out = []
    for t in range(terms):
        u = rem.view(np.uint32).astype(np.uint64)
        b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
        if t == 0 and F64 is not None:
            tie = ((u & 0xFFFF) == 0x8000) & (np.abs(F64) != np.abs(rem.astype(np.float64)))
            b = np.where(tie, (u >> 16).astype(np.uint32) + (np.abs(F64) > np.abs(rem.astype(np.float64))), b).astype(np.uint32)
        out.append(b.astype(np.uint16))
        rem = rem - (b << 16).astype(np.uint32).view(np.float32)
    return np.stack(out)


def derived_outputs(a, F64_new, num32):
    """What one launch writes besides F64, from the new fp64 factor (the stand-in's own, or the device's; what it holds in the padding is
    taken as zero, which is what the launch uses there): F, ok, bits (rowbits and colbits are two layouts of it), partials (nb x 2) with
    ptol0 (the tolerance of partials[:, 0]), blockmax, and with plane_scale q, digits (3 limbs) and q2, digits2 (2 limbs)."""
    rows_pad, rows, k, kp = a["rows_pad"], a["rows"], a["k"], a["kp"]
    nb = rows_pad // 128
    ok = (np.arange(rows_pad)[:, None] < rows) & (np.arange(kp)[None, :] < k)
    fn = np.where(ok, F64_new, 0.0)
    F32 = fn.astype(np.float32)
    out = {"F": F32, "ok": ok, "fn": fn}
    out["bits"] = ok & (fn > np.float64(np.float32(a["thr"])))
    d = fn * fn - fn
    blocks = lambda M: M.reshape(nb, 128 * kp).sum(axis=1)   # noqa: E731
    out["partials"] = np.stack([blocks(d * d), blocks(fn * np.where(ok, num32, 0).astype(np.float64))], axis=1)
    # fn * fn - fn may be one fused multiply-add on the device: d differs by up to 2^-53 fn^2 from the two roundings here, d^2 by 2 |d| of it
    out["ptol0"] = 1e-12 * out["partials"][:, 0] + blocks(2 * np.abs(d) * fn * fn * 2.0 ** -52)
    out["blockmax"] = np.abs(F32).reshape(nb, 128, kp).max(axis=1)
    if a.get("plane_scale") is not None:
        scale = np.asarray(a["plane_scale"], dtype=np.float32).astype(np.float64)
        out["q"] = np.rint(np.clip(fn * scale[None, :], -QMAX, QMAX)).astype(np.int64)
        out["digits"] = digits_of(out["q"])
        out["q2"] = np.floor((out["q"] + 128) / 256).astype(np.int64)        # two limbs: the lowest digit rounded away
        out["digits2"] = digits_of(out["q2"])[:2]
        assert not digits_of(out["q2"])[2].any()
    return out


def mu_step_ref(a, exact=False, mutant=None):
    """One bmf_mu_epilogue call on host arrays.  `a`: the fields of bmf_epilogue_args -- F64 (rows_pad x kp fp64), F (the fp32 shadow, read
    by the update without `den`: float32(F64) on the valid part, zero in the padding), rows_pad, rows, k, kp, num ([splits][>=
    slab_stride] fp32 or None), splits, slab_stride, num_block_stride, G (kp x kp fp32, or None with den), den (rows_pad x kp fp32 or
    None), reg, mode, thr, plane_scale (kp fp32 or None).
    exact: G and num taken as fp64 and nothing rounded to fp32 (the pinning against the oracle's fp64 updates).
    mutant: one term wrong, see MUTANTS (test_general_inputs_give_sharp_enclosures_that_no_mutant_stays_inside).
    Returns a dict: F64 (the centre: the step with the fp64 product), lo, hi (the enclosure of the new factor), tol, num32, and
    derived_outputs() of F64.

    tol = 16 * 2^-53 * value.  Derived, not tuned: everything in the element-wise part is a sum, product or quotient of non-negative
    terms, so nothing cancels and every rounding adds at most 2^-53 to the relative error of the result.  The device evaluates
        f2 = f f;  nume = num + (3 reg) f2;  den' = den + ((2 reg) (f2 f) + reg f);  fn = f (nume / den')
    -- at most 8 roundings of positive terms along the way to fn (f2, f2 f, the two products with reg, two sums, the quotient, the
    product with f), and the stand-in as many: 16 in all.  The compiler may contract a product and a sum into one fused multiply-add,
    which removes a rounding and adds none.  The clamps compare with 0 exactly and are not touched by any of it."""
    rows_pad, kp, mode = a["rows_pad"], a["kp"], a["mode"]
    F64 = np.asarray(a["F64"], dtype=np.float64)
    assert F64.shape == (rows_pad, kp) and mode in (PREPARE, PENALTY, WNMF)
    ok = (np.arange(rows_pad)[:, None] < a["rows"]) & (np.arange(kp)[None, :] < a["k"])
    num32 = read_num32(a, exact, mutant)
    if mode == PREPARE:
        new = lo = hi = np.where(ok, F64, 0.0)
        out = dict(F64=new, lo=lo, hi=hi, tol=np.zeros_like(new), num32=num32)
        out.update(derived_outputs(a, new, num32))
        return out
    reg = float(a["reg"]) if mode == PENALTY else 0.0
    f, num = F64, num32.astype(np.float64)
    if a.get("den") is not None:
        fg, b = np.asarray(a["den"], dtype=np.float32).astype(np.float64), 0.0
    else:
        G = np.asarray(a["G"]).astype(np.float64)
        if exact:
            f32 = F64
        else:
            f32 = np.asarray(a["F"], dtype=np.float32)
            assert np.array_equal(f32[ok], F64.astype(np.float32)[ok]) and not f32[~ok].any(), "F must be float32(F64), zero in the padding"
            f32 = f32.astype(np.float64)
        assert (G >= 0).all() and (f32 >= 0).all()
        fg = f32 @ G
        b = (kp + 2) * U24 * (np.abs(f32) @ np.abs(G)) if G.any() and not exact else 0.0
    assert (f[ok] >= 0).all() and (num[ok] >= 0).all() and (fg[ok] >= 0).all() and reg >= 0      # what the monotonicity rests on

    def step(den):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):       # (the padding holds junk; it is zeroed below)
            nume = num
            if mode == PENALTY:
                f2 = f * f
                nume = nume + (2.0 if mutant == "three" else 3.0) * reg * f2
                den = den + (2.0 * reg * (f2 if mutant == "cube" else f2 * f) + (0.0 if mutant == "regf" else reg * f))
            den = np.where(den == 0.0, EPS, den)
            fn = f * (nume / den)
            if mode == PENALTY:
                fn = np.where(fn == 0.0, EPS, fn)
        return np.where(ok, fn, 0.0)

    new, lo, hi = step(fg), step(fg + b), step(np.maximum(fg - b, 0.0))
    out = dict(F64=new, lo=lo, hi=hi, tol=16 * U53 * hi, num32=num32)
    out.update(derived_outputs(a, new, num32))
    return out


# ---- inputs of the general steps: the grid tests/test_mu_epilogue_gpu.py runs, verified here to keep the interval check sharp ---------
FORMS = {  # name: (terms, limbs, blockmax, den)
    "bf16-1": (1, 0, False, False), "bf16-2": (2, 0, False, False), "bf16-3": (3, 0, False, False), "plain": (0, 0, False, False),
    "blockmax": (0, 0, True, False), "den": (0, 0, False, True), "planes2": (0, 2, True, False), "planes3": (0, 3, True, False)}
ROW_CASES = [(128, 1), (128, 127), (128, 128), (512, 129), (512, 512), (640, 500)]
PLANE_ROW_CASES = [(512, 129), (512, 512), (4608, 4500), (8704, 8650)]   # 36 blocks: 32 permuted and a plain tail of 4; 68: round 1
K_CASES = [(1, 32), (31, 32), (32, 32), (33, 64), (63, 64), (64, 64)]
REGS = [0.0, 1.5, 1e10]
LAYOUTS = [("plain", 1), ("plain", 3), ("blocked", 1)]


def general_cases():
    """30 launches of the kernel without planes (six forms, five each) and 12 of the one with planes, every axis cycled with a step
    coprime to its length rather than multiplied out (test_general_cases_cover_the_grid)."""
    cases = []
    for i in range(30):
        form = ("bf16-1", "bf16-2", "bf16-3", "plain", "blockmax", "den")[i // 5]
        (k, kp), (rows_pad, rows), (layout, splits) = K_CASES[i % 6], ROW_CASES[(5 * i + 2) % 6], LAYOUTS[i % 3]
        mode = WNMF if i % 4 == 3 else PENALTY
        cases.append(dict(form=form, mode=mode, k=k, kp=kp, rows_pad=rows_pad, rows=rows, layout=layout, splits=splits,
                          reg=REGS[(i // 2) % 3] if mode == PENALTY else 2.5, seed=5100 + i))
    # mu_epilogue_i8_kernel<NT, MODE, LIMBS>: (limbs, mode, index into K_CASES, PLANE_ROW_CASES, LAYOUTS), written out so that each
    # of the eight instances and both large shapes with both limb counts and the blocked numerator at kp = 64 are there
    table = [(2, PENALTY, 3, 2, 2), (3, PENALTY, 4, 3, 2), (2, WNMF, 5, 3, 2), (3, WNMF, 0, 0, 0), (2, PENALTY, 1, 2, 1), (3, PENALTY, 2, 3, 0),
             (2, WNMF, 2, 1, 2), (3, WNMF, 3, 2, 2), (2, WNMF, 1, 3, 1), (3, PENALTY, 0, 0, 1), (2, PENALTY, 5, 1, 0), (3, WNMF, 4, 2, 0)]
    for i, (limbs, mode, ki, si, li) in enumerate(table):
        (k, kp), (rows_pad, rows), (layout, splits) = K_CASES[ki], PLANE_ROW_CASES[si], LAYOUTS[li]
        cases.append(dict(form="planes%d" % limbs, mode=mode, k=k, kp=kp, rows_pad=rows_pad, rows=rows, layout=layout, splits=splits,
                          reg=REGS[i % 3] if mode == PENALTY else 2.5, seed=5200 + i))
    return cases


def case_id(c):
    return "{form}-m{mode}-k{k}-kp{kp}-{rows}of{rows_pad}-{layout}{splits}-reg{reg:g}".format(**c)


def general_inputs(c):
    """Random positive factors, a real Gram, a non-negative `num` (in slabs of mixed sign when there are three) that puts the ratio
    around 1; finite junk in the padding rows and columns of F64 and of every num slab, and between the blocks of the blocked layout;
    zeros in the padding of the shadow and of G, as the header requires.  With reg = 1e10 the Gram and the numerator are scaled by 2^33
    so that no term of the update is lost against another (the mutants below must stay visible).  In WNMF mode `reg` is set and must be
    ignored."""
    rs = np.random.RandomState(c["seed"])
    rows_pad, rows, k, kp, mode = c["rows_pad"], c["rows"], c["k"], c["kp"], c["mode"]
    terms, limbs, blockmax, with_den = FORMS[c["form"]]
    n = rows_pad * kp
    s = 2.0 ** 33 if c["reg"] == 1e10 else 1.0
    ok = (np.arange(rows_pad)[:, None] < rows) & (np.arange(kp)[None, :] < k)
    F64 = np.where(ok, rs.rand(rows_pad, kp) * 1.1 + 0.05, rs.rand(rows_pad, kp) * 5 + 1)
    F = np.where(ok, F64, 0.0).astype(np.float32)
    H = rs.rand(40, k) * 0.5
    G = np.zeros((kp, kp), np.float32)
    G[:k, :k] = (H.T @ H * s).astype(np.float32)
    fg = F.astype(np.float64) @ G.astype(np.float64)
    total = (fg * rs.uniform(0.3, 1.9, (rows_pad, kp)) + s * 0.1 * rs.rand(rows_pad, kp)).astype(np.float32)
    total[~ok] = (s * (1 + rs.rand(rows_pad, kp))).astype(np.float32)[~ok]
    a = dict(F64=F64, F=F, rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=c["splits"], slab_stride=n + 96, num_block_stride=0, G=G, den=None,
             reg=c["reg"], mode=mode, thr=0.5, plane_scale=None, terms=terms, limbs=limbs, blockmax=blockmax)
    if c["layout"] == "blocked":
        a["num_block_stride"] = rows_pad * 32 + 160
        a["num"] = block_num(total, a["num_block_stride"], fill=np.float32(3 * s), tail=96)[None, :]
        a["slab_stride"] = n
    else:
        num = np.full((c["splits"], n + 96), 3 * s, np.float32)
        if c["splits"] == 1:
            num[0, :n] = total.ravel()
        else:
            r = rs.rand(n).astype(np.float32)
            num[0, :n], num[1, :n], num[2, :n] = r * total.ravel(), 2 * (1 - r) * total.ravel(), -(1 - r) * total.ravel()
        a["num"] = num
    if with_den:      # the masked path: the contraction part of the denominator as one array, G unused
        a["den"] = (fg * rs.uniform(0.8, 1.2, (rows_pad, kp)) + s * 0.01 * rs.rand(rows_pad, kp)).astype(np.float32)
        a["G"] = None
    if limbs:         # power-of-two column scales, two of them driving the larger values into the clamp
        e = 16 + (np.arange(kp) * 5) % 7
        e[0], e[k - 1] = 24, 23
        a["plane_scale"] = (2.0 ** e).astype(np.float32)
    return a


# ---- pinning ----------------------------------------------------------------------------------------------------------------------------
def exact_args(X, F, other, reg, mode):
    """The arguments of one update of factor F against `other` with num and G in fp64, padded to the kernel's shapes."""
    rows, k = F.shape
    rows_pad, kp = -(-rows // 128) * 128, 32
    pad = lambda M, shape: np.pad(M, [(0, s - d) for s, d in zip(shape, M.shape)])   # noqa: E731
    return dict(F64=pad(F, (rows_pad, kp)), F=None, rows_pad=rows_pad, rows=rows, k=k, kp=kp, splits=1, slab_stride=rows_pad * kp,
                num=pad(X @ other, (rows_pad, kp)).reshape(1, -1), num_block_stride=0, G=pad(other.T @ other, (kp, kp)), den=None, reg=reg,
                mode=mode, thr=0.5, plane_scale=None)


def test_whole_updates_reproduce_the_oracle():
    rs = np.random.RandomState(11)
    m, n, k = 150, 70, 7
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    U, V = np.abs(rs.standard_normal((m, k))) * 0.5, np.abs(rs.standard_normal((n, k))) * 0.5
    U[3], V[5, 2], X[9] = 0.0, 0.0, 0.0         # den == 0 (reg = 0), a zero entry, a zero numerator: both clamps
    for reg in (0.0, 2.0, 1e10):
        Vn = mu_step_ref(exact_args(X.T, V, U, reg, PENALTY), exact=True)["F64"]
        np.testing.assert_allclose(Vn[:n, :k], orc.penalty_update_V_reassoc(X, U, V, reg), rtol=1e-13, atol=0)
        np.testing.assert_allclose(Vn[:n, :k], orc.penalty_update_V(X, None, U, V, reg), rtol=1e-13, atol=0)
        assert not Vn[n:].any() and not Vn[:, k:].any()
        Un = mu_step_ref(exact_args(X, U, Vn[:n, :k], reg, PENALTY), exact=True)["F64"]
        np.testing.assert_allclose(Un[:m, :k], orc.penalty_update_U_reassoc(X, U, Vn[:n, :k], reg), rtol=1e-13, atol=0)
        if reg == 0:
            assert (Un[3, :k] == EPS).all() and (Un[9, :k] == EPS).all() and Vn[5, 2] == EPS
    Vn = mu_step_ref(exact_args(X.T, V, U, 7.0, WNMF), exact=True)["F64"]          # reg is ignored; no factor == 0 -> eps clamp
    Un = mu_step_ref(exact_args(X, U, Vn[:n, :k], 7.0, WNMF), exact=True)["F64"]
    Uo, Vo = orc.wnmf_update(X, None, U, V)
    np.testing.assert_allclose(Vn[:n, :k], Vo, rtol=1e-13, atol=0)
    np.testing.assert_allclose(Un[:m, :k], Uo, rtol=1e-13, atol=0)
    assert not Un[3, :k].any() and not Un[9, :k].any() and Vn[5, 2] == 0
    # PREPARE: the factor itself, padding taken as zero
    a = exact_args(X, U, V, 0.0, PREPARE)
    a["F64"][m:] = 3.0
    r = mu_step_ref(a)
    assert np.array_equal(r["F64"][:m, :k], U) and not r["F64"][m:].any()


def test_fp32_parts_are_restated_as_fp32():
    c = dict(form="plain", mode=PENALTY, k=5, kp=32, rows_pad=128, rows=100, layout="plain", splits=3, reg=1.5, seed=1)
    a = general_inputs(c)
    a["num"][:, 0] = (1e8, 1.0, -1e8)       # ascending in fp32: (1e8 + 1) - 1e8 = 0, any other order or fp64 gives 1
    r = mu_step_ref(a)
    assert r["num32"].dtype == np.float32 and r["num32"][0, 0] == 0.0
    # the enclosure holds an fp32 accumulation of the product in either direction
    f32 = a["F"]
    for order in (range(32), range(31, -1, -1)):
        acc = np.zeros((128, 32), np.float32)
        for s in order:
            acc = acc + f32[:, s:s + 1] * a["G"][s:s + 1, :]
        got = mu_step_ref(dict(a, den=acc, G=None))["F64"]
        assert (r["lo"] <= got).all() and (got <= r["hi"]).all()
    # no accumulation, no width: den given, or G = 0
    r = mu_step_ref(dict(a, G=np.zeros_like(a["G"])))
    assert np.array_equal(r["lo"], r["F64"]) and np.array_equal(r["hi"], r["F64"])
    r = mu_step_ref(general_inputs(dict(c, form="den")))
    assert np.array_equal(r["lo"], r["F64"]) and np.array_equal(r["hi"], r["F64"])
    # a stale shadow, or one with junk in the padding, is refused
    for bad in (a["F"] + 1, np.where(a["F"] == 0, np.float32(2), a["F"])):
        with pytest.raises(AssertionError):
            mu_step_ref(dict(a, F=bad))


# ---- the derived outputs and the layouts ---------------------------------------------------------------------------------------------------
def test_blocked_numerator_round_trip():
    rs = np.random.RandomState(3)
    for kp in (32, 64):
        total = rs.rand(256, kp).astype(np.float32)
        stride = 256 * 32 + 40
        flat = block_num(total, stride, fill=np.float32(9), tail=7)
        assert flat.size == (kp // 32 - 1) * stride + 256 * 32 + 7 and (flat == 9).sum() == (kp // 32 - 1) * 40 + 7
        assert np.array_equal(unblock_num(flat, 256, kp, stride), total)
        assert flat[stride * (kp // 32 - 1) + 5 * 32 + 3] == total[5, kp - 32 + 3]         # the kernel's index: block, row, column inside
        a = dict(rows_pad=256, kp=kp, splits=1, num=flat[None, :], num_block_stride=stride)
        assert np.array_equal(read_num32(a), total) and read_num32(a).dtype == np.float32
        if kp == 64:     # read as plain [rows_pad][64] it is another matrix
            assert (read_num32(a, mutant="layout") != total).mean() > 0.9


def test_two_limb_digits_round_trip():
    rs = np.random.RandomState(4)
    q = np.concatenate([rs.randint(-8355711, 8355712, 100000), [0, 127, 128, -128, -129, 8355711, -8355711, 32639, 32640]])
    q = np.resize(q, (128 * 782, 1))                                  # (cycled up to whole blocks)
    d = derived_outputs(dict(rows_pad=q.size, rows=q.size, k=1, kp=1, thr=0.5, plane_scale=np.array([2.0 ** 20], np.float32)),
                        q / 2.0 ** 20, np.zeros(q.shape, np.float32))
    assert np.array_equal(d["q"], q)
    q2, d2 = d["q2"][:, 0], d["digits2"][:, :, 0]
    assert d2.shape[0] == 2 and d2.min() >= -128 and d2.max() <= 127 and np.array_equal(d2[0] + 256 * d2[1], q2)
    assert np.abs(256 * q2 - q[:, 0]).max() <= 128                    # what two limbs keep of q: its nearest multiple of 256
    assert d2[:, 100005].tolist() == [127, 127] and d2[:, 100008].tolist() == [-128, 1] and d2[:, 100007].tolist() == [127, 0]


def test_bf16_addends():
    x = np.array([0.0, 1.0, 1.00390625, 1.01171875, 0.3, 2.2204460492503131e-16, 3.0e38, 0.1, 1 - 2.0 ** -24], np.float32)
    b = bf16_addends(x, 3)
    val = (b.astype(np.uint32) << 16).view(np.float32)
    assert val[0].tolist()[:4] == [0.0, 1.0, 1.0, 1.015625]           # ties to even: 1 + 2^-8 down, 1 + 3 2^-8 up
    assert np.array_equal(val.astype(np.float64).sum(axis=0), x.astype(np.float64))        # three addends hold an fp32 exactly
    assert (np.abs(val[0] - x) <= np.abs(x) * 2.0 ** -8).all()
    # rounded from fp64: the same, but for a shadow on a tie under an fp64 value that is not
    x64 = x.astype(np.float64)
    assert np.array_equal(bf16_addends(x, 3, x64), b)
    x64[2:4] = np.nextafter(x64[2:4], [9.0, 0.0])                     # just above 1 + 2^-8, just below 1 + 3 2^-8: the shadows stay
    b64 = bf16_addends(x, 3, x64)
    v64 = (b64.astype(np.uint32) << 16).view(np.float32)
    assert v64[0].tolist()[:4] == [0.0, 1.0, 1.0078125, 1.0078125] and np.array_equal(b64[:, [0, 1, 4, 5, 6, 7, 8]], b[:, [0, 1, 4, 5, 6, 7, 8]])
    assert np.array_equal(v64.astype(np.float64).sum(axis=0), x.astype(np.float64))


def test_derived_outputs_on_a_hand_made_block():
    kp, rows_pad = 32, 128
    F = np.zeros((rows_pad, kp))
    F[0, :4] = (0.25, 0.75, 1.5, 0.5)
    F[3, 1] = 0.6
    F[2, 5] = 9.0        # a padded column and
    F[7, 0] = 9.0        # a padded row: neither counts
    a = dict(rows_pad=rows_pad, rows=5, k=4, kp=kp, thr=0.5, plane_scale=np.full(kp, 4.0, np.float32))
    num = np.full((rows_pad, kp), 2.0, np.float32)
    d = derived_outputs(a, F, num)
    assert d["bits"].sum() == 3 and d["bits"][0, 1] and d["bits"][0, 2] and d["bits"][3, 1] and not d["bits"][0, 3]
    assert d["partials"][0, 0] == pytest.approx(2 * 0.1875 ** 2 + 0.75 ** 2 + 0.25 ** 2 + 0.24 ** 2, rel=1e-14)
    assert d["partials"][0, 1] == pytest.approx(2 * (0.25 + 0.75 + 1.5 + 0.5 + 0.6), rel=1e-14)
    assert d["blockmax"][0, 0] == 0.25 and d["blockmax"][0, 2] == 1.5 and d["blockmax"][0, 5] == 0 and d["q"][0, :4].tolist() == [1, 3, 6, 2]
    assert 0 < d["ptol0"][0] < 1e-11


# ---- the inputs of the general steps keep the interval check sharp ---------------------------------------------------------------------------
def test_general_cases_cover_the_grid():
    cases = general_cases()
    assert 36 <= len(cases) <= 44 and len({case_id(c) for c in cases}) == len(cases)
    assert {c["form"] for c in cases} == set(FORMS) and {c["mode"] for c in cases} == {PENALTY, WNMF}
    assert {(c["k"], c["kp"]) for c in cases} == set(K_CASES) and {c["reg"] for c in cases if c["mode"] == PENALTY} == set(REGS)
    assert {(c["layout"], c["splits"], c["kp"]) for c in cases} == {("plain", 1, 32), ("plain", 3, 32), ("blocked", 1, 32),
                                                                    ("plain", 1, 64), ("plain", 3, 64), ("blocked", 1, 64)}
    planes = [c for c in cases if FORMS[c["form"]][1]]
    assert {(c["rows_pad"], c["rows"]) for c in cases if c not in planes} == set(ROW_CASES)
    assert {(c["rows_pad"], c["rows"]) for c in planes} == set(PLANE_ROW_CASES)
    # every instance of the two kernel templates that an update launches (PREPARE: test_prepare_mode on the GPU side)
    assert {(c["kp"], c["mode"], FORMS[c["form"]][1]) for c in planes} == {(kp, m, l) for kp in (32, 64) for m in (PENALTY, WNMF) for l in (2, 3)}
    assert {(FORMS[c["form"]][0], c["kp"]) for c in cases if c not in planes} == {(t, kp) for t in range(4) for kp in (32, 64)}
    for shape in PLANE_ROW_CASES[2:]:      # the permuted block map: with both limb counts, and under the blocked numerator at kp = 64
        sub = [c for c in planes if (c["rows_pad"], c["rows"]) == shape]
        assert {FORMS[c["form"]][1] for c in sub} == {2, 3} and any(c["layout"] == "blocked" and c["kp"] == 64 for c in sub)
    for form in FORMS:                     # every launch form in both modes, and PENALTY with a regulariser
        sub = [c for c in cases if c["form"] == form]
        assert {c["mode"] for c in sub} == {PENALTY, WNMF} and any(c["reg"] > 0 and c["mode"] == PENALTY for c in sub)
        assert {c["kp"] for c in sub} == {32, 64} and len({c["layout"] for c in sub}) == 2


def outside(a, r, mutant):
    """fraction of the valid cells where the mutant's value leaves the enclosure plus tolerance"""
    m = mu_step_ref(a, mutant=mutant)["F64"]
    ok = r["ok"]
    return ((m < r["lo"] - r["tol"]) | (m > r["hi"] + r["tol"]))[ok].mean()


@pytest.mark.parametrize("c", general_cases(), ids=case_id)
def test_general_inputs_give_sharp_enclosures_that_no_mutant_stays_inside(c):
    a = general_inputs(c)
    r = mu_step_ref(a)
    ok, kp = r["ok"], c["kp"]
    assert (r["lo"] <= r["F64"]).all() and (r["F64"] <= r["hi"]).all() and (r["lo"][ok] > 0).all()
    assert ((r["hi"] - r["lo"]) <= (kp + 2) * 2.0 ** -22 * r["hi"]).all()            # sharp: twice the product's relative bound
    if a["den"] is not None:
        assert np.array_equal(r["lo"], r["hi"])
    assert not r["F64"][~ok].any() and np.isfinite(r["F64"]).all()
    assert np.abs(r["F64"] - a["F64"])[ok].mean() > 0.05                               # the step changes the factor
    if ok.sum() >= 500:
        assert 0.2 < r["bits"][ok].mean() < 0.8
    # mutants: a condition on the inputs, checked on the stand-in alone
    if c["mode"] == PENALTY and c["reg"] > 0:
        for mutant in ("three", "regf", "cube"):
            assert outside(a, r, mutant) >= 0.5, (mutant, outside(a, r, mutant))
    if c["splits"] > 1:
        assert outside(a, r, "slabs") >= 0.5, outside(a, r, "slabs")
    if c["layout"] == "blocked" and kp == 64:
        assert outside(a, r, "layout") >= 0.5, outside(a, r, "layout")
    if a["plane_scale"] is not None and ok.sum() >= 500:
        assert (np.abs(r["q"]) == QMAX).any() and (np.abs(r["q"][ok]) < QMAX).mean() > 0.5
        assert (np.abs(r["digits"][2]) > 1).any() and (r["digits"][1] < 0).any() and (r["digits2"][0] < 0).any()
