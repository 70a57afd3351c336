"""The real-valued WNMF kernels by direct C ABI calls, cell by cell: csrc/xf_f32.hip (tile_f32_kernel, frag_f32_kernel,
frag_rows_bf16_kernel, frag_bf16x3_kernel, xf_f32_kernel<1|2>, xf_f32_ring_kernel<1|2>, xf_f32_bf3_ring_kernel,
xf_f32_resid_ring_kernel<false|true>), frag_rows_f32_kernel of csrc/resid_f32.hip, and real_update_kernel with the C loop of
csrc/wnmf_real.hip.

tests/real_kernels_ref.py restates the orders and makes the exact inputs, tests/test_real_kernels_cpu.py proves them.  A contraction is
checked SLAB BY SLAB: slab s must equal the exact partial product over its own stages (or groups of 8), which names the launch path --
the ring kernels split by stages of 64 reduction indices, the direct kernel by groups of 8 -- and catches a stage taken from a
neighbour, dropped or counted twice, which the sum over the slabs would hide when two slabs err in opposite ways.  Every output is
pre-filled with NaN (or a marker word) and followed by guard slots that must keep it, and every input must come back byte for byte.

Bounds that are not == are the project's existing ones, cited where they are used, or derived in the docstring that uses them."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import objective_ref as R  # noqa: E402
import real_kernels_ref as K  # noqa: E402
from test_real_kernels_cpu import DIRECT_REDS, PLAIN_ONLY_PLANS, RING_PLANS  # noqa: E402

NAN = float("nan")
MARK = -1234567            # marker of the word outputs
GUARD = 64                 # slots behind every output
SUMS0 = (3.5, -1.25, 7.0, 9.0)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def as_torch(a):
    a = np.array(a, order="C")      # a copy: the shared host inputs are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)


def at(t, elems):
    """device pointer `elems` elements into tensor t"""
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


class Operands:
    """host arrays and their device copies, kept alive together; unchanged() compares every one byte for byte"""

    def __init__(self, **host):
        self.host = {k: np.ascontiguousarray(v) for k, v in host.items()}
        self.dev = {k: as_torch(v).cuda() for k, v in self.host.items()}

    def p(self, name):
        return C.c_void_p(self.dev[name].data_ptr())

    def unchanged(self):
        for k, v in self.host.items():
            assert self.dev[k].cpu().numpy().tobytes() == v.tobytes(), f"input {k} was written to"


def nan_out(n):
    return torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")


def word_out(n):
    return torch.full((n + GUARD,), MARK, dtype=torch.int32, device="cuda")


def body_and_guard(t, n):
    got = t.cpu().numpy()
    guard = got[n:]
    assert guard.size == GUARD and (np.isnan(guard).all() if got.dtype.kind == "f" else (guard == MARK).all()), "guard slots written"
    return got[:n]


# ------------------------------------------------------------------------------------------------------------------------------
# A. the re-ordering kernels, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("red,slack", [(64, 0), (320, 0), (320, 12)])
@pytest.mark.parametrize("rows_pad", [64, 192, 384])
def test_tile_f32_bit_for_bit(L, rows_pad, red, slack):
    """tile_f32_kernel on a position-coded matrix; with lda = red + 12 the slack holds NaN and none of it may arrive"""
    X = np.full((rows_pad, red + slack), np.nan, np.float32)
    X[:, :red] = K.position_coded(rows_pad, red)
    ops = Operands(X=X)
    out = nan_out(rows_pad * red)
    L.check(L.lib.bmf_tile_f32(ops.p("X"), rows_pad, red + slack, red, L.ptr(out), stream()))
    got = body_and_guard(out, rows_pad * red)
    assert got.tobytes() == K.tile_f32(X, red).tobytes()
    ops.unchanged()


def frag_calls(L, F, kp):
    """(name, call, words, expected) of every factor order that takes a rows_pad x kp factor"""
    rows_pad = F.shape[0]
    n = rows_pad * kp
    calls = [("bmf_frag_f32", lambda f, o: L.lib.bmf_frag_f32(f, rows_pad, kp, o, stream()), n, K.frag_f32(F), nan_out),
             ("bmf_frag_rows_f32", lambda f, o: L.lib.bmf_frag_rows_f32(f, rows_pad, kp, o, stream()), n, K.frag_rows_f32(F), nan_out)]
    if kp == 32:
        calls += [("bmf_frag_rows_bf16", lambda f, o: L.lib.bmf_frag_rows_bf16(f, rows_pad, kp, o, stream()), n, K.frag_rows_bf16(F), word_out),
                  ("bmf_frag_bf16x3", lambda f, o: L.lib.bmf_frag_bf16x3(f, rows_pad, o, stream()), rows_pad * 48, K.frag_bf16x3(F), word_out)]
    return calls


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("rows_pad", [64, 192, 384])
def test_factor_orders_bit_for_bit(L, rows_pad, kp):
    """frag_f32_kernel, frag_rows_f32_kernel, frag_rows_bf16_kernel and frag_bf16x3_kernel on position-coded factors (every element a
    distinct integer below 2^24: a misplaced element shows as itself), and the two bf16 orders on values at the edges of the
    rounding: expected hi = the round-to-nearest-even bf16, lo = the RNE bf16 of the fp32 remainder; the bf16 x 3 addends the
    truncations, hi + mid + lo == x exactly."""
    inputs = [K.position_coded(rows_pad, kp)]
    if kp == 32:
        inputs += [K.bf16_value_inputs(rows_pad, 0), -K.position_coded(rows_pad, kp)]
    for F in inputs:
        ops = Operands(F=F)
        for name, call, n, want, make in frag_calls(L, F, kp):
            out = make(n)
            L.check(call(ops.p("F"), L.ptr(out)))
            got = body_and_guard(out, n)
            bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
            assert bad.size == 0, (name, bad[:8].tolist(), got.view(np.uint32)[bad[:8]].tolist(), want.view(np.uint32)[bad[:8]].tolist())
        ops.unchanged()
    if kp == 32:      # the device's own three addends add up to the input
        F = inputs[1]
        ops = Operands(F=F)
        out = word_out(rows_pad * 48)
        L.check(L.lib.bmf_frag_bf16x3(ops.p("F"), rows_pad, L.ptr(out), stream()))
        halves = body_and_guard(out, rows_pad * 48).view(np.uint16)
        part, src = K.frag_bf16x3_src(rows_pad)
        total = np.zeros(rows_pad * 32)
        np.add.at(total, src, K.as_f32(halves).astype(np.float64))
        assert np.array_equal(total.reshape(rows_pad, 32), F.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------------
# B. the contractions, slab by slab
# ------------------------------------------------------------------------------------------------------------------------------
FORMS = ["plain", "tiled", "bf3", "resid", "resid_bf3"]
FUSED = ("resid", "resid_bf3")


def operands(form, c, kp):
    """the operands of one form from a case's A (rows_pad x red), F (red x kp) and, for the fused forms, G (rows_pad x 32)"""
    A, F = c["A"], c["F"]
    rows_pad, red = A.shape
    if form == "plain":      # lda = red + 12, ldft = red + 8, NaN in the parts that are not to be read
        Ap = np.full((rows_pad, red + 12), np.nan, np.float32)
        Ap[:, :red] = A
        FT = np.full((kp, red + 8), np.nan, np.float32)
        FT[:, :red] = F.T
        return Operands(A=Ap, FT=FT)
    host = dict(At=K.tile_f32(A, red))
    if form in ("tiled", "resid"):
        host["Ff"] = K.frag_f32(F)
    if form in ("bf3", "resid_bf3"):
        host["F3"] = K.frag_bf16x3(F)
    if form in FUSED:
        host["Frf"], host["G"] = K.frag_rows_bf16(F), c["G"]
    return Operands(**host)


def launch(L, form, ops, rows_pad, red, kp, out, stride, splits, sums=None):
    lib = L.lib
    if form == "plain":
        return lib.bmf_xf_f32(ops.p("A"), rows_pad, red + 12, red, ops.p("FT"), red + 8, kp, out, stride, splits, stream())
    if form == "tiled":
        return lib.bmf_xf_f32_tiled(ops.p("At"), rows_pad, red, ops.p("Ff"), kp, out, stride, splits, stream())
    if form == "bf3":
        return lib.bmf_xf_f32_tiled_bf3(ops.p("At"), rows_pad, red, ops.p("F3"), out, stride, splits, stream())
    if form == "resid":
        return lib.bmf_xf_f32_tiled_resid(ops.p("At"), rows_pad, red, ops.p("Ff"), ops.p("Frf"), ops.p("G"), kp, out, stride, splits, sums, stream())
    assert form == "resid_bf3"
    return lib.bmf_xf_f32_tiled_resid_bf3(ops.p("At"), rows_pad, red, ops.p("F3"), ops.p("Frf"), ops.p("G"), out, stride, splits, sums, stream())


def slabs_of(out, rows_pad, kp, splits, stride):
    """[splits][rows_pad][kp] of an output buffer; the gaps between the slabs and the guard behind the last must still hold NaN"""
    got = body_and_guard(out, splits * stride).reshape(splits, stride)
    assert np.isnan(got[:, rows_pad * kp:]).all(), "the gap between two slabs was written"
    return got[:, :rows_pad * kp].reshape(splits, rows_pad, kp)


def assert_slabs(got, want, what):
    bad = np.argwhere(~(got.astype(np.float64) == want))
    assert bad.size == 0, (what, [(s, r // 64, r, c, float(got[s, r, c]), float(want[s, r, c])) for s, r, c in bad[:6]], len(bad))


def sums_buffer():
    return torch.tensor(SUMS0 + (NAN,) * 4, dtype=torch.float64, device="cuda")


def assert_sums(sums, c, what):
    got = sums.cpu().numpy()
    assert got[:4].tolist() == [SUMS0[0] + c["s_abs"], SUMS0[1] + c["s_sq"], SUMS0[2], SUMS0[3]] and np.isnan(got[4:]).all(), (what, got.tolist(), c["s_abs"], c["s_sq"])


def ring_case(form, rows_pad, stages, k, kp):
    return K.residual_case(rows_pad, 64 * stages, k) if form in FUSED else K.contraction_case(rows_pad, 64 * stages, k, kp)


def run_ring_plan(L, form, rows_pad, stages, splits, k, kp):
    """one launch of one form on one (stages, splits) plan: every slab == its exact partial product, an empty range exactly zero; the
    fused forms: the sums start at SUMS0 and end at exactly that plus the exact pair.  Returns the slabs."""
    red = 64 * stages
    c = ring_case(form, rows_pad, stages, k, kp)
    ops = operands(form, c, kp)
    stride = rows_pad * kp + 32
    out, sums = nan_out(splits * stride), sums_buffer() if form in FUSED else None
    L.check(launch(L, form, ops, rows_pad, red, kp, L.ptr(out), stride, splits, L.ptr(sums)))
    got = slabs_of(out, rows_pad, kp, splits, stride)
    ranges = K.slab_ranges(stages, splits)
    what = (form, rows_pad, stages, splits, k, kp)
    assert_slabs(got, K.slab_products(c["A"], c["F"], ranges, 64), what)
    for s, (a, b) in enumerate(ranges):
        if a == b:
            assert not got[s].any(), (what, "empty slab", s)
    if form in FUSED:
        assert_sums(sums, c, what)
    ops.unchanged()
    return got


@pytest.mark.parametrize("rows_pad", [128, 384])
@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("form", ["plain", "tiled"])
def test_ring_contraction_slab_by_slab(L, form, kp, rows_pad):
    """xf_f32_ring_kernel<kp / 32> through bmf_xf_f32 (row-major A with lda = red + 12, FT with ldft = red + 8, NaN in the slack: red % 64 == 0
    and an aligned `out` take the ring kernel, which the stage-wise slabs confirm) and through bmf_xf_f32_tiled (tiled A, fragment
    order), 2 and 6 row tiles: 1 .. 7 and 9 stages in one split (the loop starts three stages early: every count below, at and above
    the three fragment sets and the four ring buffers), 3/3/2, 9/8, 6/6/6/5, one stage each, a zero-stage split, and (plain) more
    splits than stages.  k = kp - 5 and k = kp."""
    plans = RING_PLANS + (PLAIN_ONLY_PLANS if form == "plain" else [])
    for stages, splits in plans:
        for k in (kp - 5, kp):
            run_ring_plan(L, form, rows_pad, stages, splits, k, kp)


@pytest.mark.parametrize("rows_pad", [64, 192])
@pytest.mark.parametrize("form", ["bf3", "resid", "resid_bf3"])
def test_ring_contraction_slab_by_slab_kp32_forms(L, form, rows_pad):
    """xf_f32_bf3_ring_kernel, xf_f32_resid_ring_kernel<false> and <true> on 1 and 3 row tiles, the same plans.  The fused forms run on
    objective_ref.exact_real_case: the sums are counted once over all splits, the zero-stage split included, sums[2..3] untouched;
    `out` of the fused pass is bit for bit the result of the pass without the sums (bmf_xf_f32_tiled wants rows_pad % 128 == 0: it gets
    the same tiled A with one more, all-zero row tile)."""
    kp = 32
    for stages, splits in RING_PLANS:
        for k in (kp - 5, kp):
            got = run_ring_plan(L, form, rows_pad, stages, splits, k, kp)
            if form not in FUSED:
                continue
            red, stride = 64 * stages, (rows_pad + 64) * kp + 32
            c = ring_case(form, rows_pad, stages, k, kp)
            if form == "resid":
                ops = Operands(At=np.concatenate([K.tile_f32(c["A"], red), np.zeros(64 * red, np.float32)]), Ff=K.frag_f32(c["F"]))
                ref, rp = "tiled", rows_pad + 64
            else:
                ops, ref, rp, stride = operands("bf3", c, kp), "bf3", rows_pad, rows_pad * kp + 32
            out = nan_out(splits * stride)
            L.check(launch(L, ref, ops, rp, red, kp, L.ptr(out), stride, splits))
            plain = slabs_of(out, rp, kp, splits, stride)
            assert plain[:, :rows_pad].tobytes() == got.tobytes() and not plain[:, rows_pad:].any(), (form, rows_pad, stages, splits, k)


@pytest.mark.parametrize("rows_pad", [128, 384])
@pytest.mark.parametrize("kp", [32, 64])
def test_direct_contraction_slab_by_slab(L, kp, rows_pad):
    """xf_f32_kernel<kp / 32> (red % 64 != 0): 1, 3, 5, 9, 63 and 65 groups of 8 in 1, 2 and 3 slabs -- the four-at-a-time loop and every
    remainder -- with lda = red + 12, ldft = red + 8 and NaN in the slack; more splits than groups are refused and write nothing."""
    for red in DIRECT_REDS:
        assert red % 64 != 0
        for k in (kp - 5, kp):
            c = K.contraction_case(rows_pad, red, k, kp)
            ops = operands("plain", c, kp)
            stride = rows_pad * kp + 32
            for splits in (1, 2, 3):
                out = nan_out(splits * stride)
                rc = launch(L, "plain", ops, rows_pad, red, kp, L.ptr(out), stride, splits)
                if splits > red // 8:
                    assert rc != 0 and np.isnan(body_and_guard(out, splits * stride)).all()
                    continue
                L.check(rc)
                got = slabs_of(out, rows_pad, kp, splits, stride)
                assert_slabs(got, K.slab_products(c["A"], c["F"], K.slab_ranges(red // 8, splits), 8), ("direct", rows_pad, red, splits, k, kp))
            ops.unchanged()


@pytest.mark.parametrize("kp", [32, 64])
def test_unaligned_out_falls_back_to_the_direct_kernel(L, kp):
    """red = 192 in 5 slabs: the ring kernel splits 3 stages 1 / 1 / 1 / 0 / 0, the direct kernel 24 groups 5 / 5 / 5 / 5 / 4.  With `out`
    16-byte aligned the slabs are the former, with `out` shifted by 4 bytes the latter: the launcher fell back, and the numbers are
    the exact ones either way."""
    rows_pad, red, splits, k = 128, 192, 5, kp - 5
    c = K.contraction_case(rows_pad, red, k, kp)
    ops = operands("plain", c, kp)
    stride = rows_pad * kp + 32
    for shift, units, unit in ((0, 3, 64), (1, 24, 8)):
        out = nan_out(splits * stride + 4)
        L.check(launch(L, "plain", ops, rows_pad, red, kp, at(out, shift), stride, splits))
        got = out.cpu().numpy()
        assert np.isnan(got[:shift]).all() and np.isnan(got[shift + splits * stride:]).all()
        got = got[shift:shift + splits * stride].reshape(splits, stride)
        assert np.isnan(got[:, rows_pad * kp:]).all()
        assert_slabs(got[:, :rows_pad * kp].reshape(splits, rows_pad, kp), K.slab_products(c["A"], c["F"], K.slab_ranges(units, splits), unit), (shift, kp))
    ops.unchanged()


@pytest.mark.parametrize("kp", [32, 64])
def test_tiled_contraction_refuses_an_odd_tile_count(L, kp):
    """bmf_xf_f32_tiled shares bmf_xf_f32's argument check, rows_pad % 128 == 0, although the ring kernel tiles by 64 (include/bmf_hip.h says
    so): rows_pad = 192 is refused and nothing is written."""
    rows_pad, red = 192, 128
    c = K.contraction_case(rows_pad, red, kp - 5, kp)
    ops = operands("tiled", c, kp)
    out = nan_out(rows_pad * kp)
    assert launch(L, "tiled", ops, rows_pad, red, kp, L.ptr(out), rows_pad * kp, 1) != 0
    assert b"128" in L.lib.bmf_last_error()
    assert np.isnan(body_and_guard(out, rows_pad * kp)).all()
    ops.unchanged()


# ------------------------------------------------------------------------------------------------------------------------------
# C. single-cell and cross-term probes of the fused residual
# ------------------------------------------------------------------------------------------------------------------------------
def probe_delta(p):
    """a multiple of 1/8 in [-64, 64] that differs from probe to probe and is never 0"""
    d = ((37 * p) % 1023 - 511) / 8.0
    return d if d != 0 else 64.0


@pytest.mark.parametrize("form", FUSED)
@pytest.mark.parametrize("stages,splits", [(23, 4), (5, 4)])
def test_single_cell_probes_fused_residual(L, form, stages, splits):
    """X = G F^T exactly (objective_ref's exact factors: every cell a multiple of 2^-6 below 4) but for ONE cell that is off by d, a
    multiple of 1/8 with |d| <= 64: the accumulator of that cell runs through multiples of 2^-6 below 128 and ends at -d exactly, every
    other cell at 0, so sums == (|d|, d d).  Probes: all 64 row positions of a tile at two reduction positions and all 64 reduction
    positions of a stage at two rows (the 6/6/6/5 plan), the first and the last stage of every split (both plans; the 2/2/1/0 plan has a
    zero-stage split), the last real row and the last real reduction index."""
    rows_pad, red, kp = 192, 64 * stages, 32
    c = K.residual_case(rows_pad, red, 27)
    P = (c["G"].astype(np.float64) @ c["F"].astype(np.float64).T).astype(np.float32)
    assert np.array_equal(P.astype(np.float64), c["G"].astype(np.float64) @ c["F"].astype(np.float64).T)
    ops = operands(form, dict(A=P, F=c["F"], G=c["G"]), kp)
    inv = K.inverse(K.tile_src(rows_pad, red, red))
    cells = []
    if stages == 23:
        cells += [(64 + i, j) for i in range(64) for j in (5, 64 * 22 + 37)] + [(i, 64 * 7 + j) for j in range(64) for i in (3, 150)]
    for a, b in K.slab_ranges(stages, splits):
        if a < b:
            cells += [(70, 64 * a + 9), (70, 64 * (b - 1) + 54), (131, 64 * a + 40), (131, 64 * (b - 1) + 23)]
    cells += [(c["rows"] - 1, 17), (17, c["real"] - 1), (c["rows"] - 1, c["real"] - 1)]
    stride = rows_pad * kp
    out = nan_out(splits * stride)
    sums = torch.zeros(4 * len(cells) + 4, dtype=torch.float64, device="cuda")
    At = ops.dev["At"]
    want = np.zeros((len(cells) + 1, 4))
    for p, (i, j) in enumerate(cells):
        d = probe_delta(p)
        pos = int(inv[i * red + j])
        At[pos] = float(P[i, j]) + d
        L.check(launch(L, form, ops, rows_pad, red, kp, L.ptr(out), stride, splits, at(sums, 4 * p)))
        At[pos] = float(P[i, j])
        want[p, :2] = abs(d), d * d
    got = sums.cpu().numpy().reshape(-1, 4)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(cells[p], probe_delta(p), got[p].tolist()) for p in bad[:8]]
    ops.unchanged()          # every probed cell was put back


@pytest.mark.parametrize("form", FUSED)
def test_cross_terms_of_the_fused_residual(L, form):
    """The residual product keeps hi hi + hi lo + lo hi of the two-addend bf16 split.  X = 0; one factor one-hot with value 1.0 (hi = 1,
    lo = 0), the other a single value f of 16 significant bits (hi and lo both non-zero, hi + lo == f): the cell's product is
    f_hi + f_lo = f exactly, so s_abs == f and s_sq == float32(f f) (one fma of the fp32 residual), and with either cross term
    dropped it is f_hi alone.  f on the streamed factor's side (its lo part comes from bmf_frag_rows_bf16) and on the row factor's
    side (split in the kernel)."""
    rows_pad, stages, splits, kp = 192, 9, 2, 32
    red = 64 * stages
    f = np.float32(1.0 + 2.0 ** -7 + 2.0 ** -9 + 2.0 ** -15)
    want = [float(f), float(np.float32(np.float64(f) * np.float64(f))), 0.0, 0.0]
    out = nan_out(splits * rows_pad * kp)
    for side in ("F", "G"):
        for i, j, l in ((0, 3, 0), (37, 64 * 7 + 45, 17), (100, 64 * 8 + 63, 31), (191, 64 * 4 + 32, 8)):
            F, G = np.zeros((red, kp), np.float32), np.zeros((rows_pad, kp), np.float32)
            F[j, l], G[i, l] = (f, 1.0) if side == "F" else (1.0, f)
            ops = operands(form, dict(A=np.zeros((rows_pad, red), np.float32), F=F, G=G), kp)
            sums = torch.zeros(4, dtype=torch.float64, device="cuda")
            L.check(launch(L, form, ops, rows_pad, red, kp, L.ptr(out), rows_pad * kp, splits, L.ptr(sums)))
            assert sums.cpu().numpy().tolist() == want, (side, i, j, l, sums.cpu().numpy().tolist(), want)
            assert not slabs_of(out, rows_pad, kp, splits, rows_pad * kp).any()          # A = 0: the contraction is 0


# ------------------------------------------------------------------------------------------------------------------------------
# D. precision on general data
# ------------------------------------------------------------------------------------------------------------------------------
def test_general_data_per_element(L):
    """Non-negative random fp32 A and F, as WNMF's are, 23 stages in 4 splits; the bounds of test_tiled_real_matrix_kernels applied
    per element instead of in norm: |got - fp64| <= 3e-6 (|A| @ |F|) for every element of every form, the bf16 x 3 forms no worse than
    2 e_fp32 + 2e-7 (e = the largest relative error; e_fp32 from the exact-fp32 contraction of the fused pass at the same shape), the
    fused sums within 1e-6.  test_real_kernels_cpu shows that no product of the six can be lost inside the first bound."""
    stages, splits = 23, 4
    red = 64 * stages
    e = {}
    for form, kp, rows_pad in [("plain", 32, 384), ("plain", 64, 384), ("tiled", 32, 384), ("tiled", 64, 384), ("resid", 32, 192), ("bf3", 32, 192),
                               ("resid_bf3", 32, 192)]:
        c = K.general_case(rows_pad, red, kp - 5, kp)
        A64, F64, G64 = (c[x].astype(np.float64) for x in "AFG")
        ops = operands(form, c, kp)
        stride = rows_pad * kp + 32
        out, sums = nan_out(splits * stride), sums_buffer() if form in FUSED else None
        L.check(launch(L, form, ops, rows_pad, red, kp, L.ptr(out), stride, splits, L.ptr(sums)))
        got = slabs_of(out, rows_pad, kp, splits, stride).astype(np.float64).sum(0)
        exact, scale = A64 @ F64, np.abs(A64) @ np.abs(F64)
        err = np.abs(got - exact)
        print(form, kp, "largest |got - fp64| / (|A| @ |F|):", float((err / (scale + 1e-300)).max()))
        assert (err <= 3e-6 * scale).all(), (form, kp, float((err / (scale + 1e-300)).max()))
        assert not got[c["rows"]:].any() and not got[:, kp - 5:].any()
        e[form] = float((err / (scale + 1e-300)).max())
        if form in FUSED:
            r = A64 - G64 @ F64.T
            s = sums.cpu().numpy()
            rel = (abs(s[0] - SUMS0[0] - np.abs(r).sum()) / np.abs(r).sum(), abs(s[1] - SUMS0[1] - (r * r).sum()) / (r * r).sum())
            print(form, "relative error of the sums:", rel)
            assert rel[0] <= 1e-6 and rel[1] <= 1e-6 and s[2:4].tolist() == list(SUMS0[2:]), (form, rel)
        ops.unchanged()
    assert e["bf3"] <= 2 * e["resid"] + 2e-7 and e["resid_bf3"] <= 2 * e["resid"] + 2e-7, e


# ------------------------------------------------------------------------------------------------------------------------------
# E. launch after launch
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kp", [("tiled", 32), ("tiled", 64), ("bf3", 32), ("resid", 32), ("resid_bf3", 32)])
def test_exact_launch_after_launch(L, form, kp):
    """The fragment registers of the ring kernels are written by hand-placed loads behind counted waits; a copy the compiler moves ahead
    of such a wait shows only now and then and only under load (the mae32 incident of HISTORY.md: 4 launches in 100).  A 2048 x 4096
    (32 MB, 1024 workgroups over 8 splits of 8 stages), twenty launches of each form, every slab and the sums exact each time."""
    rows_pad, stages, splits, k = 2048, 64, 8, kp - 5
    red = 64 * stages
    c = ring_case(form, rows_pad, stages, k, kp)
    ops = operands(form, c, kp)
    n, stride = rows_pad * kp, rows_pad * kp + 32
    want = K.slab_products(c["A"], c["F"], K.slab_ranges(stages, splits), 64)
    want_d = torch.from_numpy(want.astype(np.float32)).cuda()
    assert np.array_equal(want_d.cpu().numpy().astype(np.float64), want)
    out = nan_out(splits * stride)
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    for rep in range(20):
        out.fill_(NAN)
        sums.zero_()
        L.check(launch(L, form, ops, rows_pad, red, kp, L.ptr(out), stride, splits, L.ptr(sums)))
        if not torch.equal(out[:splits * stride].view(splits, stride)[:, :n].reshape(splits, rows_pad, kp), want_d):
            assert_slabs(slabs_of(out, rows_pad, kp, splits, stride), want, ("launch", rep, form, kp))      # names slab, tile, row, column
        if form in FUSED:
            assert sums.cpu().numpy().tolist() == [c["s_abs"], c["s_sq"], 0.0, 0.0], ("launch", rep, sums.cpu().numpy().tolist(), c["s_abs"], c["s_sq"])
    slabs_of(out, rows_pad, kp, splits, stride)       # gaps and guard
    ops.unchanged()


# ------------------------------------------------------------------------------------------------------------------------------
# F. the fused update (real_update_kernel) and the C loop (bmf_wnmf_real_prepare / bmf_wnmf_real_run) on a hand-made state
# ------------------------------------------------------------------------------------------------------------------------------
from test_mu_epilogue_cpu import WNMF, mu_step_ref  # noqa: E402

M, N, M_PAD, N_PAD = 300, 600, 384, 640
LOG_ROWS = 8
# (k, kp, splits_xv, splits_xtu, gram_blocks, Urf, UT3 / VT3): every slab count of the update's loop (four at a time plus a remainder of
# 0 .. 3), a block that walks 1, 2 .. 3 and all 3 / 5 row groups, the residual sums fused into X^T U or in a pass of their own, the
# contractions on the exact-fp32 or the bf16 x 3 instruction; and one kp = 64 state, which takes the shared epilogue and the
# stand-alone re-order and Gram launches instead of the fused update
STATE_CASES = [(27, 32, 1, 1, 1024, True, False), (27, 32, 3, 4, 2, True, True), (32, 32, 4, 5, 1, False, True), (1, 32, 5, 6, 1024, False, False),
               (32, 32, 9, 4, 2, True, False), (1, 32, 4, 5, 1, True, True), (27, 32, 9, 6, 1, False, False), (27, 32, 5, 1, 2, False, True),
               (40, 64, 3, 4, 8, False, False)]


def state_id(c):
    return "k%d-kp%d-xv%d-xtu%d-gb%d%s%s" % (c[:5] + ("-urf" if c[5] else "", "-bf3" if c[6] else ""))


class RealState:
    """A bmf_wnmf_real_state whose every buffer the test owns: outputs pre-filled with NaN (words: MARK) and followed by GUARD slots,
    finite junk in the padding of the fp64 masters, the inputs kept on the host for the byte comparison."""

    def __init__(self, L, X, U0, V0, case, with_mae=1):
        k, kp, sxv, sxtu, gb, urf, t3 = case
        self.L, self.case, self.k, self.kp, self.fused = L, case, k, kp, kp == 32
        rs = np.random.RandomState(77)
        Xp = np.zeros((M_PAD, N_PAD), np.float32)
        Xp[:M, :N] = X
        self.Xp = Xp
        XT = np.ascontiguousarray(Xp.T)
        U64, V64 = rs.rand(M_PAD, kp) * 5 + 1, rs.rand(N_PAD, kp) * 5 + 1          # junk wherever the factor is not
        U64[:M, :k], V64[:N, :k] = U0, V0
        self.inputs = Operands(X=Xp, XT=XT, Xtiled=K.tile_f32(Xp, N_PAD), XTtiled=K.tile_f32(XT, M_PAD))
        self.t = {}
        f32, f64 = torch.float32, torch.float64
        # (the fused update leaves one Gram slab per workgroup, at most one per 128 rows: 5; bmf_gram_partial leaves gram_blocks)
        for name, n in (("U", M_PAD * kp), ("V", N_PAD * kp), ("UT", M_PAD * kp), ("VT", N_PAD * kp), ("Vrf", N_PAD * kp), ("GU", kp * kp),
                        ("GV", kp * kp), ("Mslab", sxv * M_PAD * kp), ("Nslab", sxtu * N_PAD * kp), ("gram_slabs", (5 if self.fused else gb) * kp * kp)):
            self.buf(name, n, f32)
        for name, n in (("GU64", kp * kp), ("GV64", kp * kp), ("partU", M_PAD // 128 * 2), ("partV", N_PAD // 128 * 2), ("sums", 4), ("scal", 8),
                        ("log", LOG_ROWS * L.LOG_COLS)):
            self.buf(name, n, f64)
        for name, n in (("Urf", M_PAD * kp), ("UT3", M_PAD * 48), ("VT3", N_PAD * 48), ("colbits", kp * (N_PAD // 32))):
            self.buf(name, n, torch.int32)
        self.buf("rowbits", N_PAD, torch.int64)
        self.t["U64"], self.t["V64"] = torch.from_numpy(U64).cuda(), torch.from_numpy(V64).cuda()
        self.t["stop"] = torch.zeros(1 + GUARD, dtype=torch.int32, device="cuda")
        st = self.st = L.WnmfRealState()
        st.struct_bytes = C.sizeof(L.WnmfRealState)
        st.m, st.n, st.k, st.kp, st.with_mae, st.m_pad, st.n_pad = M, N, k, kp, with_mae, M_PAD, N_PAD
        for name in ("X", "XT", "Xtiled", "XTtiled"):
            setattr(st, name, self.inputs.dev[name].data_ptr())
        names = ["U64", "V64", "U", "V", "UT", "VT", "Mslab", "Nslab", "gram_slabs", "GU", "GV", "GU64", "GV64", "partU", "partV", "rowbits", "colbits",
                 "sums", "scal", "log", "stop", "Vrf"] + (["Urf"] if urf else []) + (["UT3", "VT3"] if t3 else [])
        for name in names:
            setattr(st, name, self.t[name].data_ptr())
        st.splits_xv, st.splits_xtu, st.gram_blocks, st.ldcb, st.log_rows = sxv, sxtu, gb, N_PAD // 32, LOG_ROWS
        st.sum_x2, st.cells, st.tol, st.min_diff = float((Xp.astype(np.float64) ** 2).sum()), float(M) * float(N), 0.0, 0.0
        self.given = set(names)

    def buf(self, name, n, dtype):
        self.t[name] = torch.full((n + GUARD,), NAN if dtype.is_floating_point else MARK, dtype=dtype, device="cuda")

    def prepare(self):
        self.L.check(self.L.lib.bmf_wnmf_real_prepare(C.byref(self.st), stream()))

    def run(self, it0, it1, max_iter):
        self.L.check(self.L.lib.bmf_wnmf_real_run(C.byref(self.st), it0, it1, max_iter, stream()))

    def get(self, name, shape=None):
        """the body of a buffer (the guard behind it checked); buffers that were not handed to the library must be untouched"""
        a = self.t[name].cpu().numpy()
        if name in ("U64", "V64"):
            return a
        body, guard = a[:-GUARD], a[-GUARD:]
        mark = (lambda v: np.isnan(v).all()) if a.dtype.kind == "f" else (lambda v: (v == (0 if name == "stop" else MARK)).all())
        assert mark(guard), f"guard of {name} written"
        if name not in self.given:
            assert mark(body), f"{name} was not part of the state and was written"
        return body if shape is None else body.reshape(shape)

    def snapshot(self):
        torch.cuda.synchronize()
        return {name: t.cpu().numpy().tobytes() for name, t in self.t.items()}


def standalone_orders(L, F32, kp):
    """the stand-alone kernels of part A on the device's own fp32 factor: frag, rows_bf16, bf16x3 (words), rows_f32"""
    rows_pad = F32.shape[0]
    ops = Operands(F=F32)
    out = {}
    for name, call, n, _, make in frag_calls(L, F32, kp):
        o = make(n)
        L.check(call(ops.p("F"), L.ptr(o)))
        out[name] = body_and_guard(o, n)
    return out


def assert_derived(L, s, side):
    """every output the update derives from the new factor, bit for bit from the device's own F64: the fp32 shadow (zeros in the
    padding), the fragment order, and where the state has them the bf16 row order (U only) and the bf16 x 3 order"""
    rows_pad, rows = (M_PAD, M) if side == "U" else (N_PAD, N)
    kp, k = s.kp, s.k
    F64 = s.get(side + "64").reshape(rows_pad, kp)
    ok = (np.arange(rows_pad)[:, None] < rows) & (np.arange(kp)[None, :] < k)
    F = s.get(side, (rows_pad, kp))
    assert F.tobytes() == np.where(ok, F64, 0.0).astype(np.float32).tobytes(), side
    orders = standalone_orders(L, F, kp)
    assert s.get(side + "T").tobytes() == orders["bmf_frag_f32"].tobytes() == K.frag_f32(F).tobytes(), side + "T"
    if kp == 32:
        if side == "U":
            urf = s.get("Urf")
            assert "Urf" not in s.given or urf.tobytes() == orders["bmf_frag_rows_bf16"].tobytes(), "Urf"
        t3 = s.get(side + "T3")
        assert side + "T3" not in s.given or t3.tobytes() == orders["bmf_frag_bf16x3"].tobytes(), side + "T3"
    return F64, F, ok


def gram_check(s, name, F):
    """test_gram's bound: 2e-6 of the entry and of the largest entry; the fp64 copy exactly symmetric"""
    kp = s.kp
    want = F.astype(np.float64).T @ F.astype(np.float64)
    g64, g32 = s.get(name + "64", (kp, kp)), s.get(name, (kp, kp))
    np.testing.assert_allclose(g64, want, rtol=2e-6, atol=2e-6 * np.abs(want).max())
    np.testing.assert_allclose(g32, want, rtol=2e-6, atol=2e-6 * np.abs(want).max())
    assert np.array_equal(g64, g64.T)


@pytest.mark.parametrize("case", STATE_CASES, ids=state_id)
def test_prepare_on_exact_inputs(L, case):
    """bmf_wnmf_real_prepare on objective_ref.exact_real_case: everything it leaves, output by output.  Exact, hence ==: the slabs of
    X V and X^T U (slab s = its own stages), the residual sums (fused into X^T U or from the pass of their own), <U, X V> per group of 128 rows
    (products of multiples of 1/8 and 2^-6 summed in fp64), and the error of log row 0, whose trace form 1/2 (sum X^2 - 2 <U, X V> +
    <U^T U, V^T V>) is then exactly half the sum of squares.  RMSE and MAE follow by one division (and one square root): 4 ulp."""
    k, kp, sxv, sxtu, gb, urf, t3 = case
    c = R.exact_real_case(M, N, k)
    s = RealState(L, R.real_x(M, N), c["U"], c["V"], case)
    masters = s.t["U64"].cpu().numpy().copy(), s.t["V64"].cpu().numpy().copy()
    s.prepare()
    torch.cuda.synchronize()
    U64, U, okU = assert_derived(L, s, "U")
    V64, V, okV = assert_derived(L, s, "V")
    # PREPARE mode does not write the masters (fused update and shared epilogue alike): the junk of their padding is still there
    assert U64.tobytes() == masters[0].tobytes() and V64.tobytes() == masters[1].tobytes()
    assert np.array_equal(U[:M, :k].astype(np.float64), c["U"]) and np.array_equal(V[:N, :k].astype(np.float64), c["V"])
    Ms, Ns = s.get("Mslab", (sxv, M_PAD, kp)), s.get("Nslab", (sxtu, N_PAD, kp))
    assert_slabs(Ms, K.slab_products(s.Xp, V, K.slab_ranges(N_PAD // 64, sxv), 64), "Mslab")
    assert_slabs(Ns, K.slab_products(s.Xp.T, U, K.slab_ranges(M_PAD // 64, sxtu), 64), "Nslab")
    assert s.get("sums").tolist() == [c["s_abs"], c["s_sq"], 0.0, 0.0], (s.get("sums").tolist(), c["s_abs"], c["s_sq"])
    gram_check(s, "GU", U)
    gram_check(s, "GV", V)
    partU, partV = s.get("partU", (M_PAD // 128, 2)), s.get("partV", (N_PAD // 128, 2))
    want_dot = (U.astype(np.float64) * (s.Xp.astype(np.float64) @ V.astype(np.float64))).reshape(M_PAD // 128, -1).sum(1)
    assert partU[:, 1].tolist() == want_dot.tolist()
    if s.fused:
        assert not partU[:, 0].any() and not partV[:, 0].any()
        used = min(N_PAD // 128, gb) * kp * kp           # the V side uses the most Gram slabs; the rest of the buffer is never written
        assert np.isnan(s.get("gram_slabs")[used:]).all()
    if not urf or not s.fused:
        assert s.get("Vrf").tobytes() == K.frag_rows_f32(V).tobytes()
    log = s.get("log", (LOG_ROWS, L.LOG_COLS))
    row = log[0]
    assert row[L.LOG_ITER] == 0 and row[L.LOG_ERROR] == row[L.LOG_REC] == 0.5 * c["s_sq"] and row[L.LOG_VALID] == 1 and row[L.LOG_STOP] == 0
    assert row[L.LOG_RMSE] == pytest.approx(np.sqrt(c["s_sq"] / (M * N)), rel=4 * 2.0 ** -52, abs=0)
    assert row[L.LOG_MAE] == pytest.approx(c["s_abs"] / (M * N), rel=4 * 2.0 ** -52, abs=0)
    assert np.isnan(log[1:]).all() and s.get("scal")[1] == 0.5 * c["s_sq"] and np.isnan(np.delete(s.get("scal"), 1)).all()
    assert s.get("stop")[0] == 0
    s.inputs.unchanged()


def positive_factors(k):
    """positive random factors with one all-zero row of V0 and (k > 1) one all-zero column of U0: den == 0 there, the clamp"""
    rs = np.random.RandomState(900 + k)
    U0, V0 = rs.rand(M, k) * 1.1 + 0.05, rs.rand(N, k) * 1.1 + 0.05
    V0[7] = 0.0
    if k > 1:
        U0[:, min(3, k - 1)] = 0.0
    X = rs.rand(M, N).astype(np.float32)
    return X, U0, V0


def in_enclosure(new, r, what):
    ok = r["ok"]
    bad = np.argwhere(ok & ((new < r["lo"] - r["tol"]) | (new > r["hi"] + r["tol"]) | ~np.isfinite(new)))
    assert bad.size == 0, (what, [(i, j, new[i, j], r["lo"][i, j], r["hi"][i, j]) for i, j in bad[:6]], len(bad))
    assert not new[~ok].any(), what


@pytest.mark.parametrize("case", STATE_CASES, ids=state_id)
def test_one_iteration_on_positive_factors(L, case):
    """bmf_wnmf_real_run(1, 2): the new V64 lies inside the enclosure of test_mu_epilogue_cpu.mu_step_ref (WNMF mode) computed from the
    device's own operands as they stood before the call (V64, V, the slabs of X^T U, U^T U), the new U64 inside the one from (U64, U, the
    slabs of X V left in the buffer, the new V^T V); every derived output is again bit for bit from the device's own masters; the planted zero row
    and zero column stay exactly 0 through the den = 0 clamp, and everything is finite."""
    k, kp, sxv, sxtu, gb, urf, t3 = case
    X, U0, V0 = positive_factors(k)
    s = RealState(L, X, U0, V0, case)
    s.prepare()
    torch.cuda.synchronize()
    before = {n: s.get(n).copy() for n in ("U", "V", "Nslab", "GU")}
    before["U64"], before["V64"] = s.get("U64").copy(), s.get("V64").copy()      # (junk in the padding where the fused update prepared them)
    s.run(1, 2, 100)
    torch.cuda.synchronize()
    U64, U, okU = assert_derived(L, s, "U")
    V64, V, okV = assert_derived(L, s, "V")
    common = dict(k=k, kp=kp, slab_stride=0, num_block_stride=0, den=None, reg=0.0, mode=WNMF, thr=0.5, plane_scale=None)
    rv = mu_step_ref(dict(common, F64=before["V64"], F=before["V"].reshape(N_PAD, kp), rows_pad=N_PAD, rows=N, splits=sxtu,
                          num=before["Nslab"].reshape(sxtu, N_PAD * kp), G=before["GU"].reshape(kp, kp)))
    in_enclosure(V64, rv, "V")
    ru = mu_step_ref(dict(common, F64=before["U64"], F=before["U"].reshape(M_PAD, kp), rows_pad=M_PAD, rows=M, splits=sxv,
                          num=s.get("Mslab", (sxv, M_PAD * kp)), G=s.get("GV", (kp, kp))))
    in_enclosure(U64, ru, "U")
    live = np.ones(k, bool)
    if k > 1:
        z = min(3, k - 1)
        live[z] = False
        assert not U64[:, z].any() and not V64[:, z].any()
    assert not V64[7].any() and (np.delete(V64[:N, :k], 7, axis=0)[:, live] > 0).all() and (U64[:M, :k][:, live] > 0).all()
    gram_check(s, "GU", U)
    gram_check(s, "GV", V)
    for name in ("Mslab", "Nslab", "GU", "GV", "GU64", "GV64", "partU", "sums"):
        assert np.isfinite(s.get(name)).all(), name
    log = s.get("log", (LOG_ROWS, L.LOG_COLS))
    cols = [L.LOG_ITER, L.LOG_ERROR, L.LOG_REC, L.LOG_RMSE, L.LOG_MAE, L.LOG_VALID, L.LOG_STOP]
    assert np.isfinite(log[:2, cols]).all() and log[1, L.LOG_ITER] == 1 and log[1, L.LOG_ERROR] < log[0, L.LOG_ERROR] and np.isnan(log[2:]).all()
    # the residual sums of the new factors: 1e-6, the bound of test_tiled_real_matrix_kernels, against fp64 on the device's own shadows
    r = s.Xp.astype(np.float64) - U.astype(np.float64) @ V.astype(np.float64).T
    np.testing.assert_allclose(s.get("sums")[:2], [np.abs(r).sum(), (r * r).sum()], rtol=1e-6)
    s.inputs.unchanged()


@pytest.mark.parametrize("case", [STATE_CASES[1], STATE_CASES[6], STATE_CASES[8]], ids=state_id)
def test_stop_flag_turns_the_loop_into_a_no_op(L, case):
    """With *stop = 1, bmf_wnmf_real_run(2, 3) leaves every buffer byte for byte, the log included.  With max_iter = 2 the stopping rule
    trips at iteration 3, and bmf_wnmf_real_run(1, 6) ends in the bytes of bmf_wnmf_real_run(1, 4): checked on one state by enqueuing
    (4, 6) behind (1, 4) -- the C loop enqueues iteration after iteration, so the two calls are the launches of (1, 6) -- because the
    residual sums of general data are added by atomics in an order that differs from run to run in the last bit; and on two states
    without the MAE pass, where every output is deterministic, with (1, 6) in one call against (1, 4).
    (Found here: the fused update reduced its Gram slabs behind a raised flag as well, from a buffer that then held the other side's slabs
    -- GV and GV64 changed.  HISTORY.md.)"""
    k = case[0]
    X, U0, V0 = positive_factors(k)
    s = RealState(L, X, U0, V0, case)
    s.prepare()
    s.run(1, 2, 100)
    s.t["stop"][0] = 1
    snap = s.snapshot()
    s.run(2, 3, 100)
    after = s.snapshot()
    assert [n for n in snap if snap[n] != after[n]] == []
    s.t["stop"][0] = 0
    s.run(2, 4, 2)
    snap = s.snapshot()
    assert s.get("stop")[0] == 3 and s.get("log", (LOG_ROWS, L.LOG_COLS))[3, L.LOG_STOP] == 1
    s.run(4, 6, 2)
    after = s.snapshot()
    assert [n for n in snap if snap[n] != after[n]] == []
    assert np.isnan(s.get("log", (LOG_ROWS, L.LOG_COLS))[4:]).all()
    two = []
    for last in (4, 6):
        d = RealState(L, X, U0, V0, case, with_mae=0)
        d.prepare()
        d.run(1, last, 2)
        two.append(d.snapshot())
        assert d.get("stop")[0] == 3
    assert [n for n in two[0] if two[0][n] != two[1][n]] == []
    s.inputs.unchanged()
