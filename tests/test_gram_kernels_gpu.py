"""The three exact-fp32 MFMA kernels behind every Gram matrix and every re-associated denominator, by direct C ABI calls, slab by slab
and bit for bit against the restatements of tests/gram_ref.py (proved on the host by tests/test_gram_kernels_cpu.py):

  gram_partial_kernel<1> (kp = 32), <2> (kp = 64)   bmf_gram_partial, bmf_gram_partial_i8    csrc/util.hip
  gram_cross_kernel                                  bmf_gram_cross                           csrc/wide.hip
  fg_f32_kernel                                      bmf_fg_f32                               csrc/wide.hip

Which path each case of R.GRAM_CASES reaches is in its name and is asserted from the launch arithmetic by the CPU file: the tail loop
alone, 1 / 2 / 4 / 11 trips of the 4-pair loop followed by 0 .. 3 tail pairs, a clipped last wave, idle waves in a busy block, 48 and
960 idle blocks; each at both instantiations and at ldf = kp and kp + 32.

Every call: outputs pre-filled with NaN and followed by guard slots that must keep their NaN; NaN in every input column the kernel must
not read; every input back byte for byte; a second launch into a fresh buffer gives the same bytes.

Gates.  Exact inputs (integers times a power of two per column; every partial sum representable, so the order cannot matter): the slab
equals the integer partial Gram of ITS OWN rows on bit patterns -- tracer columns name the slab that owns a row -- and an idle slab is
all +0.0.  Mixed inputs (columns nine decades apart): equal to the fmaf chain as int32.  Both: the bound of gram_ref.py against fp64,
so that a failure of the bitwise gate tells another order from other numbers.  No entry is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gram_ref as R  # noqa: E402

F32 = np.float32
GUARD = 64
KINDS = ["exact", "mixed"]
GRAM_IDS = [c[0] for c in R.GRAM_CASES]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()        # a copy: the shared host inputs are read-only


def raw(t):
    return t.cpu().numpy().tobytes()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def nan_buffer(n, head=None):
    """n output floats and GUARD guard slots, all NaN; `head` (the old `out` of an accumulating call) replaces the first n"""
    t = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    if head is not None:
        t[:n] = dev(head).reshape(-1)
    return t


def launch_twice(call, n, inputs, head=None):
    """call(out) into two fresh buffers; the guards keep their NaN, the inputs their bytes, both launches agree; returns the n floats"""
    before = [raw(t) for t in inputs]
    got = []
    for _ in range(2):
        out = nan_buffer(n, head)
        call(out)
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    assert (got[0][n:].view(np.int32) == R.NAN_BITS).all(), "a guard slot was written"
    assert got[0].tobytes() == got[1].tobytes(), "two identical launches differ"
    assert [raw(t) for t in inputs] == before, "an input was written"
    return got[0][:n]


def differing(got, want):
    """where two float32 arrays differ as bit patterns, for the assertion message"""
    idx = np.argwhere(bits(got) != bits(want))
    return len(idx), [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:6]]


def check_slabs(S, want, ref64, mag, rows_pad, blocks, tracers, symmetric):
    """the gates of one slab array S[blocks][kp][kp]"""
    nb = len(ref64)
    assert not np.isnan(S).any(), ("unwritten or poisoned entries", int(np.isnan(S).sum()))
    assert not bits(S[nb:]).any(), "an idle slab is not all +0.0"
    for c, r in tracers:                                           # which rows a slab owns
        assert np.flatnonzero(S[:, c, c]).tolist() == [R.owner_block(r, rows_pad, blocks)], (c, r)
    if symmetric:
        assert S.tobytes() == np.ascontiguousarray(S.transpose(0, 2, 1)).tobytes(), "a slab is not its own transpose"
    err = np.abs(S[:nb].astype(np.float64) - ref64)
    within = (err <= R.bound(R.slab_roundings(rows_pad, blocks), rows_pad, mag)).all()
    same = np.array_equal(bits(S), bits(want))
    assert within, ("other numbers: outside the rounding bound", float((err / np.maximum(mag, 1e-300)).max()), differing(S, want))
    assert same, ("inside the bound but not the restated bits: another order", differing(S, want))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. bmf_gram_partial
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_ld", [0, 32], ids=["ldf_kp", "ldf_kp_plus_32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kp", [32, 64], ids=["gram_partial_kernel_1_kp32", "gram_partial_kernel_2_kp64"])
@pytest.mark.parametrize("name,rows_pad,blocks", R.GRAM_CASES, ids=GRAM_IDS)
def test_gram_partial_slab_by_slab(L, name, rows_pad, blocks, kp, kind, wide_ld):
    F, want, ref64, mag, tracers = R.gram_reference(kind, rows_pad, blocks, kp)
    ldf = kp + wide_ld
    Fd = dev(R.with_padding_columns(F, ldf))                       # NaN in the columns beyond kp
    n = blocks * kp * kp

    def call(out):
        L.check(L.lib.bmf_gram_partial(L.ptr(Fd), rows_pad, ldf, kp, L.ptr(out), blocks, stream()), "bmf_gram_partial")

    S = launch_twice(call, n, [Fd]).reshape(blocks, kp, kp)
    check_slabs(S, want, ref64, mag, rows_pad, blocks, tracers, symmetric=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. bmf_gram_partial_i8: the same slabs, whatever the scale workgroups do and whether or not the stop flag is raised
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop", [None, 0, 1], ids=["stop_null", "stop_0", "stop_1"])
@pytest.mark.parametrize("fused", [0, 1], ids=["unfused", "fused"])
@pytest.mark.parametrize("blocks", [5, 192], ids=["blocks5", "blocks192_128_idle"])
@pytest.mark.parametrize("kp", [32, 64], ids=["gram_partial_kernel_1_kp32", "gram_partial_kernel_2_kp64"])
def test_gram_partial_i8_writes_the_plain_slabs(L, kp, blocks, fused, stop):
    rows_pad, limbs = 512, 3
    F, want, ref64, mag, _ = R.gram_reference("mixed", rows_pad, blocks, kp)
    Fd = dev(F)
    bm = dev(np.abs(F).reshape(rows_pad // 128, 128, kp).max(axis=1))
    flag = None if stop is None else torch.full((1,), stop, dtype=torch.int32, device="cuda")
    n = blocks * kp * kp
    scales = []

    def plain(out):
        L.check(L.lib.bmf_gram_partial(L.ptr(Fd), rows_pad, kp, kp, L.ptr(out), blocks, stream()), "bmf_gram_partial")

    def i8(out):
        scale = nan_buffer(4 * kp)
        scale[:kp] = 1.0                                           # (fused: the scale the planes were built with)
        L.check(L.lib.bmf_gram_partial_i8(L.ptr(Fd), rows_pad, kp, kp, L.ptr(out), blocks, L.ptr(bm), limbs, L.ptr(scale), fused,
                                          L.ptr(flag), stream()), "bmf_gram_partial_i8")
        torch.cuda.synchronize()
        scales.append(scale.cpu().numpy())

    base = launch_twice(plain, n, [Fd])
    S = launch_twice(i8, n, [Fd, bm] + ([] if flag is None else [flag]))
    assert S.tobytes() == base.tobytes(), ("the slabs are not those of bmf_gram_partial", differing(S, base))
    check_slabs(S.reshape(blocks, kp, kp), want, ref64, mag, rows_pad, blocks, [], symmetric=True)
    # the scale workgroups stay inside their block, and write nothing behind a raised flag (what they write: test_i8_panel_chain_gpu.py)
    used = (4 if fused else 2) * kp
    for sc in scales:
        assert (sc[used:].view(np.int32) == R.NAN_BITS).all()
        if stop == 1:
            assert (sc[:kp] == 1.0).all() and (sc[kp:].view(np.int32) == R.NAN_BITS).all()
        else:
            assert np.isfinite(sc[:used]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. bmf_gram_cross
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("same", [True, False], ids=["A_is_B", "A_not_B"])
@pytest.mark.parametrize("blocks", R.CROSS_BLOCKS)
@pytest.mark.parametrize("rows_pad", R.CROSS_ROWS)
def test_gram_cross_slab_by_slab(L, rows_pad, blocks, same, kind):
    A, B, want, ref64, mag, tracers = R.cross_reference(kind, rows_pad, blocks, same)
    Ad = dev(A)
    Bd = Ad if same else dev(B)
    n = blocks * R.BK * R.BK

    def call(out):
        L.check(L.lib.bmf_gram_cross(L.ptr(Ad), L.ptr(Bd), rows_pad, L.ptr(out), blocks, stream()), "bmf_gram_cross")

    S = launch_twice(call, n, [Ad] if same else [Ad, Bd]).reshape(blocks, R.BK, R.BK)
    check_slabs(S, want, ref64, mag, rows_pad, blocks, tracers, symmetric=same)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. bmf_fg_f32
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("ldg", [64, 128])
@pytest.mark.parametrize("rows_pad", R.FG_ROWS)
def test_fg_f32_entry_by_entry(L, rows_pad, ldg, accumulate, kind):
    F, G, O, want, ref64, mag = R.fg_reference(kind, rows_pad, accumulate)
    Fd, Gd = dev(F), dev(R.with_padding_columns(G, ldg))           # NaN beyond column 63 of G
    n = rows_pad * R.BK

    def call(out):
        L.check(L.lib.bmf_fg_f32(L.ptr(Fd), rows_pad, L.ptr(Gd), ldg, L.ptr(out), accumulate, stream()), "bmf_fg_f32")

    got = launch_twice(call, n, [Fd, Gd], head=O if accumulate else None).reshape(rows_pad, R.BK)
    assert not np.isnan(got).any(), ("unwritten or poisoned entries", int(np.isnan(got).sum()))
    err = np.abs(got.astype(np.float64) - ref64)
    within = (err <= R.bound(64 + accumulate, 65, mag)).all()
    same = np.array_equal(bits(got), bits(want))
    assert within, ("other numbers: outside the rounding bound", float((err / np.maximum(mag, 1e-300)).max()), differing(got, want))
    assert same, ("inside the bound but not the restated bits: another order", differing(got, want))
