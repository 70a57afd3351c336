"""The cover-count and bit utility kernels of csrc/cover.hip and csrc/util.hip, called through the C ABI on every launch path, against
the packed-word restatements of tests/bits_ref.py (pinned to the oracle's dense definitions, and its case tables to the launch paths
they claim, by tests/test_bit_kernels_cpu.py).  Integer kernels: every count and every word must be equal.  The two fp64 sums
(bmf_sqdiff_sum, bmf_reduce_slabs) must be exact on integer-valued data and within a derived bound on random data:

  bmf_sqdiff_sum     |got - fsum| <= (n + 4) 2^-53 fsum     any summation order of n non-negative terms (n - 1 additions, each with a
                                                            relative error of 2^-53 of a partial sum <= the total), three roundings per
                                                            term (A - B, d * d, W * .), and the rounding of the reference's own terms
  bmf_reduce_slabs   |out64 - ref| <= count 2^-53 sum|v|    count - 1 additions in any order; the float -> double conversions are exact

Inputs are made on the host with fixed seeds; padding words and bytes hold ones.  No factor bit at or above kp is ever set: the product
kernel indexes colbits by the set bits without looking at kp.  Run with -s to see each case's launch plan and the observed ratios."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bits_ref as R  # noqa: E402
import oracle as orc  # noqa: E402

RATIOS = {}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib as L
    yield L, torch.device("cuda:0"), int(torch.cuda.get_device_properties(0).multi_processor_count)
    print()
    for key in sorted(RATIOS):
        print(f"RATIO {key}: observed / bound = {RATIOS[key]:.3g}")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def dev(a):
    """host array -> device tensor, unsigned words as the signed type of the same width"""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:      # the shared cases are read-only; torch wants a writable source
        a = a.copy()
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))


# ---- bmf_cover_count ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kp", R.COVER_PARAMS)
def test_cover_count(env, name, kp):
    """(TP, FP) equal the reference and are added to what counts held; a second call doubles them; a set stop word skips the call."""
    L, d, cus = env
    c = R.cover_case(name, kp, cus)
    print(name, kp, {k: v for k, v in c.items() if not isinstance(v, np.ndarray)}, R.cover_launch_plan(c["rows_pad"], c["words"], cus))
    X, u, colw = dev(c["X"]), dev(c["u"]), dev(c["colw"])
    assert X.shape == (c["rows_pad"], c["ldx"]) and colw.shape == (kp, c["ldcb"]) and u.shape == (c["rows_pad"],)
    counts = torch.tensor([7, 11, 13, 17], dtype=torch.int64, device=d)
    stop = torch.zeros(1, dtype=torch.int32, device=d)

    def call(stop_word):
        L.check(L.lib.bmf_cover_count(L.ptr(X), c["rows_pad"], c["ldx"], c["words"], L.ptr(u), L.ptr(colw), c["ldcb"], kp, L.ptr(counts),
                                      L.ptr(stop_word), stream()), "bmf_cover_count")
        return tuple(int(v) for v in counts.cpu().numpy())

    tp, fp = c["tp"], c["fp"]
    assert call(None) == (7 + tp, 11 + fp, 13, 17)
    assert call(stop) == (7 + 2 * tp, 11 + 2 * fp, 13, 17)        # stop word 0: counts
    stop.fill_(1)
    assert call(stop) == (7 + 2 * tp, 11 + 2 * fp, 13, 17)        # stop word 1: untouched


# ---- bmf_boolean_product_bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("name", [c[0] for c in R.PRODUCT_CASES])
def test_boolean_product_bits(env, name, kp):
    L, d, _ = env
    c = R.product_case(name, kp)
    fill = R.PRODUCT_SENTINEL if c["ldo"] > c["words"] else R.ONES       # ones: a row whose factor word is zero must come out zero
    out = dev(np.full((c["rows"], c["ldo"]), fill, np.uint32))
    u, colw = dev(c["u"]), dev(c["colw"])
    L.check(L.lib.bmf_boolean_product_bits(L.ptr(u), c["rows"], L.ptr(colw), c["ldcb"], kp, c["words"], L.ptr(out), c["ldo"], stream()),
            "bmf_boolean_product_bits")
    got = host_u32(out)
    assert np.array_equal(got[:, :c["words"]], c["want"])
    assert (got[:, c["words"]:] == fill).all()
    if c["rows"] > 1:
        assert c["u"][1] == 0 and not got[1, :c["words"]].any()


@pytest.mark.parametrize("k", [65, 128, 130])
def test_boolean_product_bits_beyond_64_factors(env, k):
    """device_ops.boolean_product_bits: the OR of the products of the 64-column blocks"""
    L, d, _ = env
    from pybmf_amd import device_ops as D
    m, n = 70, 200
    rs = np.random.RandomState(k)
    Ub, Vb = rs.rand(m, k) < 0.03, rs.rand(n, k) < 0.05
    Ub[0] = False
    Ub[0, k - 1] = Vb[n - 1, k - 1] = True
    Ub[1] = False
    want = orc.boolean_product(Ub.astype(np.int64), Vb.astype(np.int64))
    assert want[0, n - 1] == 1 and 0 < want.mean() < 0.6 and not want[1].any()
    bits = D.boolean_product_bits(Ub, Vb, d)
    got = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert np.array_equal(got[:m, :n], want) and not got[m:].any() and not got[:, n:].any()
    assert np.array_equal(D.boolean_product_csr(Ub, Vb, device=d).toarray(), want)


# ---- bmf_confusion_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,words,dg,dp", R.CONFUSION_CASES)
def test_confusion_rows(env, rows, words, dg, dp):
    L, d, _ = env
    c = R.confusion_case(rows, words, dg, dp)
    G, P = dev(c["G"]), dev(c["P"])
    tp = torch.full((rows,), -1, dtype=torch.int32, device=d)
    fp = torch.full((rows,), -1, dtype=torch.int32, device=d)
    L.check(L.lib.bmf_confusion_rows(L.ptr(G), c["ldg"], L.ptr(P), c["ldp"], rows, words, L.ptr(tp), L.ptr(fp), stream()), "bmf_confusion_rows")
    assert np.array_equal(tp.cpu().numpy(), c["tp"]) and np.array_equal(fp.cpu().numpy(), c["fp"])


@pytest.fixture(scope="module")
def metrics_problem():
    m, n, k = 70, 4100, 40
    rs = np.random.RandomState(70)
    X = (rs.rand(m, n) < 0.3).astype(np.int64)
    Ub, Vb = (rs.rand(m, k) < 0.05).astype(np.int64), (rs.rand(n, k) < 0.1).astype(np.int64)
    Ub[5] = 0
    return X, Ub, Vb, orc.boolean_product(Ub, Vb)


@pytest.mark.parametrize("axis", [None, 0, 1])
def test_metrics_confusion_by_axis(env, metrics_problem, axis):
    from pybmf_amd.utils import metrics as M
    X, Ub, Vb, pd = metrics_problem
    got = M.confusion(X, pd, axis)
    want = orc.confusion_counts_axis(X, pd, axis)
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w))
    assert np.asarray(want[0]).sum() > 0 and np.asarray(want[1]).sum() > 0


def test_description_length_without_a_prediction(env, metrics_problem):
    from pybmf_amd.utils import metrics as M
    X, Ub, Vb, pd = metrics_problem
    tp, fp, fn, tn = orc.confusion_counts(X, pd)
    for w_model, w_fp, w_fn in [(1.0, 1.0, 1.0), (0.5, 2.0, 3.0)]:
        dense = w_model * (Ub.sum() + Vb.sum()) + w_fp * fp + w_fn * fn
        assert M.description_length(X, Ub, Vb, None, w_model, w_fp, w_fn) == dense
        assert M.description_length(X, Ub, Vb, pd, w_model, w_fp, w_fn) == dense


# ---- bmf_pack_rows_u8 / bmf_popcount ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,dx,dw", R.PACK_CASES)
def test_pack_rows_u8(env, rows, cols, dx, dw):
    """bytes other than 0 / 1 count as set, padding bytes of 255 are not packed, words past the packed pairs are not written"""
    L, d, _ = env
    c = R.pack_case(rows, cols, dx, dw)
    X = dev(c["X"])
    bits = dev(np.full((rows, c["ldw"]), R.PACK_SENTINEL, np.uint32))
    L.check(L.lib.bmf_pack_rows_u8(L.ptr(X), rows, cols, c["ldx"], L.ptr(bits), c["ldw"], stream()), "bmf_pack_rows_u8")
    got = host_u32(bits)
    assert np.array_equal(got[:, :c["need"]], c["want"])
    assert (got[:, c["need"]:] == R.PACK_SENTINEL).all()
    # and the count of what was packed, added to a preset that makes the sum carry into the high word
    preset = (1 << 32) - 5
    count = torch.tensor([preset], dtype=torch.int64, device=d)
    L.check(L.lib.bmf_popcount(L.ptr(bits), rows, c["need"], c["ldw"], L.ptr(count), stream()), "bmf_popcount")
    assert int(count.item()) == preset + int((c["X"][:, :cols] != 0).sum())


@pytest.mark.parametrize("rows,words,dw", R.POPCOUNT_CASES)
def test_popcount(env, rows, words, dw):
    L, d, _ = env
    rng = np.random.default_rng([20244, rows, words, dw])
    W = R.padded(R.random_words(rng, (rows, words)), words + dw)
    want = R.popcount(W[:, :words])
    assert want > 0 and (dw == 0 or R.popcount(W) > want)
    bits = dev(W)
    preset = (1 << 32) - 5
    count = torch.tensor([preset, 23], dtype=torch.int64, device=d)
    L.check(L.lib.bmf_popcount(L.ptr(bits), rows, words, words + dw, L.ptr(count), stream()), "bmf_popcount")
    assert count.cpu().numpy().tolist() == [preset + want, 23]
    assert preset + want >= 1 << 32 or rows * words < 4


# ---- bmf_sqdiff_sum -----------------------------------------------------------------------------------------------------------------
def sqdiff_call(L, d, A, B, W, n, preset):
    work = torch.zeros(int(L.lib.bmf_sqdiff_work()), dtype=torch.float64, device=d)
    out = torch.tensor([preset, -1.5], dtype=torch.float64, device=d)
    Ad, Bd, Wd = dev(A), dev(B), (None if W is None else dev(W))
    L.check(L.lib.bmf_sqdiff_sum(L.ptr(Ad), L.ptr(Bd), L.ptr(Wd), n, L.ptr(work), L.ptr(out), stream()), "bmf_sqdiff_sum")
    got = out.cpu().numpy()
    assert got[1] == -1.5
    return float(got[0])


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", R.SQDIFF_N)
def test_sqdiff_sum_exact_on_small_integers(env, n, weighted):
    """|values| <= 8: every term and every partial sum is an integer below 2^53, so any summation order gives the same fp64 number"""
    L, d, _ = env
    rs = np.random.RandomState(n % 1000 + 7)
    size = max(n, 1)      # n = 0: valid pointers, nothing read, `out` unchanged
    A, B = rs.randint(-8, 9, size=size).astype(np.float64), rs.randint(-8, 9, size=size).astype(np.float64)
    W = rs.randint(0, 9, size=size).astype(np.float64) if weighted else None
    want = R.sqdiff(A[:n], B[:n], None if W is None else W[:n])
    if n >= 255:
        assert want > 0 and (W is None or ((W[:n] == 0).any() and want != R.sqdiff(A[:n], B[:n])))
    assert sqdiff_call(L, d, A, B, W, n, 0.0) == want
    assert sqdiff_call(L, d, A, B, W, n, 3.0) == 3.0 + want           # out +=


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", [n for n in R.SQDIFF_N if n])
def test_sqdiff_sum_random_within_the_summation_bound(env, n, weighted):
    L, d, _ = env
    rs = np.random.RandomState(n % 1000 + 8)
    A, B = rs.randn(n), rs.randn(n) * 3.0
    W = None
    if weighted:
        W = rs.rand(n) * 4.0
        W[::5] = 0.0
    want = R.sqdiff(A, B, W)
    got = sqdiff_call(L, d, A, B, W, n, 0.0)
    bound = (n + 4) * 2.0 ** -53 * want
    ratio = abs(got - want) / bound if bound > 0 else float(got != want)
    print(f"sqdiff n={n} weighted={weighted}: |got - fsum| / ((n + 4) 2^-53 fsum) = {ratio:.3g}")
    note("bmf_sqdiff_sum", ratio)
    assert abs(got - want) <= bound


@pytest.mark.parametrize("sparse", [False, True])
def test_weighted_sqdiff_in_chunks(env, sparse):
    """device_ops.weighted_sqdiff: three row chunks (17 + 17 + 16 rows of 70) add up to the one-chunk result, exactly on integer data"""
    L, d, _ = env
    from pybmf_amd import device_ops as D
    import scipy.sparse as sp
    rs = np.random.RandomState(50)
    A, B = rs.randint(0, 9, size=(50, 70)).astype(np.float64), rs.randint(0, 9, size=(50, 70)).astype(np.float64)
    W = rs.randint(0, 4, size=(50, 70)).astype(np.float64)
    want = R.sqdiff(A, B, W)
    conv = sp.csr_matrix if sparse else (lambda a: a)
    one = D.weighted_sqdiff(conv(A), conv(B), conv(W), device=d)
    three = D.weighted_sqdiff(conv(A), conv(B), conv(W), device=d, chunk_cells=17 * 70)
    assert len(range(0, 50, max(1, (17 * 70) // 70))) == 3
    assert one == three == want and want > 0
    assert D.weighted_sqdiff(conv(A), conv(B), None, device=d, chunk_cells=17 * 70) == R.sqdiff(A, B)


# ---- bmf_reduce_slabs ---------------------------------------------------------------------------------------------------------------
def reduce_call(L, d, slabs_t, stride, count, n, want32, want64, alias=False):
    """one call; returns (out32 or None, out64 or None) as host arrays.  alias: out32 is the first slab"""
    o32 = slabs_t if alias else (torch.full((n,), -7.0, dtype=torch.float32, device=d) if want32 else None)
    o64 = torch.full((n,), -7.0, dtype=torch.float64, device=d) if want64 else None
    L.check(L.lib.bmf_reduce_slabs(L.ptr(slabs_t), stride, count, n, L.ptr(o32), L.ptr(o64), stream()), "bmf_reduce_slabs")
    return (None if o32 is None else o32[:n].cpu().numpy()), (None if o64 is None else o64.cpu().numpy())


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                 b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("n", R.REDUCE_N)
def test_reduce_slabs(env, n):
    """n >= 65536 (a multiple of 4, aligned pointers): the float4 kernel; below: the 64 x 16 kernel.  Every count and both strides;
    out32 only, out64 only, both, and out32 aliasing the first slab; the padding between slabs holds 1e30 and is never read."""
    L, d, _ = env
    rs = np.random.RandomState(n % 977)
    for count in R.REDUCE_COUNTS:
        for stride in (n, n + 4):
            for kind in ("integers", "random"):
                if kind == "integers":      # integer-valued, |v| < 2^20: every partial sum is exact in fp64
                    vals = rs.randint(-(1 << 20) + 1, 1 << 20, size=(count, n)).astype(np.float32)
                else:
                    # magnitudes spread over 2^-30 .. 2^30: sums of 24-bit floats of similar size would be exact in fp64
                    vals = np.ldexp(rs.randn(count, n), rs.randint(-30, 31, size=(count, n))).astype(np.float32)
                slabs = np.full((count, stride), 1e30, np.float32)
                slabs[:, :n] = vals
                ref = R.reduce_slabs(slabs.ravel(), stride, count, n)
                sd = dev(slabs.ravel())
                a32, a64 = reduce_call(L, d, sd, stride, count, n, True, True)
                b32, _ = reduce_call(L, d, sd, stride, count, n, True, False)
                _, c64 = reduce_call(L, d, sd, stride, count, n, False, True)
                assert same_bits(a32, a64.astype(np.float32))          # out32 is the rounding of the same sum
                assert same_bits(a32, b32) and same_bits(a64, c64)
                if kind == "integers":
                    assert np.array_equal(a64, ref), (count, stride)
                else:
                    bound = count * 2.0 ** -53 * np.abs(vals.astype(np.float64)).sum(axis=0)
                    err = np.abs(a64 - ref)
                    note("bmf_reduce_slabs", (err / bound).max())
                    assert (err <= bound).all(), (count, stride, float((err / bound).max()))
                assert np.array_equal(sd.cpu().numpy(), slabs.ravel())          # the slabs are inputs
                # out32 = the first slab: its n sums replace slab 0, nothing else changes
                d32, d64 = reduce_call(L, d, sd, stride, count, n, True, True, alias=True)
                assert same_bits(d32, a32) and same_bits(d64, a64)
                after = sd.cpu().numpy().reshape(count, stride)
                assert np.array_equal(after[1:], slabs[1:]) and np.array_equal(after[0, n:], slabs[0, n:])
                if n == 65536:
                    # the same data one float further on: not 16-byte aligned, so the 64 x 16 kernel runs.  It adds 16 groups of
                    # ceil(count / 16) consecutive slabs: for count <= 16 that is slab order, the float4 kernel's order, and the
                    # two results are equal bit for bit on any data; for larger counts they are equal where the sums are exact
                    # (integers) and both within the bound otherwise
                    off = torch.empty(count * stride + 1, dtype=torch.float32, device=d)[1:]
                    off.copy_(dev(slabs.ravel()))
                    assert off.data_ptr() % 16 == 4
                    e32, e64 = reduce_call(L, d, off, stride, count, n, True, True)
                    assert same_bits(e32, e64.astype(np.float32))
                    if kind == "integers" or count <= 16:
                        assert same_bits(e64, a64) and same_bits(e32, a32), (count, stride, kind)
                    else:
                        assert (np.abs(e64 - ref) <= bound).all()
    if "bmf_reduce_slabs" in RATIOS:
        print(f"reduce_slabs n={n}: worst |out64 - ref| / (count 2^-53 sum|v|) so far = {RATIOS['bmf_reduce_slabs']:.3g}")
