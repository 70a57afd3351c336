"""The three entry points of csrc/link_wide.hip -- bmf_link_pass_wide, bmf_link_sums_wide, bmf_masked_link_pass_wide -- by direct
C ABI calls against NumPy fp64 on the fp32-rounded factors the kernels see; both links, both orientations.

Shapes (m, n, k):
    (1, 1, 65)         smallest case
    (33, 31, 65)       one ragged tile, one column in block 1
    (129, 97, 72)      a second 128-row workgroup with one live row, a ragged last column tile
    (130, 700, 128)    two column splits one way, six row blocks the other

Gates: those of tests/test_link_gpu.py::test_link_pass_and_sums_against_numpy for the exact-fp32 pass, rtol 2e-5 + atol 1e-6 on num /
den and 2e-5 relative on the sums.  The factors are scaled so that P = U V^T is around 1/2, where the sigmoid link is steepest (at the
scale of that test a rank-128 product sits near 13 and every d underflows).  Every case prints its worst deviation as a fraction of its
gate (run with -s).  Padding: output rows >= rows are exact zeros, X bits set beyond (rows, cols) change no bit of any output, the
inputs are unchanged, a marker-filled guard slab after every output stays intact."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402

SHAPES = [(1, 1, 65), (33, 31, 65), (129, 97, 72), (130, 700, 128)]
LAM = 7.0
RTOL, ATOL = 2e-5, 1e-6
MARK = -7.0
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    print()
    for key in sorted(WORST, key=str):
        print("WORST (fraction of the gate)", key, " ".join(f"{n}={v:.3g}" for n, v in sorted(WORST[key].items())))


def note(key, **figures):
    slot = WORST.setdefault(key, {})
    for name, value in figures.items():
        slot[name] = max(slot.get(name, 0.0), float(value))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pad128(x):
    return (max(x, 1) + 127) // 128 * 128


def gate_fraction(got, want):
    """max over the entries of |got - want| / (atol + rtol |want|): <= 1 is what assert_allclose(rtol, atol) accepts"""
    return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want))))


def sums_fraction(got, want):
    """max relative deviation of the sums as a fraction of RTOL (a zero reference must be met exactly)"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    nz = want != 0
    assert np.array_equal(got[~nz], want[~nz])
    return float(np.max(np.abs(got[nz] / want[nz] - 1), initial=0.0) / RTOL)


def pack_bits(X, rows_pad, ldx, poison):
    """rows_pad x ldx words, bit j % 32 of word j / 32; `poison`: every bit outside the rows x cols matrix set"""
    rows, cols = X.shape
    full = np.full((rows_pad, ldx * 32), 1 if poison else 0, dtype=np.uint8)
    full[:rows, :cols] = X
    return np.packbits(full, axis=1, bitorder="little").view(np.uint32).reshape(rows_pad, ldx)


def blocks_of(F, rows_pad, k):
    """the two zero-padded 64-column fp32 blocks of a factor (the layout of pybmf_amd/wide.py)"""
    out = []
    for b in range(2):
        t = np.zeros((rows_pad, 64), dtype=np.float32)
        part = F[:, 64 * b: min(64 * b + 64, k)]
        t[: F.shape[0], : part.shape[1]] = part
        out.append(torch.from_numpy(t).cuda())
    return out


@functools.lru_cache(maxsize=None)
def case(m, n, k):
    """X, the factors (fp64 values of their fp32 roundings) and the fp64 references of one shape, computed once"""
    rs = np.random.RandomState(1000 * k + 7 * m + n)
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    s = np.sqrt(0.5 / k) / 0.8                                   # E[P] ~ 1/2
    U = (np.abs(rs.standard_normal((m, k))) * s + 1e-3).astype(np.float32).astype(np.float64)
    V = (np.abs(rs.standard_normal((n, k))) * s + 1e-3).astype(np.float32).astype(np.float64)
    P = U @ V.T
    sig = orc.stable_sigmoid((P - 0.5) * LAM)
    d = sig * (1 - sig)
    for a in (X, U, V, P, sig, d):
        a.setflags(write=False)
    return dict(X=X, U=U, V=V, P=P, sig=sig, d=d)


def oriented(m, n, k, transposed, poison=False):
    c = case(m, n, k)
    X, Fs, Fo = (c["X"].T, c["V"], c["U"]) if transposed else (c["X"], c["U"], c["V"])
    rows, cols = X.shape
    rows_pad, other_pad = pad128(rows), pad128(cols)
    ldx = (cols + 31) // 32 + 1                                    # one spare word per row
    bits = torch.from_numpy(pack_bits(X.astype(np.uint8), rows_pad, ldx, poison).view(np.int32)).cuda()
    T = (lambda a: a.T) if transposed else (lambda a: a)
    return dict(X=X, Fs=Fs, Fo=Fo, rows=rows, cols=cols, rows_pad=rows_pad, other_pad=other_pad, ldx=ldx, bits=bits, k=k,
                Fsd=blocks_of(Fs, rows_pad, k), Fod=blocks_of(Fo, other_pad, k), P=T(c["P"]), sig=T(c["sig"]), d=T(c["d"]))


def run_pass(o, link):
    """one bmf_link_pass_wide call; (num, den) per block as [splits + 1][rows_pad][64] host arrays, the last slab a marker-filled guard"""
    from pybmf_amd import _lib as L
    splits = L.lib.bmf_link_splits(o["rows"], o["cols"])
    outs = [torch.full((splits + 1, o["rows_pad"], 64), MARK, device="cuda") for _ in range(4)]
    keep = [t.clone() for t in (o["bits"], *o["Fsd"], *o["Fod"])]
    L.check(L.lib.bmf_link_pass_wide(L.ptr(o["bits"]), o["rows_pad"], o["ldx"], o["rows"], o["cols"], L.ptr(o["Fsd"][0]), L.ptr(o["Fsd"][1]),
                                     L.ptr(o["Fod"][0]), L.ptr(o["Fod"][1]), o["other_pad"], o["k"], link, LAM, L.ptr(outs[0]), L.ptr(outs[1]),
                                     L.ptr(outs[2]), L.ptr(outs[3]), o["rows_pad"] * 64, splits, stream()), "bmf_link_pass_wide")
    torch.cuda.synchronize()
    for a, b in zip(keep, (o["bits"], *o["Fsd"], *o["Fod"])):
        assert torch.equal(a, b)                                   # the inputs are unchanged
    return splits, [t.cpu().numpy() for t in outs]


def joined(slabs0, slabs1, splits, rows, k):
    """the two blocks' slab sums side by side: rows x k, fp64"""
    return np.concatenate([slabs0[:splits].astype(np.float64).sum(0), slabs1[:splits].astype(np.float64).sum(0)], axis=1)[:rows, :k]


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_link_pass_wide_against_numpy(m, n, k, transposed):
    from pybmf_amd import _lib as L
    o = oriented(m, n, k, transposed)
    po = oriented(m, n, k, transposed, poison=True)
    rows, X, Fo = o["rows"], o["X"], o["Fo"]
    for link in (L.LINK_SIGMOID, L.LINK_KL):
        splits, (n0, n1, d0, d1) = run_pass(o, link)
        if m == 130 and n == 700:
            assert splits == (1 if transposed else 2)
        num = joined(n0, n1, splits, rows, k)
        if link == L.LINK_SIGMOID:
            want_num, want_den = LAM * (X * o["d"]) @ Fo, LAM * (o["sig"] * o["d"]) @ Fo
            den = joined(d0, d1, splits, rows, k)
            note((m, n, k, "T" if transposed else "N", "sigmoid"), num=gate_fraction(num, want_num), den=gate_fraction(den, want_den))
            np.testing.assert_allclose(den, want_den, rtol=RTOL, atol=ATOL)
            written = (n0, n1, d0, d1)
        else:
            want_num = (X / o["P"]) @ Fo
            note((m, n, k, "T" if transposed else "N", "kl"), num=gate_fraction(num, want_num))
            assert (d0 == MARK).all() and (d1 == MARK).all()       # KL: den is not written
            written = (n0, n1)
        np.testing.assert_allclose(num, want_num, rtol=RTOL, atol=ATOL)
        for t in written:
            assert not t[:splits, rows:].any()                     # output rows >= rows: exact zeros
            assert (t[splits] == MARK).all()                       # the guard slab is intact
        assert not n1[:splits, :, k - 64:].any()                   # columns >= k: the factor padding is zero
        # X bits set beyond (rows, cols) change nothing
        _, poisoned = run_pass(po, link)
        for a, b in zip((n0, n1, d0, d1), poisoned):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("m,n,k", SHAPES[1:])
def test_block_zero_agrees_with_the_narrow_pass_when_block_one_is_zero(m, n, k):
    """With block 1 all zero, P is the product over block 0 alone: block 0 of the output is bmf_link_pass at kp = 64 of the same factors."""
    from pybmf_amd import _lib as L
    o = oriented(m, n, k, False)
    zero_s, zero_o = torch.zeros_like(o["Fsd"][1]), torch.zeros_like(o["Fod"][1])
    splits = L.lib.bmf_link_splits(o["rows"], o["cols"])
    stride = o["rows_pad"] * 64
    for link in (L.LINK_SIGMOID, L.LINK_KL):
        wide = [torch.full((splits, o["rows_pad"], 64), MARK, device="cuda") for _ in range(4)]
        L.check(L.lib.bmf_link_pass_wide(L.ptr(o["bits"]), o["rows_pad"], o["ldx"], o["rows"], o["cols"], L.ptr(o["Fsd"][0]), L.ptr(zero_s),
                                         L.ptr(o["Fod"][0]), L.ptr(zero_o), o["other_pad"], k, link, LAM, L.ptr(wide[0]), L.ptr(wide[1]),
                                         L.ptr(wide[2]), L.ptr(wide[3]), stride, splits, stream()), "bmf_link_pass_wide")
        narrow = [torch.full((splits, o["rows_pad"], 64), MARK, device="cuda") for _ in range(2)]
        L.check(L.lib.bmf_link_pass(L.ptr(o["bits"]), o["rows_pad"], o["ldx"], o["rows"], o["cols"], L.ptr(o["Fsd"][0]), L.ptr(o["Fod"][0]),
                                    o["other_pad"], 64, link, LAM, L.ptr(narrow[0]), L.ptr(narrow[1]), stride, splits, stream()), "bmf_link_pass")
        pairs = [(wide[0], narrow[0])] + ([(wide[2], narrow[1])] if link == L.LINK_SIGMOID else [])
        for w, nr in pairs:
            w, nr = w.double().sum(0).cpu().numpy(), nr.double().sum(0).cpu().numpy()
            note((m, n, k, "block 1 zero", link), vs_narrow=gate_fraction(w, nr))
            np.testing.assert_allclose(w, nr, rtol=RTOL, atol=ATOL)
        assert not wide[1].any()                                   # block 1 of the output: g times zeros


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_link_sums_wide_against_numpy(m, n, k):
    from pybmf_amd import _lib as L
    c = case(m, n, k)
    X, P, sig = c["X"], c["P"], c["sig"]
    rs = np.random.RandomState(m + n)
    O = ((rs.rand(m, n) < 0.6) | (X != 0)).astype(np.uint8)       # observed cells: every non-zero of X and 60 % of the rest
    for poison in (False, True):
        o = oriented(m, n, k, False, poison)
        ob = torch.from_numpy(pack_bits(O, o["rows_pad"], o["ldx"], poison).view(np.int32)).cuda()
        kl_cell = np.where(X > 0, -np.log(P) - 1 + P, P)
        for link, obits, want in ((L.LINK_SIGMOID, None, (np.abs(X - sig).sum(), ((X - sig) ** 2).sum())),
                                  (L.LINK_KL, None, (np.abs(X - P).sum(), ((X - P) ** 2).sum(), kl_cell.sum())),
                                  (L.LINK_KL, ob, (np.abs(X - P).sum(), ((X - P) ** 2).sum(), (kl_cell * O).sum()))):
            sums = torch.cat([torch.zeros(3, dtype=torch.float64), torch.full((2,), MARK, dtype=torch.float64)]).cuda()
            L.check(L.lib.bmf_link_sums_wide(L.ptr(o["bits"]), o["rows_pad"], o["ldx"], m, n, L.ptr(o["Fsd"][0]), L.ptr(o["Fsd"][1]), L.ptr(o["Fod"][0]),
                                             L.ptr(o["Fod"][1]), o["other_pad"], k, link, LAM, L.ptr(obits), L.ptr(sums), stream()), "bmf_link_sums_wide")
            got = sums.cpu().numpy()
            note((m, n, k, "sums", link, obits is not None), sums=sums_fraction(got[: len(want)], want))
            np.testing.assert_allclose(got[: len(want)], want, rtol=RTOL)
            assert (got[3:] == MARK).all()
            if link == L.LINK_SIGMOID:
                assert got[2] == 0.0


def observed_cells(m, n, k):
    """a SparseObs of ~40 % of the cells (explicit zeros included), real weights, one unobserved row and column where the shape allows"""
    from pybmf_amd.engine import SparseObs
    c = case(m, n, k)
    rs = np.random.RandomState(3 * m + n)
    obs = rs.rand(m, n) < 0.4
    if m > 3 and n > 3:
        obs[2, :] = False
        obs[:, 1] = False
    obs[0, 0] = True
    W = obs * rs.choice([0.5, 1.0, 2.0], size=(m, n))
    r, cc = np.nonzero(obs)
    return SparseObs(r, cc, c["X"][r, cc], W[r, cc], (m, n), "cuda:0"), W


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_masked_link_pass_wide_against_numpy(m, n, k):
    from pybmf_amd import _lib as L
    c = case(m, n, k)
    X, U, V, P, sig, d = (c[x] for x in ("X", "U", "V", "P", "sig", "d"))
    so, W = observed_cells(m, n, k)
    Pc = np.maximum(P, 1e-30)
    for transposed in (False, True):
        ls, rows = (so.csc, n) if transposed else (so.csr, m)
        T = (lambda a: a.T) if transposed else (lambda a: a)
        Fs, Fo = (V, U) if transposed else (U, V)
        Fsd, Fod = blocks_of(Fs, pad128(Fs.shape[0]), k), blocks_of(Fo, pad128(Fo.shape[0]), k)
        part = [torch.zeros((max(ls["nseg"], 1), 2, 64), device="cuda") for _ in range(2)]
        for link in (L.LINK_SIGMOID, L.LINK_KL):
            outs = [torch.full((rows + 1, 64), MARK, device="cuda") for _ in range(4)]
            sums = torch.cat([torch.zeros(2, dtype=torch.float64), torch.full((2,), MARK, dtype=torch.float64)]).cuda()
            keep = [t.clone() for t in (*Fsd, *Fod, ls["val"], ls["wgt"], ls["idx"])]
            L.check(L.lib.bmf_masked_link_pass_wide(L.ptr(ls["ptr"]), L.ptr(ls["idx"]), L.ptr(ls["val"]), L.ptr(ls["wgt"]), rows, L.ptr(ls["seg_row"]),
                                                    L.ptr(ls["seg_beg"]), ls["nseg"], L.ptr(ls["row_seg_ptr"]), L.ptr(Fsd[0]), L.ptr(Fsd[1]), L.ptr(Fod[0]),
                                                    L.ptr(Fod[1]), L.ptr(part[0]), L.ptr(part[1]), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]),
                                                    L.ptr(outs[3]), L.ptr(sums), link, LAM, stream()), "bmf_masked_link_pass_wide")
            for a, b in zip(keep, (*Fsd, *Fod, ls["val"], ls["wgt"], ls["idx"])):
                assert torch.equal(a, b)
            n0, n1, d0, d1 = (t.cpu().numpy() for t in outs)
            for t in (n0, n1, d0, d1):
                assert (t[rows] == MARK).all()
            num = np.concatenate([n0[:rows], n1[:rows]], axis=1).astype(np.float64)[:, :k]
            den = np.concatenate([d0[:rows], d1[:rows]], axis=1).astype(np.float64)[:, :k]
            got = sums.cpu().numpy()
            assert (got[2:] == MARK).all()
            if link == L.LINK_SIGMOID:
                want_num, want_den = LAM * T(W * X * d) @ Fo, LAM * T(W * sig * d) @ Fo
                want_sums = ((W * (X - sig) ** 2).sum(), (W * np.abs(X - sig)).sum())
                note((m, n, k, "masked", "T" if transposed else "N", "sigmoid"), num=gate_fraction(num, want_num), den=gate_fraction(den, want_den),
                     sums=sums_fraction(got[:2], want_sums))
                np.testing.assert_allclose(den, want_den, rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(got[:2], want_sums, rtol=RTOL)
            else:
                want_num = T(W * X / Pc) @ Fo
                want_kl = 2.0 * (W * np.where(X > 0, -np.log(Pc) - 1 + P, P)).sum()
                note((m, n, k, "masked", "T" if transposed else "N", "kl"), num=gate_fraction(num, want_num), sums=sums_fraction(got[0], want_kl))
                assert not den.any() and got[1] == 0.0            # KL: the caller supplies the denominator
                assert got[0] == pytest.approx(want_kl, rel=RTOL)
            np.testing.assert_allclose(num, want_num, rtol=RTOL, atol=ATOL)
            assert not n1[:rows, k - 64:].any() and not d1[:rows, k - 64:].any()
