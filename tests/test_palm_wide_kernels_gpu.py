"""The two kernels of the proximal step at a rank 64 < k <= 128 (csrc/palm_wide.hip), cell by cell in the manner of
tests/test_palm_kernels_gpu.py: bmf_sym_norms_wide against numpy.linalg.norm, and one bmf_palm_epilogue_wide call with every output it
writes -- the new fp64 masters against the fp64 formula (oracle.elbmf_update(reassoc=True) / oracle.primp_step), and everything derived
(shadow, row bits, bit-columns, gap partials, the advanced previous iterate) against the device's own new master, exactly.

The prox jumps at 0.5 (by (2 kai + lam) / (1 + lam)) and, with kai > 0, falls at 0 and 1: a cell whose argument x lies within the
fp32 rounding of the Fe G product of a kink may land on either side, which no tolerance on the factor covers.  The random inputs are
therefore drawn until the fp64 argument of every cell (of both stages for PRIMP) is at least 1e-5 from 0, 0.5 and 1 -- a hundred times
the rounding of the product (|Fe G| 2^-24 eta <= 1e-7 here).  The kinks themselves are the subject of the last test, where G = 0
and num = 0 make the argument exact."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle as orc
from test_palm_kernels_cpu import colbits_to_bool, rowbits_to_bool

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ELBMF, PRIMP = 1, 2
SPECTRAL, FROBENIUS = 0, 1
BK = 64


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def relf(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


# ---- bmf_sym_norms_wide ----------------------------------------------------------------------------------------------------------------
def norm_cases():
    rs = np.random.RandomState(34)
    B = rs.standard_normal((140, 128))
    yield "random-psd", B.T @ B
    F = rs.rand(200, 65)
    G = np.zeros((128, 128))
    G[:65, :65] = F.T @ F
    yield "gram-200x65-embedded", G
    v = np.arange(1, 129.0)
    yield "rank-one", np.outer(v, v)
    yield "zero", np.zeros((128, 128))
    yield "identity", np.eye(128)
    Q, _ = np.linalg.qr(rs.standard_normal((128, 128)))
    yield "top-pair-3-and-3-minus-1e-9", Q @ np.diag([3.0, 3.0 - 1e-9] + list(rs.rand(126))) @ Q.T
    yield "top-pair-1-and-0.99", Q @ np.diag([1.0, 0.99] + list(0.5 * rs.rand(126))) @ Q.T


@pytest.mark.parametrize("name,G", list(norm_cases()), ids=[n for n, _ in norm_cases()])
def test_sym_norms_wide_against_numpy(name, G):
    from pybmf_amd import _lib as L
    G = 0.5 * (G + G.T)
    d = torch.from_numpy(np.ascontiguousarray(G)).cuda()
    out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_sym_norms_wide(L.ptr(d), L.ptr(out), None), "bmf_sym_norms_wide")
    got = out.cpu().numpy()
    print(name, got, np.linalg.norm(G, ord=2), np.linalg.norm(G))
    if name == "zero":
        assert got[0] == 0.0 and got[1] == 0.0
        return
    assert got[0] == pytest.approx(np.linalg.norm(G, ord=2), rel=1e-9)
    assert got[1] == pytest.approx(np.linalg.norm(G), rel=1e-12)
    out2 = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.bmf_sym_norms_wide(L.ptr(d), L.ptr(out2), None), "bmf_sym_norms_wide")
    assert np.array_equal(out2.cpu().numpy(), got)       # fixed order of every sum


# ---- bmf_palm_epilogue_wide ---------------------------------------------------------------------------------------------------------------
def blocks_of(A, rows_pad, dtype):
    """rows x k host array -> two zero-padded rows_pad x 64 device blocks"""
    out = []
    for b in range(2):
        t = np.zeros((rows_pad, BK), dtype=dtype)
        part = A[:, BK * b: BK * b + BK]
        t[: part.shape[0], : part.shape[1]] = part
        out.append(torch.from_numpy(t).cuda())
    return out


def launch(a):
    """One bmf_palm_epilogue_wide call on host inputs `a`; every output as host arrays, the factor-shaped ones as rows_pad x 128."""
    from pybmf_amd import _lib as L
    rows_pad, rows, k = a["rows_pad"], a["rows"], a["k"]
    F64, P64 = blocks_of(a["F"], rows_pad, np.float64), blocks_of(a["Fprev"], rows_pad, np.float64)
    F32 = [t.float() for t in F64]
    G = np.zeros((128, 128), np.float32)
    G[:k, :k] = a["G"]
    Gd = [[torch.from_numpy(np.ascontiguousarray(G[BK * i: BK * i + BK, BK * j: BK * j + BK])).cuda() for j in range(2)] for i in range(2)]
    num = [torch.from_numpy(np.ascontiguousarray(a["num"][b])).cuda() for b in range(2)]          # [splits][stride] fp32 per block
    norms = torch.from_numpy(np.asarray(a["norms"], dtype=np.float64)).cuda()
    rb = [torch.full((rows_pad,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    cb = [torch.full((BK, rows_pad // 32), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    part = [torch.full((rows_pad // 128,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    s = L.PalmWideArgs()
    s.struct_bytes = C.sizeof(L.PalmWideArgs)
    s.rows, s.k, s.splits, s.rows_pad, s.slab_stride = rows, k, a["num"][0].shape[0], rows_pad, a["num"][0].shape[1]
    for b in range(2):
        s.F64[b], s.Fprev64[b], s.F[b], s.num[b] = F64[b].data_ptr(), P64[b].data_ptr(), F32[b].data_ptr(), num[b].data_ptr()
        s.rowbits[b], s.colbits[b], s.partials[b] = rb[b].data_ptr(), cb[b].data_ptr(), part[b].data_ptr()
        for j in range(2):
            s.G[b][j] = Gd[b][j].data_ptr()
    s.norms, s.norm_kind, s.variant = norms.data_ptr(), a["norm_kind"], a["variant"]
    s.beta, s.l1, s.l2, s.gap_l1, s.gap_l2 = a["beta"], a["l1"], a["l2"], a["gap_l1"], a["gap_l2"]
    s.advance_prev, s.thr, s.ldcb = a["advance_prev"], 0.5, rows_pad // 32
    L.check(L.lib.bmf_palm_epilogue_wide(C.byref(s), None), "bmf_palm_epilogue_wide")
    torch.cuda.synchronize()
    cat = lambda ts: np.concatenate([t.cpu().numpy() for t in ts], axis=1)   # noqa: E731
    return dict(F64=cat(F64), Fprev64=cat(P64), F=cat(F32), partials=[p.cpu().numpy() for p in part],
                rowbits=np.concatenate([rowbits_to_bool(t.cpu().numpy(), BK) for t in rb], axis=1),
                colbits=np.concatenate([colbits_to_bool(t.cpu().numpy(), rows_pad) for t in cb], axis=1))


def step_inputs(k, variant, beta, seed):
    """A 130-row factor (a second 128-row block holding two rows) against a 200-row other factor, num = X H in three slabs with junk in
    their padding; (inputs, the fp64 formula's new factor, the smallest distance of a prox argument to a kink)."""
    rs = np.random.RandomState(seed)
    rows, rows_pad, n = 130, 256, 200
    X = (rs.rand(rows, n) < 0.3).astype(np.float64)
    H = rs.rand(n, k) * 0.3
    F = rs.rand(rows, k) * 1.2
    Fprev = F + 0.1 * rs.standard_normal((rows, k))
    G = H.T @ H
    kind = SPECTRAL if variant == ELBMF else FROBENIUS
    norms = np.array([np.linalg.norm(G, 2), np.linalg.norm(G)])
    l1, l2 = 0.02 * norms[0], 0.05 * norms[0]
    total = X @ H
    stride = rows_pad * BK + 96
    num = []
    for b in range(2):
        slabs = np.full((3, stride), 3.0, np.float32)                 # junk beyond the array
        t = rs.rand(rows_pad, BK).astype(np.float32) * 5.0            # junk in padded rows and columns
        part = total[:, BK * b: BK * b + BK]
        t[:rows, : part.shape[1]] = part
        r = rs.rand(rows_pad * BK).astype(np.float32)
        slabs[0, : rows_pad * BK], slabs[1, : rows_pad * BK], slabs[2, : rows_pad * BK] = r * t.ravel(), 2 * (1 - r) * t.ravel(), -(1 - r) * t.ravel()
        num.append(slabs)
    a = dict(rows=rows, rows_pad=rows_pad, k=k, F=F, Fprev=Fprev, G=G.astype(np.float32), num=num, norms=norms, norm_kind=kind, variant=variant, beta=beta,
             l1=l1, l2=l2, gap_l1=0.3, gap_l2=1.7)
    eta = orc.elbmf_step_size(G, beta, "spectral" if variant == ELBMF else "fro")
    fe = F + beta * (F - Fprev)
    x = fe - eta * (fe @ G - total)
    args = [x]
    if variant == ELBMF:
        want, _ = orc.elbmf_update(X, F, H, None, l1, l2, beta, Fprev, reassoc=True)
    else:
        want = orc.primp_step(X, F, np.ascontiguousarray(H.T), Fprev, l1, l2, 1.0, beta)
        # the argument of the second prox is max(p, 0): p < 0 gives exactly 0 on either side, p > 0 itself -- and the second prox, which
        # has no lower clamp, falls at 0 too
        args.append(orc.primp_prox(x, l1 * eta, l2 * eta))
    margin = min(float(np.abs(v - t).min()) for v in args for t in (0.0, 0.5, 1.0))
    return a, want, margin


@pytest.mark.parametrize("variant", [ELBMF, PRIMP], ids=["elbmf", "primp"])
@pytest.mark.parametrize("k", [65, 72, 127, 128])
def test_palm_epilogue_wide_cell_by_cell(k, variant):
    from pybmf_amd.models.ELBMF import get_integrality_gap
    for beta, advance in itertools.product((0.0, 0.2), (0, 1)):
        for seed in range(3400, 3500):
            a, want, margin = step_inputs(k, variant, beta, seed)
            if margin >= 1e-5:
                break
        else:
            raise AssertionError("no inputs keep their distance from the kinks")
        a["advance_prev"] = advance
        rows, rows_pad = a["rows"], a["rows_pad"]
        got = launch(a)
        tag = (k, variant, beta, advance, seed)
        new = got["F64"]
        print(tag, "margin", margin, "rel", relf(new[:rows, :k], want))
        assert relf(new[:rows, :k], want) < 1e-5, tag
        assert not new[rows:].any() and not new[:, k:].any() and not got["F"][rows:].any() and not got["F"][:, k:].any(), tag
        assert np.array_equal(got["F"], new.astype(np.float32)), tag
        bits = new > 0.5
        assert np.array_equal(got["rowbits"], bits) and np.array_equal(got["colbits"], bits), tag
        for b in range(2):
            blk = new[:, BK * b: BK * b + BK]
            want_gap = sum(get_integrality_gap(blk[128 * i: 128 * i + 128][: max(0, min(128, rows - 128 * i)), : min(BK, k - BK * b)], 0.3, 1.7)
                           for i in range(rows_pad // 128))
            assert got["partials"][b].sum() == pytest.approx(want_gap, rel=1e-12), tag
            assert got["partials"][b][1] == pytest.approx(get_integrality_gap(blk[128:rows, : min(BK, k - BK * b)], 0.3, 1.7), rel=1e-12), tag
        Fpad, Ppad = np.zeros((rows_pad, 128)), np.zeros((rows_pad, 128))
        Fpad[:rows, :k], Ppad[:rows, :k] = a["F"], a["Fprev"]
        assert np.array_equal(got["Fprev64"], Fpad if advance else Ppad), tag
        again = launch(a)
        for name in ("F64", "F", "Fprev64", "rowbits", "colbits"):
            assert np.array_equal(again[name], got[name]), (tag, name)
        assert all(np.array_equal(p, q) for p, q in zip(again["partials"], got["partials"])), tag


@pytest.mark.parametrize("variant", [ELBMF, PRIMP], ids=["elbmf", "primp"])
def test_palm_epilogue_wide_at_the_kinks(variant):
    """G = 0 and num = 0: the step is prox(Fe) and its argument is exact.  Entries at 0, 0.5, 1, the two neighbours of 0.5 and negative
    values, in both blocks and in both 128-row blocks, against the host prox / proxelbmfnn chain to 1e-15."""
    from pybmf_amd.models.ELBMF import prox
    from pybmf_amd.models.PRIMP import _proxelbmfnn, proxelbmfnn
    rows, rows_pad, k = 130, 256, 100
    special = np.array([0.0, 0.5, 1.0, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), -0.3, -1e-9, 0.25, 0.75, 1.4, np.nextafter(1.0, 2.0), 5e-324])
    F = np.resize(special, (rows, k)).copy()
    assert all(np.isin(special, F[r0:r1, c0:c1]).all() for r0, r1 in ((0, 128), (128, 130)) for c0, c1 in ((0, 64), (64, 100)))
    norms = np.array([2.0, 3.0])
    zeros = [np.zeros((1, rows_pad * BK), np.float32) for _ in range(2)]
    for l1, l2 in ((0.0, 0.0), (0.05, 0.4)):
        a = dict(rows=rows, rows_pad=rows_pad, k=k, F=F, Fprev=F.copy(), G=np.zeros((k, k), np.float32), num=zeros, norms=norms,
                 norm_kind=SPECTRAL if variant == ELBMF else FROBENIUS, variant=variant, beta=0.0, l1=l1, l2=l2, gap_l1=0.0, gap_l2=0.0, advance_prev=1)
        eta = 1.0 / (1.1 * norms[0 if variant == ELBMF else 1])
        kai, lam = l1 * eta, l2 * eta
        want = prox(F, kai, lam) if variant == ELBMF else _proxelbmfnn(proxelbmfnn(F, kai, lam), kai, lam)
        got = launch(a)
        np.testing.assert_allclose(got["F64"][:rows, :k], want, rtol=0, atol=1e-15)
        assert not got["F64"][rows:].any() and not got["F64"][:, k:].any()
        assert np.array_equal(got["rowbits"], got["F64"] > 0.5)
