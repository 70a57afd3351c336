"""MEBF on the device: the kernels of csrc/mebf.hip against the NumPy stand-in of tests/test_mebf_cpu.py at the family's boundary
shapes, the selection and the threshold on constructed inputs, the engine's residual / cover bookkeeping, MEBF.fit() against the
reference's results (tests/golden/g27_mebf.*), and one run at 2049 x 300 that no reference stands behind, held to invariants.

Everything is integers and bits: every comparison is equality.  Outputs are pre-filled with a marker and have slots behind them that
must keep it.
"""
import ctypes as C

import numpy as np
import pytest

from boolean_family import BOUNDARY, planted
from test_grecond_cpu import pack_rows, popcount, unpack
from test_mebf_cpu import (CASES, NumpyMedianEngine, check_fit, check_state, fit_case, grow, load_case, log_rows, order, row_popcounts,
                           select_median)

pytestmark = pytest.mark.gpu

MARK = -7


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def marked(n, dtype):
    import torch
    return torch.full((n,), MARK, dtype=dtype, device="cuda:0")


def device_scores(R, N):
    import torch
    from pybmf_amd._lib import check, lib
    Rd, score, out = dev(R.view(np.int32)), marked(N + 3, torch.int32), marked(3, torch.int64)
    check(lib.bmf_mebf_scores(vp(Rd), N, R.shape[1], vp(score), vp(out), None), "bmf_mebf_scores")
    torch.cuda.synchronize()
    score, out = score.cpu().numpy(), out.cpu().numpy()
    assert (score[N:] == MARK).all() and out[2] == MARK
    return score[:N], int(out[0]), int(out[1])


def device_select(scores, weak=0):
    import torch
    from pybmf_amd._lib import check, lib
    sd, rec = dev(np.asarray(scores, dtype=np.int32)), marked(11, torch.int64)
    check(lib.bmf_mebf_select(vp(sd), len(scores), weak, vp(rec), None), "bmf_mebf_select")
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    assert (rec[8:] == MARK).all() and not rec[2:8].any()
    return int(rec[0]), int(rec[1])


def device_grow(rs, x, pd, N, t, mid=None, a=None):
    """bmf_mebf_grow with a taken from bit row `mid` on the device (a is None) or given; (a, b as bools over N, |a|, |b|, dTP, dFP)."""
    import torch
    from pybmf_amd._lib import check, lib
    ld, nbw = rs.shape[1], -(-N // 32)
    rd, xd, pdd = dev(rs.view(np.int32)), dev(x.view(np.int32)), dev(pd.view(np.int32))
    ad = marked(ld + 4, torch.int32)
    if a is not None:
        ad[:ld] = dev(a.view(np.int32))
    bd, work = marked(nbw + 3, torch.int32), marked(3 * N + 3, torch.int32)
    rec = marked(9, torch.int64)
    rec[:8] = 0
    rec[0] = -1 if mid is None else mid
    check(lib.bmf_mebf_grow(vp(rd), vp(xd), vp(pdd), N, ld, vp(ad), int(a is None), float(t), vp(work), vp(bd), nbw, vp(rec), None), "bmf_mebf_grow")
    torch.cuda.synchronize()
    ad, bd, work, rec = (z.cpu().numpy() for z in (ad, bd, work, rec))
    assert (ad[ld:] == MARK).all() and (bd[nbw:] == MARK).all() and (work[3 * N:] == MARK).all() and rec[8] == MARK
    assert rd.cpu().numpy().tobytes() == rs.tobytes()
    b = unpack(bd[:nbw].view(np.uint32), nbw * 32)
    assert not b[N:].any()
    return ad[:ld].view(np.uint32), b[:N], int(rec[2]), int(rec[3]), int(rec[4]), int(rec[5])


def device_apply(rs, pd, N, hit, mask, score, pdcount):
    import torch
    from pybmf_amd._lib import check, lib
    rd, pdd, hd, md = dev(rs.view(np.int32)), dev(pd.view(np.int32)), dev(hit.view(np.int32)), dev(mask.view(np.int32))
    sd, cd = marked(N + 3, torch.int32), marked(N + 3, torch.int32)
    sd[:N], cd[:N] = dev(score.astype(np.int32)), dev(pdcount.astype(np.int32))
    out = marked(3, torch.int64)
    check(lib.bmf_mebf_apply(vp(rd), vp(pdd), N, rs.shape[1], vp(hd), vp(md), vp(sd), vp(cd), vp(out), None), "bmf_mebf_apply")
    torch.cuda.synchronize()
    sd, cd, out = sd.cpu().numpy(), cd.cpu().numpy(), out.cpu().numpy()
    assert (sd[N:] == MARK).all() and (cd[N:] == MARK).all() and out[2] == MARK
    return rd.cpu().numpy().view(np.uint32), pdd.cpu().numpy().view(np.uint32), sd[:N], cd[:N], int(out[0]), int(out[1])


def state_after(X, factors=2, t=0.6):
    """A stand-in engine on X with a few factors applied: a residual that differs from X and a non-empty cover."""
    ref = NumpyMedianEngine(X)
    for _ in range(factors):
        c = ref.growth(t)[0]
        if c["na"] and c["nb"]:
            ref.apply(c["u"], c["v"])
    return ref


@pytest.mark.parametrize("shape", BOUNDARY)
def test_kernels_at_the_boundary_shapes(shape):
    m, n = shape
    X = planted(m, n, 3, 0.3, 0.03, 2700 + m)
    ref = state_after(X)
    st = ref._live
    for axis in (0, 1):
        N, rs, pd, x = ref.N[axis], st.rs[axis], st.pd[axis], ref.x[axis]
        want = row_popcounts(rs[:N])
        score, total, npos = device_scores(rs, N)
        assert score.tolist() == want.tolist() and total == int(want.sum()) and npos == int((want > 0).sum())
        mid, P = select_median(want)
        assert device_select(want) == (mid, P)
        if N >= 2:
            assert device_select(want, weak=1) == tuple(int(i) for i in order(want)[:2])
        for t in (0.0, 0.3, 0.6):
            b0, na0, nb0, tp0, fp0 = grow(rs, x, pd, N, rs[mid], t)
            a1, b1, na1, nb1, tp1, fp1 = device_grow(rs, x, pd, N, t, mid=mid)
            assert a1.tobytes() == rs[mid].tobytes() and b1.tolist() == b0.tolist() and (na1, nb1, tp1, fp1) == (na0, nb0, tp0, fp0)
            assert tp1 == popcount(rs[:N][b0] & rs[mid])          # the cover is X & ~residual here: dTP is the residual ones of a x b
        # apply: the candidate of this axis on this orientation's matrices
        c = ref.growth(0.6)[axis]
        hit, mask = (c["v"], c["u"]) if axis == 0 else (c["u"], c["v"])
        rs1, pd1, s1, c1, rsum, pdsum = device_apply(rs, pd, N, hit, mask, want, row_popcounts(pd[:N]))
        after = NumpyMedianEngine(X)
        after._live.rs, after._live.pd = [z.copy() for z in st.rs], [z.copy() for z in st.pd]
        after.apply(c["u"], c["v"])
        assert rs1.tobytes() == after._live.rs[axis].tobytes() and pd1.tobytes() == after._live.pd[axis].tobytes()
        assert s1.tolist() == row_popcounts(rs1[:N]).tolist() and c1.tolist() == row_popcounts(pd1[:N]).tolist()
        assert (rsum, pdsum) == (popcount(rs1), popcount(pd1))


def test_selection():
    rng = np.random.RandomState(2711)
    vectors = {
        "all equal": np.full(300, 7), "P = 1": np.eye(1, 130, 77, dtype=int)[0] * 5, "P = 2": np.array([0, 3, 0, 3, 0]),
        "P even": np.array([2, 9, 2, 0, 9, 4, 2, 0, 1]), "P odd": np.array([2, 9, 2, 0, 9, 4, 2, 0]), "all zero": np.zeros(70, dtype=int),
        # 5000 scores, 5 per thread of the 1024: the tie group of the median (value 3, indices 40 .. 3100) spans 64-lane chunks, the
        # contiguous chunks of many threads and more than 1024 indices
        "wide tie": np.concatenate([np.full(40, 9), np.full(3061, 3), rng.randint(0, 3, 1899)]),
        "random": rng.randint(0, 6, 2049), "one": np.array([4]),
    }
    for label, s in vectors.items():
        assert device_select(s) == select_median(s), label
        if len(s) >= 2:
            assert device_select(s, weak=1) == tuple(int(i) for i in order(s)[:2]), label
    assert device_select(vectors["all zero"]) == (-1, 0)
    top3 = np.array([1, 8, 0, 8, 2, 8, 3])                # the top score held by three indices: the two highest indices, in that order
    assert device_select(top3, weak=1) == (5, 3)
    # nothing is grown from P = 0: a, b empty and every count zero
    X = np.zeros((33, 65), dtype=np.uint8)
    ref = NumpyMedianEngine(X)
    a, b, na, nb, tp, fp = device_grow(ref._live.rs[0], ref.x[0], ref._live.pd[0], 65, 0.5, mid=None)
    assert not a.any() and not b.any() and (na, nb, tp, fp) == (0, 0, 0, 0)


def test_threshold_is_strict_and_in_fp64():
    m, n = 70, 40
    R = np.zeros((m, n), dtype=np.uint8)
    R[:10, 0] = 1                      # a = column 0: |a| = 10
    R[:5, 1] = 1                       # c = 5 = 0.5 * 10 exactly: left out
    R[:6, 2] = 1                       # c = 6: in
    R[:10, 3] = 1                      # c = 10 = 1.0 * 10: in at t = 0.5, out at t = 1.0
    R[20:30, 4] = 1                    # c = 0: out even at t = 0 (0 > 0 is false)
    ref = NumpyMedianEngine(R)
    rs, x, pd = ref._live.rs[0], ref.x[0], ref._live.pd[0]
    for t, cols in ((0.5, [0, 2, 3]), (0.0, [0, 1, 2, 3]), (1.0, []), (0.59, [0, 2, 3]), (0.6, [0, 3])):
        a, b, na, nb, tp, fp = device_grow(rs, x, pd, n, t, mid=0)
        b0, na0, nb0, tp0, fp0 = grow(rs, x, pd, n, rs[0], t)
        assert np.nonzero(b)[0].tolist() == cols == np.nonzero(b0)[0].tolist(), t
        assert (na, nb, tp, fp) == (10, len(cols), tp0, fp0)
        assert fp == sum(10 - int(R[:10, j].sum()) for j in cols)
    assert 0.6 * 10 == 6.0         # (the fp64 product is exactly 6: column 2, c = 6, is out at t = 0.6 by the strict comparison)


def test_weak_signal_with_disjoint_top_columns():
    X = np.zeros((40, 6), dtype=np.uint8)
    X[:12, 1], X[20:31, 4], X[35:, 2] = 1, 1, 1
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.mebf import MedianEngine
    eng, ref = MedianEngine(BitMatrix(X, "cuda:0")), NumpyMedianEngine(X)
    got, want = eng.weak(0.5), ref.weak(0.5)
    assert (got["mid"], got["P"]) == (1, 4) == (want["mid"], want["P"])
    assert (got["na"], got["nb"], got["dTP"], got["dFP"]) == (0, 0, 0, 0) and not got["u"].any() and not got["v"].any()


def same_candidate(got, want):
    for key in ("axis", "mid", "P", "na", "nb", "dTP", "dFP"):
        assert got[key] == want[key], key
    assert got["u"].tobytes() == want["u"].tobytes() and got["v"].tobytes() == want["v"].tobytes()


def same_bits(eng, ref):
    """The engine's four bit matrices (zero padded to 512 bit rows) against the stand-in's (its bit rows only)."""
    for a, b in zip(eng.bit_matrices(), ref.bit_matrices()):
        assert a[: b.shape[0]].tobytes() == b.tobytes() and not a[b.shape[0]:].any()


def test_engine_keeps_both_orientations_and_rebuilds():
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.mebf import MedianEngine
    X = planted(65, 129, 3, 0.3, 0.03, 2720)
    eng, ref = MedianEngine(BitMatrix(X, "cuda:0")), NumpyMedianEngine(X)
    applied = []
    for i in range(3):
        got, want = eng.growth(0.6), ref.growth(0.6)
        for g, w in zip(got, want):
            same_candidate(g, w)
        same_candidate(eng.weak(0.6), ref.weak(0.6))
        got = eng.growth(0.6)                              # (the weak call made the first candidates stale: take fresh ones)
        c = got[i % 2]
        assert c["na"] and c["nb"]
        reads = eng.reads
        eng.apply(c["u"], c["v"], c)
        assert eng.reads == reads                          # applied from the device's own vectors, counts from the record
        ref.apply(c["u"], c["v"])
        applied.append((c["u"], c["v"]))
        R, P = check_state(eng, X)
        same_bits(eng, ref)
        assert eng.counts("train") == ref.counts("train") and eng.error_counts() == ref.error_counts()
    before = [z.copy() for z in eng.bit_matrices()]
    eng.rebuild(applied)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(eng.bit_matrices(), before))
    assert eng.counts("train") == ref.counts("train")
    # a truncation: the candidates are counted against the cover of the kept factors, the next apply starts from them
    eng.truncate(applied[:1])
    ref.truncate(applied[:1])
    assert eng.base_counts() == ref.base_counts() != eng.error_counts()
    for g, w in zip(eng.growth(0.6), ref.growth(0.6)):
        same_candidate(g, w)
    c = ref.growth(0.6)[0]
    eng.apply(c["u"], c["v"])
    ref.apply(c["u"], c["v"])
    check_state(eng, X)
    same_bits(eng, ref)
    assert eng.counts("train") == ref.counts("train")


@pytest.mark.parametrize("name", CASES)
def test_fit_on_the_device_reproduces_the_reference(name):
    case = load_case(name)
    model = fit_case(case)
    check_fit(model, case)
    check_state(model._engine, case["X"])
    want = fit_case(case, lambda mdl: __import__("test_mebf_cpu").numpy_engine(mdl))
    assert log_rows(model) == log_rows(want)
    for nm in model._engine.truth:
        assert model._engine.counts(nm) == want._engine.counts(nm)


def test_fit_without_a_reference_keeps_the_invariants():
    from pybmf_amd._lib import check, lib
    X = planted(2049, 300, 5, 0.2, 0.03, 2730)
    # cost starts at X.sum(), which is the weighted error of the empty prediction only for w_fn = 1: the identity below needs it
    w_fp, w_fn = 2, 1
    model = fit_case(dict(X=X, k=5, tol=0, t=0.7, w_fp=w_fp, w_fn=w_fn))
    eng = model._engine
    rows = log_rows(model)
    assert len(rows) == 5 and model.U.shape[1] == 5
    R, P = check_state(eng, X)                                        # X_rs = X & ~X_pd, in both orientations
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    assert (P == ((U.astype(np.int64) @ V.T.astype(np.int64)) > 0)).all()
    import torch
    st = eng._live
    work, conf = torch.zeros(2 * eng.n, dtype=torch.int32, device="cuda:0"), torch.zeros(2, dtype=torch.int64, device="cuda:0")
    check(lib.bmf_bits_confusion(vp(st.pd[0]), vp(eng.x[0]), eng.n, eng.W, vp(work), vp(conf), None), "bmf_bits_confusion")
    tp, n_pd = (int(v) for v in conf.cpu().numpy())
    fp, fn = n_pd - tp, int(X.sum()) - tp
    assert (tp, fp, fn) == eng.counts("train")[:3] == (int((P & (X != 0)).sum()), int((P & (X == 0)).sum()), int((~P & (X != 0)).sum()))
    assert rows[-1][0] == w_fp * fp + w_fn * fn                       # cost: exact, integer weights
    costs = [float(X.sum())] + [r[0] for r in rows]
    assert all(b - a <= 0 for a, b in zip(costs, costs[1:]))          # every accepted d_cost <= 0
    assert [r[3] for r in rows][-1] == fn and eng.reads <= 2 * len(rows) + 2
