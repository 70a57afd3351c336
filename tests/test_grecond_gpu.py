"""GreConD on the device: the concept kernels (csrc/grecond.hip) against the NumPy stand-in of tests/test_grecond_cpu.py on the
recorded get_concept calls and on ragged shapes, GreConD.fit() against the reference's results (tests/golden/g23_grecond.*), and one
run at the MovieLens-1M shape that no reference stands behind, held to the invariants of any correct GreConD.

Everything is integers: every comparison is equality.
"""
import ctypes as C
import time

import numpy as np
import pytest

from boolean_family import grecond_invariants
from test_grecond_cpu import (NumpyConceptEngine, check_fit, close_concept, fit_case, load_case, log_rows, pack_rows, popcount, scan_block,
                              unpack)

pytestmark = pytest.mark.gpu

MARK = -7


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def device_scan(ref, best_u, cands, best_score, extra=3):
    """bmf_concept_scan on the stand-in's matrices; outputs pre-filled with a marker, `extra` slots behind them must keep it."""
    import torch
    from pybmf_amd._lib import check, lib
    Xt, rs = dev(ref.Xt.view(np.int32)), dev(ref.rs_t.view(np.int32))
    nc = len(cands)
    work = torch.full((int(lib.bmf_concept_scan_work(nc)) // 8 + 1,), MARK, dtype=torch.int64, device="cuda:0")
    score = torch.full((nc + extra,), MARK, dtype=torch.int64, device="cuda:0")
    nu = torch.full((nc + extra,), MARK, dtype=torch.int32, device="cuda:0")
    nv = torch.full((nc + extra,), MARK, dtype=torch.int32, device="cuda:0")
    rec = torch.full((8,), MARK, dtype=torch.int64, device="cuda:0")
    bu, cd = dev(best_u.view(np.int32)), dev(np.asarray(cands, dtype=np.int32))     # (named: they must outlive the launch)
    check(lib.bmf_concept_scan(vp(Xt), vp(rs), ref.n, ref.W, vp(bu), vp(cd), nc, int(best_score), vp(work), vp(score), vp(nu), vp(nv),
                               vp(rec), None), "bmf_concept_scan")
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (score, nu, nv, rec)]
    for a in out[:3]:
        assert (a[nc:] == MARK).all()
    assert (out[3][5:] == MARK).all()
    return out[0][:nc], out[1][:nc], out[2][:nc], out[3][:5]


def device_close(ref, best_u, j):
    import torch
    from pybmf_amd._lib import check, lib
    u = dev(best_u.view(np.int32).copy())
    v = torch.full((ref.nvw + 2,), MARK, dtype=torch.int32, device="cuda:0")
    Xt = dev(ref.Xt.view(np.int32))
    check(lib.bmf_concept_close(vp(Xt), ref.n, ref.W, int(j), None, vp(u), vp(v), None), "bmf_concept_close")
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    written = -(-ref.n // 64) * 2
    assert (v[written:] == MARK).all()
    return u.cpu().numpy().view(np.uint32), v[:written].view(np.uint32)


def device_apply(ref, u, v):
    import torch
    from pybmf_amd._lib import check, lib
    rs, pd = dev(ref.rs_t.view(np.int32)), dev(ref.pd_t.view(np.int32))
    cc = torch.full((ref.n + 3,), MARK, dtype=torch.int32, device="cuda:0")
    rsum = torch.full((2,), MARK, dtype=torch.int64, device="cuda:0")
    ud, vd = dev(u.view(np.int32)), dev(v.view(np.int32))
    check(lib.bmf_concept_apply(vp(rs), vp(pd), ref.n, ref.W, vp(ud), vp(vd), vp(cc), vp(rsum), None), "bmf_concept_apply")
    torch.cuda.synchronize()
    cc, rsum = cc.cpu().numpy(), rsum.cpu().numpy()
    assert (cc[ref.n:] == MARK).all() and rsum[1] == MARK
    return rs.cpu().numpy().view(np.uint32), pd.cpu().numpy().view(np.uint32), cc[: ref.n], int(rsum[0])


def check_point(ref, best_u, cands, best_score, label):
    """Scan, close and apply on the device against the stand-in at one state."""
    cands = np.asarray(cands, dtype=np.int64)
    s0, nu0, nv0, first0 = scan_block(ref.Xt, ref.rs_t, ref.n, best_u, cands, best_score)
    s1, nu1, nv1, rec1 = device_scan(ref, best_u, cands, best_score)
    s2, nu2, nv2, rec2 = device_scan(ref, best_u, cands, best_score)
    print(f"grecond scan {label}: {len(cands)} candidates, first winner {first0}, max score {int(s0.max())}, empty u_j {int((nu0 == 0).sum())}")
    assert s1.tolist() == s0.tolist() and nu1.tolist() == nu0.tolist() and nv1.tolist() == nv0.tolist()
    want = [first0, cands[first0], s0[first0], nu0[first0], nv0[first0]] if first0 >= 0 else [-1, -1, 0, 0, 0]
    assert rec1.tolist() == [int(x) for x in want]
    assert all(a.tobytes() == b.tobytes() for a, b in ((s1, s2), (nu1, nu2), (nv1, nv2), (rec1, rec2)))   # two calls: the same bits
    j = int(cands[first0]) if first0 >= 0 else int(cands[0])
    u0, v0 = close_concept(ref.Xt, ref.n, best_u, j, ref.nvw)
    u1, v1 = device_close(ref, best_u, j)
    assert u1.tobytes() == u0.tobytes() and v1.tobytes() == v0[: v1.size].tobytes() and not v0[v1.size:].any()
    rs1, pd1, cc1, rsum1 = device_apply(ref, u0, v0)
    before = ref.residual_sum()
    ref.apply(u0, v0)
    assert rs1.tobytes() == ref.rs_t.tobytes() and pd1.tobytes() == ref.pd_t.tobytes()
    assert cc1.tolist() == [popcount(r) for r in ref.rs_t[: ref.n]] and rsum1 == ref.residual_sum()
    if first0 >= 0:
        assert before - rsum1 == s0[first0]


@pytest.mark.parametrize("name", ["a", "b"])
def test_kernels_at_the_recorded_calls(name):
    case = load_case(name)
    for i, p in enumerate(case["points"]):
        ref = NumpyConceptEngine(case["X"])
        ref.rs_t = pack_rows(p["X_rs"].T, ref.W)
        ref.pd_t = ref.Xt & ~ref.rs_t
        j_rs = np.nonzero(p["X_rs"].sum(axis=0) > 0)[0]
        check_point(ref, ref.all_rows, j_rs, 0, f"{name}{i} first sweep")
        # a later state of the same call: the recorded u as best_u, one below the recorded score to beat
        ref = NumpyConceptEngine(case["X"])
        ref.rs_t = pack_rows(p["X_rs"].T, ref.W)
        ref.pd_t = ref.Xt & ~ref.rs_t
        check_point(ref, pack_rows(p["u"][None, :], ref.W)[0], j_rs, p["score"] - 1, f"{name}{i} closing sweep")
        _, _, _, rec = device_scan(ref, pack_rows(p["u"][None, :], ref.W)[0], j_rs, p["score"])
        assert rec.tolist() == [-1, -1, 0, 0, 0]          # the recorded concept is the fixed point: nothing beats it


# (32256 padded rows: the most the scan takes, 63 KiB of row sets in LDS and a last chunk of 48 words)
@pytest.mark.parametrize("m,n", [(37, 1), (100, 45), (600, 530), (2100, 70), (513, 65), (32256, 40), (31800, 33)])
def test_kernels_at_ragged_shapes(m, n):
    rng = np.random.RandomState(100 * m + n)
    X = rng.rand(m, n) < 0.3
    X[:, 0] = True                                    # a column of all ones
    if n > 4:
        X[: m // 2, 3] = False                        # with best_u below, u_3 is empty
        X[:, 4] = X[:, 2]                             # equal columns: each lies in the other's closure
    ref = NumpyConceptEngine(X)
    resid = X & (rng.rand(m, n) < 0.7)
    ref.rs_t, ref.pd_t = pack_rows(resid.T, ref.W), pack_rows((X & ~resid).T, ref.W)
    check_point(ref, ref.all_rows, np.arange(n), 0, f"{m}x{n} all rows")
    ref = NumpyConceptEngine(X)
    ref.rs_t, ref.pd_t = pack_rows(resid.T, ref.W), pack_rows((X & ~resid).T, ref.W)
    half = pack_rows((np.arange(m) < m // 2)[None, :], ref.W)[0]
    cands = np.arange(n)[::-1] if n > 1 else np.arange(n)          # any order of candidates is a list
    check_point(ref, half, cands, 10 ** 12, f"{m}x{n} upper half, nothing can win")
    ref = NumpyConceptEngine(X)
    ref.rs_t, ref.pd_t = pack_rows(resid.T, ref.W), pack_rows((X & ~resid).T, ref.W)
    check_point(ref, half, np.arange(n), 3, f"{m}x{n} upper half")


def test_engine_scan_hooks_and_row_limit():
    """The engine's own launch (what concept() and scripts/grecond_times.py use) against the stand-in, and the refusal above the limit."""
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.grecond import ConceptEngine
    case = load_case("a")
    ref, eng = NumpyConceptEngine(case["X"]), ConceptEngine(BitMatrix(case["X"], "cuda:0"))
    cands = eng.residual_columns()
    assert cands.tolist() == np.nonzero(case["X"].sum(axis=0) > 0)[0].tolist()
    half = pack_rows((np.arange(ref.m) % 3 == 0)[None, :], ref.W)[0]
    for best_u in (None, half):
        eng.set_search_state(best_u, cands)
        eng.launch_scan(0, len(cands), 5)
        s1, nu1, nv1, rec1 = eng.scan_results(len(cands))
        s0, nu0, nv0, first0 = scan_block(ref.Xt, ref.rs_t, ref.n, ref.all_rows if best_u is None else best_u, cands, 5)
        assert s1.tolist() == s0.tolist() and nu1.tolist() == nu0.tolist() and nv1.tolist() == nv0.tolist() and rec1[0] == first0
    with pytest.raises(NotImplementedError, match="32256"):
        ConceptEngine(BitMatrix(np.zeros((32257, 3), dtype=np.uint8), "cuda:0"))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_fit_reproduces_the_reference(name):
    case = load_case(name)
    t0 = time.time()
    model = fit_case(case)
    wall = time.time() - t0
    print(f"grecond fit {name}: {len(log_rows(model))} rows, {model.U.shape[1]} factors kept, {wall:.2f} s "
          f"({wall / max(len(log_rows(model)), 1) * 1e3:.1f} ms per concept)")
    from pybmf_amd.grecond import ConceptEngine
    assert isinstance(model._engine, ConceptEngine)
    check_fit(model, case)


@pytest.mark.parametrize("block", [1, 7, 40])
def test_block_size_on_the_device(block):
    case = load_case("a")
    check_fit(fit_case(case, block=block), case)


def planted_ml1m():
    """6040 x 3706, about 4.5 % ones: 26 planted rectangles (6 % of the rows x 3 % of the columns each), 0.1 % of the cells flipped."""
    rng = np.random.RandomState(2310)
    m, n, k = 6040, 3706, 26
    U, V = rng.rand(m, k) < 0.06, rng.rand(n, k) < 0.03
    X = (U.astype(np.float32) @ V.astype(np.float32).T) > 0
    X ^= rng.rand(m, n) < 0.001
    return X.astype(np.uint8)


def test_ml1m_shape_invariants():
    import contextlib
    import io
    from pybmf_amd.models import GreConD
    X = planted_ml1m()
    print(f"grecond ml1m: density {X.mean():.4f}")
    assert 0.035 < X.mean() < 0.055
    k = 20
    with contextlib.redirect_stdout(io.StringIO()):
        model = GreConD(k=k)
        t0 = time.time()
        model.fit(X, task="reconstruction", show_logs=False, show_result=False, save_model=False)
        wall = time.time() - t0
    print(f"grecond ml1m: k = {k} fit {wall:.2f} s")
    rows = log_rows(model)
    assert len(rows) == k
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    assert U.shape == (X.shape[0], k) and V.shape == (X.shape[1], k)
    # every factor a closed rectangle of ones, score = the drop of the residual sum, FP = 0 in every row, the counts and the prediction
    covered = grecond_invariants(X, rows, U, V, model._engine.counts("train"), model._engine.residual_sum(), np.asarray(model.X_pd.todense()))
    assert int(covered.sum()) == model._engine.counts("train")[0]
    # the first three concepts against the stand-in, and block sizes against each other
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.grecond import ConceptEngine
    ref, eng = NumpyConceptEngine(X), ConceptEngine(BitMatrix(X, "cuda:0"))
    for f in range(3):
        t0 = time.time()
        s0, u0, v0 = ref.concept()
        t1 = time.time()
        s1, u1, v1 = eng.concept(block=None if f != 1 else 500)
        t2 = time.time()
        print(f"grecond ml1m concept {f}: score {s1}, shape [{popcount(u1)}, {popcount(v1)}], {eng.launches} launches, {eng.accepted} accepted, "
              f"device {t2 - t1:.3f} s, NumPy stand-in {t1 - t0:.1f} s")
        assert s1 == s0 == rows[f][1] and u1.tobytes() == u0.tobytes() and v1.tobytes() == v0.tobytes()
        assert unpack(u1, X.shape[0]).tolist() == U[:, f].tolist() and unpack(v1, X.shape[1]).tolist() == V[:, f].tolist()
        ref.apply(u0, v0)
        eng.apply(u1, v1)
        assert eng.residual_sum() == ref.residual_sum() and eng.counts("train") == ref.counts("train")
