"""Panda on the device: the kernels of csrc/panda.hip against the NumPy stand-in of tests/test_panda_cpu.py at the family's boundary
shapes, the three decisions on constructed inputs at their kinks, first-winner and correlation-pick semantics, Panda.fit() against
the reference's results (tests/golden/g28_panda.*) at three block sizes, and one fit at 2049 x 300 that no reference stands behind,
held to invariants.

Everything is integers and bits: every comparison is equality.  Outputs are pre-filled with a marker and have slots behind them that
must keep it.
"""
import ctypes as C

import numpy as np
import pytest

from boolean_family import BOUNDARY, planted
from test_grecond_cpu import pack_rows, popcount, unpack
from test_mebf_cpu import row_popcounts
from test_panda_cpu import (CASES, STEP_CASES, NumpyPatternEngine, check_fit, check_state, check_steps, core_d_cost, core_scan,
                            couples_scores, description_length, ext_scan, fit_case, load_case, log_rows, numpy_engine, rows_pass)

pytestmark = pytest.mark.gpu

MARK = -7
WEIGHTS = [(1.0, 1.0, 1.0), (0.3, 0.7, 1.1)]      # (w_model, w_fp, w_fn)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def marked(n, dtype):
    import torch
    return torch.full((n,), MARK, dtype=dtype, device="cuda:0")


def words(t):
    return t.cpu().numpy().view(np.uint32)


def device_couples(rs_t, n, rowcount):
    import torch
    from pybmf_amd._lib import check, lib
    rd, cd, out = dev(rs_t.view(np.int32)), dev(np.asarray(rowcount, dtype=np.int32)), marked(n + 3, torch.int64)
    check(lib.bmf_panda_couples(vp(rd), n, rs_t.shape[1], vp(cd), len(rowcount), vp(out), None), "bmf_panda_couples")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n:] == MARK).all()
    return out[:n]


def device_core_scan(rs_t, n, T, cands, mode, w_model, w_fn, w0, h0, close=True):
    """(h1, winner, pick, T after the close, |T| the close counted)."""
    import torch
    from pybmf_amd._lib import check, lib
    count, ld = len(cands), rs_t.shape[1]
    rd, Td = dev(rs_t.view(np.int32)), marked(ld + 4, torch.int32)
    Td[:ld] = dev(T.view(np.int32))
    cd, h1, rec = dev(np.asarray(cands, dtype=np.int32)), marked(count + 3, torch.int32), marked(11, torch.int64)
    check(lib.bmf_panda_core_scan(vp(rd), n, ld, vp(Td), vp(cd), count, mode, float(w_model), float(w_fn), int(w0), int(h0), vp(h1), vp(rec), None),
          "bmf_panda_core_scan")
    torch.cuda.synchronize()
    r0 = rec.cpu().numpy().copy()
    assert words(Td)[:ld].tobytes() == T.tobytes() and not r0[4:8].any()
    if close:
        check(lib.bmf_panda_close(vp(rd), n, ld, -1, vp(rec), vp(Td), None), "bmf_panda_close")
        torch.cuda.synchronize()
    h1, rec, Tn = h1.cpu().numpy(), rec.cpu().numpy(), Td.cpu().numpy()
    assert (h1[count:] == MARK).all() and (rec[8:] == MARK).all() and (Tn[ld:] == MARK).all() and rec[:4].tolist() == r0[:4].tolist()
    assert rd.cpu().numpy().tobytes() == rs_t.tobytes()
    win = int(rec[0])
    assert (rec[1], rec[2]) == ((cands[win], h1[win]) if win >= 0 else (-1, 0))
    return h1[:count], win, int(rec[3]), Tn[:ld].view(np.uint32), int(rec[4])


def device_ext_scan(rs_t, pd_t, n, T, cands, n_t, w_model, w_fp, w_fn, cost_old):
    import torch
    from pybmf_amd._lib import check, lib
    count, ld = len(cands), rs_t.shape[1]
    a, b, rec = marked(count + 3, torch.int32), marked(count + 3, torch.int32), marked(11, torch.int64)
    rd, pdd, Td, cd = dev(rs_t.view(np.int32)), dev(pd_t.view(np.int32)), dev(T.view(np.int32)), dev(np.asarray(cands, dtype=np.int32))
    check(lib.bmf_panda_ext_scan(vp(rd), vp(pdd), n, ld, vp(Td), vp(cd), count, int(n_t), float(w_model), float(w_fp), float(w_fn), float(cost_old),
                                 vp(a), vp(b), vp(rec), None), "bmf_panda_ext_scan")
    torch.cuda.synchronize()
    a, b, rec = a.cpu().numpy(), b.cpu().numpy(), rec.cpu().numpy()
    assert (a[count:] == MARK).all() and (b[count:] == MARK).all() and (rec[8:] == MARK).all() and not rec[4:8].any()
    win = int(rec[0])
    assert tuple(rec[1:4]) == ((cands[win], a[win], b[win]) if win >= 0 else (-1, 0, 0))
    return a[:count], b[:count], win


def device_rows(rs, pd, m, n, I, n_i, T, w_model, w_fp, w_fn, j=None, rec1=None):
    """bmf_panda_rows with column j joining I (or rec[1] = rec1 read on the device); (I after, T after, added, sum d_fn, sum d_fp)."""
    import torch
    from pybmf_amd._lib import check, lib
    ldr, ldt = rs.shape[1], T.size
    Id, Td = marked(ldr + 4, torch.int32), marked(ldt + 4, torch.int32)
    Id[:ldr], Td[:ldt] = dev(I.view(np.int32)), dev(T.view(np.int32))
    work, out, rec = marked(3 * m + 3, torch.int32), marked(7, torch.int64), marked(8, torch.int64)
    rec[1] = -1 if rec1 is None else rec1
    rd, pdd = dev(rs.view(np.int32)), dev(pd.view(np.int32))
    check(lib.bmf_panda_rows(vp(rd), vp(pdd), m, ldr, n, -1 if j is None else j, vp(rec), vp(Id), int(n_i),
                             vp(Td), ldt, float(w_model), float(w_fp), float(w_fn), vp(work), vp(out), None), "bmf_panda_rows")
    torch.cuda.synchronize()
    Id, Td, work, out = Id.cpu().numpy(), Td.cpu().numpy(), work.cpu().numpy(), out.cpu().numpy()
    assert (Id[ldr:] == MARK).all() and (Td[ldt:] == MARK).all() and (work[3 * m:] == MARK).all() and (out[4:] == MARK).all() and out[3] == 0
    return Id[:ldr].view(np.uint32), Td[:ldt].view(np.uint32), int(out[0]), int(out[1]), int(out[2])


def state_after(X):
    """A stand-in engine on X with two rectangles applied: a residual that differs from X and a cover with false positives."""
    ref = NumpyPatternEngine(X)
    for _ in range(2):
        top = np.argsort(row_popcounts(ref.rs[0][: ref.n]), kind="stable")[::-1]
        ref.start_core(int(top[0]))
        ref.set_items([int(c) for c in top[:3]])
        ref.apply_core()
    return ref


def row_sets(ref):
    """(label, T) of the row sets the scans are tried with: a residual column, nothing, every row."""
    top = int(np.argmax(row_popcounts(ref.rs[0][: ref.n])))
    return [("column", ref.rs[0][top].copy()), ("empty", np.zeros(ref.W, dtype=np.uint32)),
            ("full", pack_rows(np.ones((1, ref.m), dtype=bool), ref.W)[0])]


@pytest.mark.parametrize("shape", BOUNDARY)
def test_kernels_at_the_boundary_shapes(shape):
    m, n = shape
    X = planted(m, n, 3, 0.3, 0.03, 2800 + m)
    X[:, n // 2] = 0                                             # an empty column
    ref = state_after(X)
    rs_t, pd_t, rs, pd = ref.bit_matrices()
    assert popcount(pd_t & ~ref.x[0]) > 0 and popcount(rs_t) not in (0, popcount(ref.x[0]))
    rowcount = row_popcounts(rs[:m])
    assert device_couples(rs_t, n, rowcount).tolist() == couples_scores(rs_t, n, rowcount).tolist()
    rng = np.random.RandomState(2810 + n)
    lists = [rng.permutation(n), rng.permutation(n)[: max(1, n // 3)], np.array([n // 2]), np.array([int(rng.randint(n))])]
    tally = {"core": set(), "ext": set(), "rows": set()}         # which of (winner, no winner) / (rows join, none joins) were seen
    for label, T in row_sets(ref):
        n_t = popcount(T)
        for cands in lists:
            for w_model, w_fp, w_fn in WEIGHTS:
                for mode in (0, 1):
                    h1, win, pick = core_scan(rs_t, T, cands, mode, w_model, w_fn, 2, n_t)
                    g_h1, g_win, g_pick, g_T, g_nt = device_core_scan(rs_t, n, T, cands, mode, w_model, w_fn, 2, n_t)
                    assert g_h1.tolist() == h1.tolist() and (g_win, g_pick) == (win, pick), (label, mode)
                    want_T = T & rs_t[cands[win]] if win >= 0 else T
                    assert g_T.tobytes() == want_T.tobytes() and g_nt == popcount(want_T)
                    tally["core"].add((mode, win >= 0))
                for cost_old in (0.0, 3.0 * n_t + 0.5):
                    a, b, win = ext_scan(rs_t, pd_t, T, cands, n_t, w_model, w_fp, w_fn, cost_old)
                    g_a, g_b, g_win = device_ext_scan(rs_t, pd_t, n, T, cands, n_t, w_model, w_fp, w_fn, cost_old)
                    assert g_a.tolist() == a.tolist() and g_b.tolist() == b.tolist() and g_win == win, label
                    tally["ext"].add(win >= 0)
        items = [int(c) for c in lists[0][:4]]
        I0 = pack_rows(np.isin(np.arange(n), items[:-1])[None, :], ref.nvw)[0]
        I1 = pack_rows(np.isin(np.arange(n), items)[None, :], ref.nvw)[0]
        for w_model, w_fp, w_fn in WEIGHTS + [(0.0, 0.5, 1.0)]:
            want_T, added, s_fn, s_fp = rows_pass(rs, pd, m, I1, len(items), T, w_model, w_fp, w_fn)
            tally["rows"].add(added > 0)
            for kw in (dict(j=items[-1]), dict(rec1=items[-1])):
                got = device_rows(rs, pd, m, n, I0, len(items), T, w_model, w_fp, w_fn, **kw)
                assert got[0].tobytes() == I1.tobytes() and got[1].tobytes() == want_T.tobytes() and got[2:] == (added, s_fn, s_fp), label
        got = device_rows(rs, pd, m, n, I0, len(items), T, 1, 1, 1)           # no winner behind the scan: nothing joins, nothing is counted
        assert got[0].tobytes() == I0.tobytes() and got[1].tobytes() == T.tobytes() and got[2:] == (0, 0, 0)
    assert len(tally["core"]) == 4 and len(tally["ext"]) == 2 and len(tally["rows"]) == 2      # winners and none, in both modes


def test_rows_join_somewhere():
    """The row pass of the boundary test is not vacuous: with a cheap model rows do join, and their sums are those of the stand-in."""
    X = planted(65, 129, 3, 0.3, 0.03, 2820)
    ref = NumpyPatternEngine(X)
    rs_t, pd_t, rs, pd = ref.bit_matrices()
    cols = np.argsort(row_popcounts(rs_t[:129]), kind="stable")[::-1][:3]
    I = pack_rows(np.isin(np.arange(129), cols)[None, :], ref.nvw)[0]
    T = rs_t[cols[0]] & rs_t[cols[1]] & rs_t[cols[2]]
    want_T, added, s_fn, s_fp = rows_pass(rs, pd, 65, I, 3, T, 1, 1, 1)
    assert added > 0 and popcount(want_T) == popcount(T) + added
    I0 = pack_rows(np.isin(np.arange(129), cols[:2])[None, :], ref.nvw)[0]
    got = device_rows(rs, pd, 65, 129, I0, 3, T, 1, 1, 1, j=int(cols[2]))
    assert got[1].tobytes() == want_T.tobytes() and got[2:] == (added, s_fn, s_fp)


def test_core_decision_at_the_kink():
    # w_model = w_fn = 1, w0 = 1, h0 = 2: h1 = 1 gives d_cost == 0 and accepts; its neighbour h1 = 0 gives 1 and rejects
    assert core_d_cost(1, 1, 1, 2, 1) == 0 and core_d_cost(1, 1, 1, 2, 0) == 1
    X = np.zeros((70, 5), dtype=np.uint8)
    X[[3, 40], 0] = 1               # T = column 0: rows 3 and 40
    X[[3, 50], 1] = 1               # h1 = 1
    X[[50, 60], 2] = 1              # h1 = 0
    ref = NumpyPatternEngine(X)
    rs_t, T = ref.rs[0], ref.rs[0][0]
    for cands, want in (([1], 0), ([2], -1), ([2, 1], 1), ([2, 3, 4], -1)):
        for mode in (0, 1):
            h1, win, _, g_T, g_nt = device_core_scan(rs_t, 5, T, cands, mode, 1, 1, 1, 2)
            assert core_scan(rs_t, T, cands, mode, 1, 1, 1, 2)[1] == want
            assert win == (want if mode == 0 or cands != [2, 1] else 1), (cands, mode)
            assert g_nt == (1 if win >= 0 else 2) and unpack(g_T, 70).nonzero()[0].tolist() == ([3] if win >= 0 else [3, 40])


def test_extension_decision_at_the_kink():
    # weights 1, |T| = 3, b = 0: a = 2 gives cost_new == cost_old and accepts; a = 1 gives cost_old + 2 and rejects
    X = np.zeros((40, 4), dtype=np.uint8)
    X[[1, 33, 35], 0] = 1           # T
    X[[1, 33], 1] = 1               # a = 2
    X[[35], 2] = 1                  # a = 1
    ref = NumpyPatternEngine(X)
    rs_t, pd_t, T = ref.rs[0], ref.pd[0], ref.rs[0][0].copy()
    for cost_old in (10.0, 0.0, 12345.0):
        for cands, want in (([1], 0), ([2], -1), ([3, 2, 1], 2)):
            a, b, win = device_ext_scan(rs_t, pd_t, 4, T, cands, 3, 1, 1, 1, cost_old)
            assert win == want == ext_scan(rs_t, pd_t, T, cands, 3, 1, 1, 1, cost_old)[2] and not b.any()
    # covered cells are no new false positives: 1 + (3 - b - a) - a with a = 1 is 0 at b = 2 (accepts) and 1 at b = 1 (rejects)
    for rows, want_b, want in (([1, 33], 2, 0), ([1], 1, -1)):
        ref = NumpyPatternEngine(X)
        T = ref.rs[0][0].copy()
        ref.set_items([0, 2])
        ref.T = pack_rows(np.isin(np.arange(40), rows)[None, :], ref.W)[0]    # the factor rows x {0, 2} joins the cover
        ref.apply_core()
        a, b, win = device_ext_scan(ref.rs[0], ref.pd[0], 4, T, [2], 3, 1, 1, 1, 10.0)
        assert (a.tolist(), b.tolist(), win) == ([1], [want_b], want)


def test_row_decision_at_the_kink():
    # weights 1, |I| = 3, no prediction bits: two residual bits give d = 1 + (-2 + 1) = 0 and the row joins; one gives 2
    R = np.zeros((70, 3), dtype=np.uint8)
    R[0], R[1, :2], R[2, :1], R[66, 1:] = 1, 1, 1, 1
    ref = NumpyPatternEngine(R)
    I0 = pack_rows(np.array([[1, 1, 0]], dtype=bool), ref.nvw)[0]
    T0 = pack_rows(np.isin(np.arange(70), [0])[None, :], ref.W)[0]
    I1, T1, added, s_fn, s_fp = device_rows(ref.rs[1], ref.pd[1], 70, 3, I0, 3, T0, 1, 1, 1, j=2)
    assert unpack(I1, 3).all() and unpack(T1, 70).nonzero()[0].tolist() == [0, 1, 66] and (added, s_fn, s_fp) == (2, -4, 2)
    want = rows_pass(ref.rs[1], ref.pd[1], 70, I1, 3, T0, 1, 1, 1)
    assert want[0].tobytes() == T1.tobytes() and want[1:] == (2, -4, 2)
    # a dearer model: d = 1.5 + ... > 0, nobody joins
    assert device_rows(ref.rs[1], ref.pd[1], 70, 3, I0, 3, T0, 1.5, 1, 1, j=2)[2:] == (0, 0, 0)


def test_first_winner_in_list_order_and_correlation_pick():
    X = np.zeros((50, 8), dtype=np.uint8)
    X[:10, 0] = 1                   # T: 10 rows
    X[:10, 6] = 1                   # h1 = 10: d_cost = (2 + 10 - 11) - (20 - 10) < 0
    X[:9, 2] = 1                    # h1 = 9: accepted too
    X[:10, 4] = 1                   # h1 = 10, equal to column 6
    X[20:21, 5] = 1                 # h1 = 0: d_cost = (2 + 0 - 11) - (0 - 10) = 1, rejected
    ref = NumpyPatternEngine(X)
    rs_t, T = ref.rs[0], ref.rs[0][0]
    cands = [5, 6, 2, 4, 7]         # not ascending: the earlier in the list wins, not the lower column
    assert core_d_cost(1, 1, 1, 10, 0) > 0
    h1, win, pick, _, _ = device_core_scan(rs_t, 8, T, cands, 0, 1, 1, 1, 10)
    assert h1.tolist() == [0, 10, 9, 10, 0] and (win, pick) == (1, 1) == core_scan(rs_t, T, cands, 0, 1, 1, 1, 10)[1:]
    h1, win, pick, _, _ = device_core_scan(rs_t, 8, T, [5, 2, 6, 4], 0, 1, 1, 1, 10)
    assert (win, pick) == (1, 1)                                   # column 2 (h1 = 9) stands before the two 10s
    # correlation: the highest score; of the equal ones the LATER position
    h1, win, pick, g_T, g_nt = device_core_scan(rs_t, 8, T, cands, 1, 1, 1, 1, 10)
    assert (win, pick) == (3, 3) == core_scan(rs_t, T, cands, 1, 1, 1, 1, 10)[1:] and g_nt == 10
    h1, win, pick, _, _ = device_core_scan(rs_t, 8, T, [4, 5, 6, 2], 1, 1, 1, 1, 10)
    assert (win, pick) == (2, 2)
    # the pick is rejected: no winner, T stays (w_model = 30: d_cost = 30 (12 - 11) - (20 - 10) = 20)
    h1, win, pick, g_T, g_nt = device_core_scan(rs_t, 8, T, cands, 1, 30, 1, 1, 10)
    assert (win, pick) == (-1, 3) and g_T.tobytes() == T.tobytes() and g_nt == 10
    # extension scan: first winner in list order as well
    a, b, win = device_ext_scan(rs_t, ref.pd[0], 8, T, [5, 4, 6], 10, 1, 1, 1, 100.0)
    assert a.tolist() == [0, 10, 10] and win == 1


def same_fit(a, b):
    assert log_rows(a) == log_rows(b)
    for key in ("U", "V"):
        assert (np.asarray(getattr(a, key).todense()) == np.asarray(getattr(b, key).todense())).all()
    for nm in a._engine.truth:
        assert a._engine.counts(nm) == b._engine.counts(nm)
    for x, y in zip(a._engine.bit_matrices(), b._engine.bit_matrices()):
        assert x[: y.shape[0]].tobytes() == y.tobytes() and not x[y.shape[0]:].any()


@pytest.mark.parametrize("name", CASES)
def test_fit_on_the_device_reproduces_the_reference(name):
    case = load_case(name)
    want = fit_case(case, numpy_engine)
    for block in (None, 1, 7):
        model = fit_case(case, block=block, record=name in STEP_CASES and block is None)
        check_fit(model, case)
        check_state(model._engine, case["X"])
        if model.steps:
            check_steps(model, case)
        same_fit(model, want)


@pytest.mark.parametrize("init_method", ["correlation", "couples-frequency"])
def test_fit_without_a_reference_keeps_the_invariants(init_method):
    X = planted(2049, 300, 5, 0.2, 0.03, 2830)
    case = dict(X=X, k=5, tol=0, w_model=1, w_fp=1, w_fn=1, init_method=init_method, exact_decomp=False)
    model = fit_case(case, record=True)
    eng, rows = model._engine, log_rows(model)
    assert len(rows) == 6 == model.U.shape[1]                      # k + 1
    U, V = eng.factor_arrays()
    assert (U == (np.asarray(model.U.todense()) != 0)).all() and (V == (np.asarray(model.V.todense()) != 0)).all()
    Xb = X != 0
    for f, row in enumerate(rows):
        assert row[0] == description_length(X, U[:, :f + 1], V[:, :f + 1], 1, 1, 1)          # unit weights: exact
        assert [row[1], row[2]] == [int(U[:, f].sum()), int(V[:, f].sum())]
    cores = [s for s in model.steps if s[0] == "core"]
    assert len(cores) == 6
    for f, (_, T, I, E, cost) in enumerate(cores):
        covered = (U[:, :f].astype(np.int64) @ V[:, :f].astype(np.int64).T) > 0
        assert T.any() and (Xb & ~covered)[np.ix_(T, I)].all()       # every core is all ones in the residual it was found on
        assert sorted(E + I) == list(range(300))
    R, P = check_state(eng, X)
    assert (P == ((U.astype(np.int64) @ V.astype(np.int64).T) > 0)).all()
    assert eng.counts("train") == (int((P & Xb).sum()), int((P & ~Xb).sum()), int((~P & Xb).sum()), int((~P & ~Xb).sum()))
