"""GreConD+ on the device: the kernels of csrc/grecondplus.hip against the NumPy stand-in of tests/grecondplus_ref.py step for step,
the engine's rebuild and pruning, and GreConDPlus.fit() against the reference's results (tests/golden/g29_grecondplus.*).

Everything is integers or bit-identical fp64: every comparison is equality (scores as raw fp64 bits), except the ratio columns of
the log (1e-12, inside check_fit, as for GreConD).
"""
import time

import numpy as np
import pytest

from grecondplus_ref import (CASES, OVERLAPPED, NumpyExpansionEngine, check_fit, expansion_ref, fit_case, fit_model, line_counts, load_case,
                             load_overlapped, log_rows, numpy_engine, overlap_prefilter_ref, remove_overlapped_ref, trace_array)
from test_grecond_cpu import pack_rows, popcount, unpack

pytestmark = pytest.mark.gpu


def make_engine(X, RS=None):
    """ExpansionEngine on X; RS (inside X) replaces the residual in both orientations."""
    import torch
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.grecondplus import ExpansionEngine
    eng = ExpansionEngine(BitMatrix(np.ascontiguousarray(X, dtype=np.uint8), "cuda:0"))
    if RS is not None:
        assert not (np.asarray(RS, bool) & ~np.asarray(X, bool)).any()
        rs = np.zeros(tuple(eng.rs.shape), dtype=np.uint32)
        rs[: eng.m] = pack_rows(RS, eng.ldx)
        rs_t = np.zeros(tuple(eng.rs_t.shape), dtype=np.uint32)
        rs_t[: eng.n] = pack_rows(np.asarray(RS).T, eng.W)
        eng.rs.copy_(torch.from_numpy(rs.view(np.int32)))
        eng.rs_t.copy_(torch.from_numpy(rs_t.view(np.int32)))
    return eng


def bits(a):
    return np.array(a, dtype=np.float64).view(np.int64).tolist()


def check_expansion(X, RS, u, v, w_fp, w_fn, label, max_steps=None):
    """One expansion at steps = 1: before every step the device's counters equal the definition's, after it the record holds the
    stand-in's decision, index and both scores bit for bit; then the sets."""
    m, n = X.shape
    u_exp0, v_exp0, trace0, counters0 = expansion_ref(X, RS, u, v, w_fp, w_fn, max_steps=max_steps, with_counters=True)
    eng = make_engine(X, RS)
    eng.set_expansion_state(pack_rows(u[None, :], eng.W)[0], pack_rows(v[None, :], eng.nvw)[0])
    rows, cols = eng.counters()
    a, b, c = line_counts(X, RS, v)
    assert rows.tolist() == [a.tolist(), b.tolist(), c.tolist()]                     # the counts pass against the set definition
    a, b, c = line_counts(X.T, RS.T, u)
    assert cols.tolist() == [a.tolist(), b.tolist(), c.tolist()]
    for step, (want, (rows0, cols0)) in enumerate(zip(trace0, counters0)):
        rows, cols = eng.counters()
        assert rows.tolist() == rows0.tolist() and cols.tolist() == cols0.tolist(), step
        eng.launch_steps(w_fp, w_fn, 1)
        joins, stopped, trace = eng.read_record()
        assert len(trace) == step + 1 and stopped == (want[0] == -1) and joins == sum(t[0] >= 0 for t in trace0[: step + 1])
        assert trace[step][:2] == want[:2] and bits(trace[step][2:]) == bits(want[2:]), (step, trace[step], want)
    su, sue, sv, sve = eng.sets()
    assert unpack(sue, m).tolist() == u_exp0.tolist() and unpack(sve, n).tolist() == v_exp0.tolist()
    assert unpack(su, m).tolist() == (u | u_exp0).tolist() and unpack(sv, n).tolist() == (v | v_exp0).tolist()
    assert popcount(su) == int((u | u_exp0).sum()) and popcount(sv) == int((v | v_exp0).sum())          # padding bits stay zero
    if trace0[-1][0] == -1:
        before = eng._rec.cpu().numpy().tobytes(), eng._sets.cpu().numpy().tobytes()
        eng.launch_steps(w_fp, w_fn, 5)                                               # a launch after the stop is a no-op
        assert (eng._rec.cpu().numpy().tobytes(), eng._sets.cpu().numpy().tobytes()) == before
    n_row, n_col = sum(t[0] == 1 for t in trace0), sum(t[0] == 0 for t in trace0)
    print(f"grecondplus expansion {label}: {len(trace0)} steps ({n_row} rows, {n_col} columns joined), last scores {trace0[-1][2:]}")
    return trace0


def random_state(m, n, seed, density=0.35):
    """X with duplicated rows and columns (the first index decides among equal scores), a residual inside it, a small rectangle."""
    rng = np.random.RandomState(seed)
    X = rng.rand(m, n) < density
    r0, c0 = rng.choice(m, max(m // 6, 4), replace=False), rng.choice(n, max(n // 6, 4), replace=False)
    X[np.ix_(r0, c0)] |= rng.rand(r0.size, c0.size) < 0.6           # a dense block for the expansion to grow into
    RS = X & (rng.rand(m, n) < 0.4)
    for src, dst in ((3, 7), (3, m - 1), (10, 5)):                   # equal rows, one of them BEFORE its twin
        X[dst], RS[dst] = X[src], RS[src]
    for src, dst in ((2, 9), (2, n - 1), (11, 4)):
        X[:, dst], RS[:, dst] = X[:, src], RS[:, src]
    u, v = np.zeros(m, bool), np.zeros(n, bool)
    u[r0[:3]], v[c0[:12]] = True, True                               # far more columns than rows: the best scores of the two axes differ
    return X, RS, u, v


# 33 x 65 and 96 x 72: the fixture shapes.  257 x 130: m no multiple of 32, n no multiple of 64.  40 x 8300: rows of 272 words, so the
# 64 lanes of a wave in the counts pass take a second round of 16-byte loads.  3001 x 1537: the counts pass puts 4 lines in a workgroup
# (751 and 385 workgroups), and in the one workgroup of 1024 threads that steps every thread holds 2 or 3 rows and 1 or 2 columns, so the
# argmax crosses lanes, waves and the per-thread loop, and the last partial round of both axes is exercised.
@pytest.mark.parametrize("m,n,max_steps", [(33, 65, None), (96, 72, None), (257, 130, None), (40, 8300, 12), (3001, 1537, 12)])
@pytest.mark.parametrize("w_fp,w_fn", [(0.5, 0.5), (0.3, 0.7)])
def test_counts_and_steps_follow_the_stand_in(m, n, max_steps, w_fp, w_fn):
    X, RS, u, v = random_state(m, n, 1000 * m + n)
    trace = check_expansion(X, RS, u, v, w_fp, w_fn, f"{m}x{n} w=({w_fp}, {w_fn})", max_steps)
    assert len(trace) >= (9 if w_fp == 0.3 else 1)                    # with 0.3 / 0.7 every shape runs through joins on both axes


@pytest.mark.parametrize("m,n", [(33, 65), (257, 130)])
@pytest.mark.parametrize("w_fp,w_fn", [(0.5, 0.5), (0.3, 0.7)])
def test_edge_states(m, n, w_fp, w_fn):
    X, RS, u, v = random_state(m, n, 7 * m + n)
    # u of all rows: every row scores 0.0 (r_index 0), only columns can join
    trace = check_expansion(X, RS, np.ones(m, bool), v, w_fp, w_fn, f"{m}x{n} all rows")
    assert all(t[0] != 1 and t[2] == 0.0 for t in trace)
    # an empty residual: everything is covered already, a = 0 on every line
    trace = check_expansion(X, np.zeros_like(X), u, v, w_fp, w_fn, f"{m}x{n} empty residual")
    assert len(trace) >= 2
    # nothing covered yet (RS = X): b = a on every line outside the sets, no score above 0, the first step stops
    trace = check_expansion(X, X.copy(), u, v, w_fp, w_fn, f"{m}x{n} nothing covered")
    assert len(trace) == 1 and trace[0][0] == -1 and trace[0][2] <= 0 and trace[0][3] <= 0
    # empty X
    Z = np.zeros((m, n), bool)
    trace = check_expansion(Z, Z, u, v, w_fp, w_fn, f"{m}x{n} zeros")
    assert len(trace) == 1


@pytest.mark.parametrize("k", [33, 257])
@pytest.mark.parametrize("w_fp,w_fn", [(0.5, 0.5), (0.3, 0.7)])
def test_equal_positive_scores_stop(k, w_fp, w_fn):
    """A symmetric X with a symmetric residual and u = v: the row and column scores are the same numbers, so the best of each are equal;
    they are positive, and the expansion stops at once."""
    rng = np.random.RandomState(k)
    S = rng.rand(k, k) < 0.8
    X = S | S.T
    M = rng.rand(k, k) < 0.2
    RS = X & (M | M.T)
    u = np.zeros(k, bool)
    u[[1, 4, 6, 9, 12]] = True
    trace = check_expansion(X, RS, u, u.copy(), w_fp, w_fn, f"{k}x{k} symmetric")
    assert len(trace) == 1 and trace[0][0] == -1 and trace[0][2] == trace[0][3] > 0


def test_step_budgets_give_the_same_expansion():
    case = load_case("c")
    X = case["X"] != 0
    rng = np.random.RandomState(3)
    RS = X & (rng.rand(*X.shape) < 0.5)
    u, v = np.zeros(X.shape[0], bool), np.zeros(X.shape[1], bool)
    u[:5], v[:4] = True, True
    u_exp0, v_exp0, trace0 = expansion_ref(X, RS, u, v, 0.3, 0.7)
    assert len(trace0) >= 20
    eng = make_engine(X, RS)
    pu, pv = pack_rows(u[None, :], eng.W)[0], pack_rows(v[None, :], eng.nvw)[0]
    outs = []
    for steps, reads in ((1, len(trace0)), (7, -(-len(trace0) // 7)), (None, 1)):
        ue, ve, n_iter = eng.expand(pu, pv, 0.3, 0.7, steps=steps)
        assert eng.host_reads == reads and n_iter == len(trace0)
        outs.append((ue.tobytes(), ve.tobytes(), eng._rec.cpu().numpy().tobytes(), eng._row_abc.cpu().numpy().tobytes(),
                     eng._col_abc.cpu().numpy().tobytes()))
        assert unpack(ue, eng.m).tolist() == u_exp0.tolist() and unpack(ve, eng.n).tolist() == v_exp0.tolist()
        assert [t[:2] for t in eng.trace] == [t[:2] for t in trace0] and bits([t[2:] for t in eng.trace]) == bits([t[2:] for t in trace0])
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.parametrize("m,n", [(257, 130), (600, 530)])
def test_rebuild_after_dropping_factors(m, n):
    rng = np.random.RandomState(m + n)
    f = 40
    U, V = rng.rand(m, f) < 0.08, rng.rand(n, f) < 0.08
    U[:, 5], V[:, 6] = False, False                                   # a factor without rows, one without columns
    X = ((U.astype(np.float64) @ V.T.astype(np.float64)) > 0) & (rng.rand(m, n) < 0.9) | (rng.rand(m, n) < 0.05)
    eng, ref = make_engine(X), NumpyExpansionEngine(X)
    Ub, Vb = pack_rows(U.T, eng.W), pack_rows(V.T, eng.nvw)
    keep_sets = [np.arange(f), np.sort(rng.choice(f, 25, replace=False)), np.array([7]), np.arange(0)]
    for keep in keep_sets:                                            # all 40, then 25 of them: the prediction shrinks
        eng.rebuild(Ub[keep], Vb[keep])
        ref.rebuild(Ub[keep], Vb[keep])
        pd = (U[:, keep].astype(np.float64) @ V[:, keep].T.astype(np.float64)) > 0
        rs = X & ~pd
        assert eng.pd_t.cpu().numpy().view(np.uint32)[:n].tobytes() == pack_rows(pd.T, eng.W).tobytes() == ref.pd_t.tobytes()
        assert eng.rs_t.cpu().numpy().view(np.uint32)[:n].tobytes() == pack_rows(rs.T, eng.W).tobytes() == ref.rs_t.tobytes()
        assert eng.rs.cpu().numpy().view(np.uint32)[:m].tobytes() == pack_rows(rs, eng.ldx).tobytes()
        assert not eng.pd_t.cpu().numpy()[n:].any() and not eng.rs_t.cpu().numpy()[n:].any() and not eng.rs.cpu().numpy()[m:].any()
        assert eng._col_host.tolist() == rs.sum(axis=0).tolist() and eng.residual_sum() == int(rs.sum()) == ref.residual_sum()
        assert eng.residual_columns().tolist() == np.nonzero(rs.sum(axis=0))[0].tolist()
        assert eng.counts("train") == ref.counts("train") and len(eng._factors) == len(keep)
        if len(keep) in (25, 0):
            s0, u0, v0 = ref.concept()
            s1, u1, v1 = eng.concept()
            assert s1 == s0 > 0 and u1.tobytes() == u0.tobytes() and v1.tobytes() == v0.tobytes()
    with pytest.raises(NotImplementedError, match="rebuild"):
        eng.apply(Ub[0], Vb[0])


def device_prune(X, U, V, Ue, Ve):
    eng = make_engine(X)
    out = eng.prune_overlapped(pack_rows(U.T, eng.W), pack_rows(V.T, eng.nvw), pack_rows(Ue.T, eng.W), pack_rows(Ve.T, eng.nvw))
    dense = [np.array([unpack(r, length) for r in A], dtype=np.uint8).reshape(len(A), length).T
             for A, length in zip(out, (eng.m, eng.n, eng.m, eng.n))]
    for A, words in zip(out, (eng.W, eng.nvw, eng.W, eng.nvw)):
        assert A.shape == (U.shape[1], words)
    assert [popcount(A) for A in out] == [int(D.sum()) for D in dense]          # padding bits stay zero
    return dense, eng.pruned


@pytest.mark.parametrize("name", OVERLAPPED)
def test_pruning_on_the_constructed_states(name):
    s = load_overlapped(name)
    got, pruned = device_prune(s["X"], s["U0"], s["V0"], s["Ue0"], s["Ve0"])
    for g, key in zip(got, ("U1", "V1", "Ue1", "Ve1")):
        assert g.tolist() == s[key].tolist(), key
    passed = overlap_prefilter_ref(s["X"], s["U0"], s["V0"], s["Ue0"], s["Ve0"])
    assert pruned == (passed, s["rows_removed"], s["columns_removed"])
    assert (passed > 0) == (name in ("row", "column", "stale", "twice", "single"))


@pytest.mark.parametrize("m,n", [(70, 45), (130, 257)])
def test_pruning_on_overlapping_factors(m, n):
    """Overlapping rectangles of ones with random extension marks: rows and columns do leave, over more columns than a wave has lanes."""
    rng = np.random.RandomState(m)
    f = 12
    U, V = rng.rand(m, f) < 0.45, rng.rand(n, f) < 0.45
    X = (U.astype(np.float64) @ V.T.astype(np.float64)) > 0
    X &= rng.rand(m, n) < 0.999                                       # a few zeros under the factors
    Ue, Ve = U & (rng.rand(m, f) < 0.5), V & (rng.rand(n, f) < 0.5)
    want = remove_overlapped_ref(X, U, V, Ue, Ve)
    got, pruned = device_prune(X, U.astype(np.uint8), V.astype(np.uint8), Ue.astype(np.uint8), Ve.astype(np.uint8))
    for g, w in zip(got, want):
        assert g.tolist() == w.tolist()
    rows, cols = int(Ue.sum() - want[2].sum()), int(Ve.sum() - want[3].sum())
    print(f"grecondplus pruning {m}x{n}: {pruned[0]} pairs pass the subset test, {rows} rows and {cols} columns leave")
    assert pruned == (overlap_prefilter_ref(X, U, V, Ue, Ve), rows, cols) and rows >= 1 and cols >= 1


@pytest.mark.parametrize("name", CASES)
def test_fit_reproduces_the_reference(name):
    from pybmf_amd.grecondplus import ExpansionEngine
    case = load_case(name)
    t0 = time.time()
    model = fit_case(case)
    wall = time.time() - t0
    print(f"grecondplus fit {name}: {len(log_rows(model))} rows, {model.U.shape[1]} factors, steps {sum(model.n_steps)}, {wall:.2f} s")
    assert isinstance(model._engine, ExpansionEngine)
    check_fit(model, case)
    if name == "g":
        assert model._engine.counts("val")[0] + model._engine.counts("val")[2] == int(case["X_val"].sum())


@pytest.mark.parametrize("name,steps,block", [("c", 1, None), ("c", 7, 5), ("d", 3, 1)])
def test_fit_with_step_budgets(name, steps, block):
    case = load_case(name)
    check_fit(fit_case(case, steps=steps, block=block), case)


def test_larger_fit_against_the_stand_in():
    """600 x 400, 6 planted factors, 0.03 % flips, k = None, w_fp = 0.3: 67 log rows, 58 factors left, 9 swallowed by later ones,
    expansions of up to 147 steps (the stand-in takes about 8 s on the host)."""
    rng = np.random.RandomState(77)
    U, V = rng.rand(600, 6) < 0.1, rng.rand(400, 6) < 0.1
    X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(600, 400) < 0.0003)).astype(np.uint8)
    params = dict(k=None, tol=0, w_fp=0.3, w_fn=None)
    t0 = time.time()
    ref = fit_model(X, params, numpy_engine)
    t1 = time.time()
    model = fit_model(X, params)
    t2 = time.time()
    print(f"grecondplus 600x400: {len(log_rows(ref))} rows, {ref.U.shape[1]} factors, {sum(ref.n_covered)} covered, longest expansion "
          f"{max(ref.n_steps)}, stand-in {t1 - t0:.1f} s, device {t2 - t1:.2f} s")
    assert len(log_rows(ref)) > 50 and sum(ref.n_covered) >= 5 and max(ref.n_steps) > 100
    assert [r[:4] for r in log_rows(model)] == [r[:4] for r in log_rows(ref)]
    assert np.abs(np.array([r[4:] for r in log_rows(model)]) - np.array([r[4:] for r in log_rows(ref)])).max() <= 1e-12
    for name in ("U", "V", "U_exp", "V_exp"):
        assert (getattr(model, name) != getattr(ref, name)).nnz == 0 and getattr(model, name).shape == getattr(ref, name).shape
    assert trace_array(model.traces).tobytes() == trace_array(ref.traces).tobytes()
    assert model.n_steps == ref.n_steps and model.n_covered == ref.n_covered and model.n_pruned == ref.n_pruned
    assert model._engine.counts("train") == ref._engine.counts("train")
    assert (model.X_pd != ref.X_pd).nnz == 0
