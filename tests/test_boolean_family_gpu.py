"""The four bit-set models on the device against their NumPy stand-ins on the edge-case family of tests/boolean_family.py, constructed
exact ties at kernel level, and the branches of csrc/asso_refine.hip and of the GreConD scan that no other test reaches.

Everything compared is integers or bits (==), except the one float that is a sum over rows -- the score -- which is compared by the
project's rule (check_score): == for weights whose products with the counts are exact, within 1e-12 relative otherwise.  Every tie test
first asserts, on the host, that its input does contain ties.  The largest shapes are 2049 x 20 and 20 x 2049 (one row search runs on
3 x 54785: the narrowest matrix at which that kernel chunks on its own).
"""
import functools

import numpy as np
import pytest

import boolean_family as F
import test_asso_cpu as A
import test_asso_gpu as AG
import test_asso_refine_gpu as RG
import test_grecond_cpu as G
import test_grecond_gpu as GG

pytestmark = pytest.mark.gpu


# ---- C1: whole fits, device against stand-in ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stand_in(kind, name, params):
    """The stand-in's snapshot of one fit, computed once per (model, case, parameter set)."""
    p = dict(params)
    if kind == "GreConD":
        return F.snapshot(F.fit_grecond(name, **p), kind)
    if kind == "Asso":
        return F.snapshot(F.fit_asso(name, **p), kind)
    return F.snapshot(F.fit_refine(name, kind, **p), kind)


def frozen(p):
    return tuple(sorted(p.items(), key=lambda kv: kv[0]))


@pytest.mark.parametrize("name", F.CASES)
def test_grecond_fit_on_device_equals_the_stand_in(name):
    from pybmf_amd.grecond import ConceptEngine
    by_k = {}
    for p in F.grecond_grid(name):
        model = F.fit_grecond(name, device=True, **p)
        assert isinstance(model._engine, ConceptEngine)
        snap = F.snapshot(model, "GreConD")
        F.assert_same_fit(snap, stand_in("GreConD", name, frozen(p)), True)
        F.assert_same_fit(snap, by_k.setdefault(p["k"], snap), True)          # the block size does not change the result
    assert set(F.family()[name].get(key) is not None for key in ("X_val", "X_test")) == {name == "split"}
    assert set(snap["counts"]) == ({"train", "val", "test"} if name == "split" else {"train"})


@pytest.mark.parametrize("name", F.CASES)
def test_asso_fit_on_device_equals_the_stand_in(name):
    from pybmf_amd.asso import AssoEngine
    first = {}
    for p in F.asso_grid(name):
        model = F.fit_asso(name, device=True, **p)
        assert isinstance(model._engine, AssoEngine)
        snap = F.snapshot(model, "Asso")
        F.assert_same_fit(snap, stand_in("Asso", name, frozen(p)), F.exact_weights(p["w_fp"], p["w_fn"]))
        F.assert_same_fit(snap, first.setdefault((p["tau"], p["w_fp"], p["w_fn"]), snap), True)
    assert set(snap["counts"]) == ({"train", "val", "test"} if name == "split" else {"train"})


@pytest.mark.parametrize("name", F.CASES)
def test_refiner_fits_on_device_equal_the_stand_in(name):
    from pybmf_amd.asso_refine import AssoRefineEngine
    for kind in ("AssoIter", "AssoOpt"):
        for p in F.refine_grid(name):
            model = F.fit_refine(name, kind, device=True, **p)
            assert isinstance(model._engine, AssoRefineEngine)
            snap = F.snapshot(model, kind)
            F.assert_same_fit(snap, stand_in(kind, name, frozen(p)), F.exact_weights(p["w_fp"], p["w_fn"]))
    assert set(snap["counts"]) == ({"train", "val", "test"} if name == "split" else {"train"})


# ---- C2: constructed ties ---------------------------------------------------------------------------------------------------
def tie_matrix():
    """70 x 45 with planted structure, and columns built so that C[0][j] / C[0][0] is exactly 1/2, 1/4 and 1/3 (column 0 has 12 ones,
    of which columns 1, 2, 3 share 6, 3 and 4), and columns 5, 9 and 20 equal."""
    X = F.planted(70, 45, 3, 0.3, 0.02, 2640).astype(bool)
    X[:, :4] = False
    X[:12, 0] = True
    X[:6, 1], X[:3, 2], X[:4, 3] = True, True, True
    X[20:30, 1], X[30:33, 2], X[40:48, 3] = True, True, True
    X[:, 9], X[:, 20] = X[:, 5], X[:, 5]
    return X.astype(np.uint8)


def test_asso_basis_on_the_boundary_of_tau():
    X = tie_matrix()
    Xi = X.astype(np.int64)
    Cm = Xi.T @ Xi
    s = np.diag(Cm).astype(np.float64)
    assert [Cm[0, j] for j in range(4)] == [12, 6, 3, 4] and (s == 0).any()      # (an empty column: no candidate, whatever tau)
    eng, ref = AG.device_engine(X), A.NumpyAssoEngine(X)
    for tau in (0.5, 0.25, 1 / 3):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = Cm.astype(np.float64) / s[:, None]
        on_boundary = ratio == tau
        assert on_boundary.sum() >= 1 and on_boundary[0].any()          # the input holds cells exactly on tau
        want = (ratio > tau) & (s[:, None] > 0)                         # NumPy's fp64 >: a cell on the boundary is off
        assert not want[on_boundary].any()
        count = eng.build_basis(tau)
        got = eng.basis_rows() != 0
        assert not got[on_boundary].any()
        assert (got == want).all() and count == int(want.any(axis=1).sum()) == ref.build_basis(tau)
        assert eng.basis.cpu().numpy().view(np.uint32).tobytes() == ref.basis.tobytes()


@pytest.mark.parametrize("w", [0.5, 1.0])
def test_asso_row_decision_on_equal_gain_and_loss(w):
    """w_fp == w_fn: a candidate that adds as many false as true positives to a row leaves the row's score where it was; the row does
    not take it (strict >), in the sweep's sums (launch_score) and in the column vector (column)."""
    X = tie_matrix()
    rng = np.random.RandomState(2641)
    pd = (rng.rand(*X.shape) < 0.2).astype(np.uint8)
    eng, ref = AG.device_engine(X), A.NumpyAssoEngine(X)
    assert eng.build_basis(0.3) == ref.build_basis(0.3)
    eng.load_prediction(pd)
    ref.load_prediction(pd)
    cands = ref.list.copy()
    B = ref.basis_rows().astype(np.int64)[cands]                        # (candidates, n)
    free = (1 - pd.astype(np.int64))
    a = (X.astype(np.int64) * free) @ B.T                               # true positives a candidate adds to a row
    c = free @ B.T - a                                                  # false positives
    tied = (a == c)                                                     # (rows, candidates): the score does not move
    assert (tied & (a > 0)).sum() > 0 and (a > c).sum() > 0 and (a < c).sum() > 0
    T, Fp, score, rec, vectors = AG.sweep_both(eng, ref, cands, 0.0, w, w)
    assert (vectors == (a > c).T).all() and not vectors[tied.T].any()     # the stand-in's fp64 decision is the integer one
    tp0, fp0 = ref.row_counts()
    assert T.tolist() == (tp0[:, None] + np.where(a > c, a, 0)).sum(axis=0).tolist()
    assert Fp.tolist() == (fp0[:, None] + np.where(a > c, c, 0)).sum(axis=0).tolist()
    for i in np.nonzero((tied & (a > 0)).any(axis=0))[0][:6]:
        u, v = eng.column(int(cands[i]), w, w)
        assert A.unpack(u, eng.m).tolist() == (a[:, i] > c[:, i]).tolist() and v.tobytes() == ref.basis[cands[i]].tobytes()


def test_asso_pick_takes_the_first_of_equal_candidates():
    X = tie_matrix()
    eng, ref = AG.device_engine(X), A.NumpyAssoEngine(X)
    assert eng.build_basis(0.5) == ref.build_basis(0.5)
    assert ref.basis[5].tobytes() == ref.basis[9].tobytes() == ref.basis[20].tobytes() and {5, 9, 20} <= set(ref.list.tolist())
    for w_fp, w_fn in ((0.5, 0.5), (1.0, 1.0)):
        for cands in (ref.list.copy(), ref.list[::-1].copy()):
            T, Fp, score, rec, _ = AG.sweep_both(eng, ref, cands, 0.0, w_fp, w_fn)
            top = score.max()
            tied = np.nonzero(score == top)[0]
            assert tied.size >= 2 and top > 0                           # the input holds a tie for the largest score
            assert rec[0] == tied[0] == int(np.argmax(score)) and rec[1] == cands[tied[0]]
            assert (T[tied] == T[tied[0]]).all() and (Fp[tied] == Fp[tied[0]]).all()
            # the top score itself as best_score: nothing exceeds it
            _, _, _, rec, _ = AG.sweep_both(eng, ref, cands, float(top), w_fp, w_fn)
            assert rec[0] == -1 and rec[1] == -1
            for block in (None, 1, 7):
                eng.set_list(cands)
                ref.set_list(cands)
                hit = eng.best(0.0, w_fp, w_fn, block=block)
                assert hit == ref.best(0.0, w_fp, w_fn, block=block) and hit[:2] == (int(tied[0]), int(cands[tied[0]]))
                assert eng.best(float(top), w_fp, w_fn, block=block) is None


def test_grecond_pick_takes_the_first_of_equal_candidates():
    X = tie_matrix()

    def fresh():
        return G.NumpyConceptEngine(X)
    ref = fresh()
    full = np.arange(X.shape[1])
    for cands in (full, full[::-1].copy()):
        s0, _, _, _ = G.scan_block(ref.Xt, ref.rs_t, ref.n, ref.all_rows, cands, 0)
        top = int(s0.max())
        tied = np.nonzero(s0 == top)[0]
        assert tied.size >= 2 and top > 0                               # the input holds a tie for the largest score
        _, _, _, first = G.scan_block(ref.Xt, ref.rs_t, ref.n, ref.all_rows, cands, top - 1)
        assert first == tied[0]
        _, _, _, rec = GG.device_scan(ref, ref.all_rows, cands, top - 1)
        assert rec.tolist() == [int(tied[0]), int(cands[tied[0]]), top] + rec.tolist()[3:] and rec[1] in (5, 9, 20)
        _, _, _, rec = GG.device_scan(ref, ref.all_rows, cands, top)      # best_score equal to the top score: no winner
        assert rec.tolist() == [-1, -1, 0, 0, 0]
        GG.check_point(fresh(), ref.all_rows, cands, top - 1, "ties, one below the top")
        GG.check_point(fresh(), ref.all_rows, cands, top, "ties, at the top")
        GG.check_point(fresh(), ref.all_rows, cands, 0, "ties, first above zero")


@pytest.mark.parametrize("w", [0.5, 1.0])
def test_assoiter_visit_drops_a_factor_that_changes_nothing_or_ties(w):
    rng = np.random.RandomState(2642)
    m, n, k, kc = 70, 45, 5, 2
    V = rng.rand(n, k) < 0.25
    V[:, kc] = np.arange(n) < 10                    # 10 cells
    V[:, 4] |= V[:, kc]                             # factor 4 covers factor kc
    U = rng.rand(m, k) < 0.3
    X = ((U.astype(int) @ V.T.astype(int)) > 0) ^ (rng.rand(m, n) < 0.05)
    U[:10, 4], U[:10, kc] = True, True              # rows 0-9: V[kc] lies inside what they hold already; their bit is 1 now
    U[10:20] = False
    U[10:20, kc] = True                             # rows 10-19 hold factor kc alone ...
    X[10:20, :10] = np.arange(10)[None, :] < 5      # ... and it brings them 5 true and 5 false positives
    others = [l for l in range(k) if l != kc]
    old = (U[:, others].astype(int) @ V[:, others].T.astype(int)) > 0
    new = old | V[:, kc][None, :]
    gain, loss = ((new & ~old) & X).sum(axis=1), ((new & ~old) & ~X).sum(axis=1)
    nothing, equal = (gain + loss == 0), (gain == loss) & (gain > 0)
    assert nothing[:10].all() and equal[10:20].all() and (gain[10:20] == 5).all() and (gain > loss).any() and (gain < loss).any()
    assert U[nothing | equal, kc].sum() >= 20       # bits that are 1 before the visit and must come out 0
    eng = RG.device_engine(X, U, V)
    Uh = U.copy()
    RG.visit_both(eng, X, Uh, V, kc, w, w)
    column = eng.column()
    assert not column[nothing | equal].any() and column.tolist() == (gain > loss).tolist()
    assert (eng.factor_arrays()[0][:, kc] != 0).tolist() == (gain > loss).tolist()


def test_faststep_counts_on_the_boundary_of_tau():
    """Integer factors and an integer tau: every S is exact on both sides, so the counts and the prediction are NumPy's S > tau."""
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.faststep import FastStepEngine
    rng = np.random.RandomState(2643)
    m, n, k = 70, 45, 17                            # 17: the second 16-column step of the base kernel holds one column
    U, V = rng.randint(0, 3, (m, k)).astype(np.float64), rng.randint(0, 3, (n, k)).astype(np.float64)
    X = (rng.rand(m, n) < 0.5).astype(np.uint8)
    S = U @ V.T
    assert (S == np.round(S)).all()
    tau = float(int(np.median(S)))
    on_boundary = int((S == tau).sum())
    assert on_boundary > 0 and (S > tau).any() and (S < tau).any()
    pd = S > tau
    want = (int((pd & (X == 1)).sum()), int((pd & (X == 0)).sum()))
    eng = FastStepEngine(BitMatrix(X, "cuda:0"), k, tau, U, V)
    for col in (0, k // 2, k - 1):
        eng.set_factor(col)
        for grad in (False, True):
            _, _, _, tp, fp = eng.evaluate(U[:, col], V[:, col], grad, True)
            print(f"faststep ties, skip {col}, grad {grad}: TP/FP {tp}/{fp}, NumPy {want[0]}/{want[1]}, {on_boundary} cells with S == tau")
            assert (tp, fp) == want
    assert (np.asarray(eng.prediction().todense()) != 0).tolist() == pd.tolist()


# ---- C3: the branches of asso_refine.hip that no other test reaches -------------------------------------------------------------
def check_state(eng, X, U, V):
    """The engine's factors, prediction and counts against the host's U, V; mask bits past k are zero."""
    k = V.shape[1]
    Ue, Ve = eng.factor_arrays()
    assert (Ue != 0).tolist() == U.tolist() and (Ve != 0).tolist() == V.tolist()
    P = (U.astype(np.int64) @ V.T.astype(np.int64)) > 0
    assert (np.asarray(eng.prediction().todense()) != 0).tolist() == P.tolist()
    tp, fp = int((X & P).sum()), int((~X & P).sum())
    assert eng.counts("train") == (tp, fp, int(X.sum()) - tp, X.size - int(X.sum()) - fp)
    masks = np.unpackbits(eng.U.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert masks.shape[1] == -(-k // 32) * 32 and not masks[:, k:].any()


def dense_case(m, n, k, seed, u_density=0.5):
    rng = np.random.RandomState(seed)
    U, V = rng.rand(m, k) < u_density, rng.rand(n, k) < 1.5 / k
    X = ((rng.rand(m, 3) < 0.4).astype(int) @ (rng.rand(n, 3) < 0.4).astype(int).T > 0) ^ (rng.rand(m, n) < 0.05)
    return X, U, V


@pytest.mark.parametrize("k,cols", [(32, (0, 31)), (64, (0, 31, 32, 63)), (96, (0, 31, 32, 63, 64, 95))])
@pytest.mark.parametrize("w_fp,w_fn", [(0.5, 0.5), (0.3, 0.7)])
def test_column_kernel_with_k_a_multiple_of_32(k, cols, w_fp, w_fn):
    """The last mask word is all factors; with 96, kc = 32 .. 63 sits in the middle word of three.  Half of every mask is set, so the
    inner loop over a mask's bits runs long."""
    X, U, V = dense_case(70, 45, k, 2650 + k)
    assert U[:, -1].any() and U.sum(axis=1).min() >= 8
    eng = RG.device_engine(X, U, V)
    assert eng.kw == k // 32
    for kc in cols + cols[:1]:
        RG.visit_both(eng, X, U, V, kc, w_fp, w_fn)
    check_state(eng, X, U, V)


@pytest.mark.parametrize("m", [1, 31, 32, 33])
def test_column_kernel_at_row_counts_around_a_word(m):
    X, U, V = RG.random_case(m, 45, 5, 2660 + m)
    for w_fp, w_fn in ((0.5, 0.5), (0.3, 0.7)):
        eng, Uh = RG.device_engine(X, U, V), U.copy()
        for kc in (0, 4, 2, 0):
            RG.visit_both(eng, X, Uh, V, kc, w_fp, w_fn)
        assert eng._u.numel() == -(-m // 32) and eng.column().size == m
        check_state(eng, X, Uh, V)


@pytest.mark.parametrize("fill", ["all", "none"])
def test_column_kernel_with_full_and_empty_masks_and_factors(fill):
    X, _, V = dense_case(70, 45, 40, 2670)
    V[:, 3], V[:, 37] = False, True                 # an empty factor and a full one
    U = np.ones((70, 40), dtype=bool) if fill == "all" else np.zeros((70, 40), dtype=bool)
    for w_fp, w_fn in ((0.5, 0.5), (0.0, 1.0)):
        eng, Uh = RG.device_engine(X, U, V), U.copy()
        for kc in (3, 37, 0, 39, 32, 37):
            RG.visit_both(eng, X, Uh, V, kc, w_fp, w_fn)
            assert not Uh[:, 3].any()               # the empty factor changes nothing: no row takes it (strict >)
        check_state(eng, X, Uh, V)


@pytest.mark.parametrize("k,want_chunk", [(800, 12), (1024, 8)])
def test_column_kernel_chunks_on_its_own(k, want_chunk):
    from pybmf_amd._lib import lib
    m, n = 40, 45
    X, U, V = RG.random_case(m, n, k, 2680 + k, density=0.1)
    U[:, -1] = np.arange(m) % 2 == 0
    eng = RG.device_engine(X, U, V)
    assert eng.ldx == 16 and lib.bmf_asso_refine_chunk(k, eng.ldx, 0) == want_chunk < eng.ldx      # chunk=None walks over n in pieces
    forced = RG.device_engine(X, U, V)
    Uh = U.copy()
    for kc in (0, k // 2, k - 1):
        got = RG.visit_both(eng, X, Uh, V, kc, 0.3, 0.7, chunk=None)
        assert forced.refine_column(kc, 0.3, 0.7, chunk=4) == got          # a forced chunk from the same state: the same bytes
        assert forced.U.cpu().numpy().tobytes() == eng.U.cpu().numpy().tobytes()
        assert forced._u.cpu().numpy().tobytes() == eng._u.cpu().numpy().tobytes()
    check_state(eng, X, Uh, V)


def test_column_kernel_refuses_k_1025():
    rng = np.random.RandomState(2690)
    X = rng.rand(40, 45) < 0.3
    eng = RG.device_engine(X, rng.rand(40, 1025) < 0.01, rng.rand(45, 1025) < 0.1)
    with pytest.raises(NotImplementedError, match="k <= 1024"):
        eng.refine_column(0, 0.5, 0.5)


@pytest.mark.parametrize("k", [3, 4, 5])
@pytest.mark.parametrize("w_fp,w_fn", [(1.0, 1.0), (0.3, 0.7)])
def test_row_search_with_few_factors(k, w_fp, w_fn):
    """k = 4: one thread, no thread bits; 3: fewer leaves than a thread walks; 5: the first thread bit."""
    X, U, V = RG.random_case(40, 30, k, 300 + k, density=0.15)
    RG.search_both(X, U, V, w_fp, w_fn)


def test_row_search_chunks_on_its_own():
    from pybmf_amd._lib import lib
    k, m = 8, 3
    ldx = 16
    while lib.bmf_asso_refine_chunk(k, ldx, 1) == ldx:
        ldx += 16
        assert ldx < 1 << 16
    chunk = lib.bmf_asso_refine_chunk(k, ldx, 1)
    n = (ldx - 16) * 32 + 1                         # the first column count that pads to ldx words
    print(f"row search: chunk {chunk} of {ldx} words at n = {n}")
    assert 0 < chunk < ldx and lib.bmf_asso_refine_chunk(k, ldx - 16, 1) == ldx - 16
    X, U, V = RG.random_case(m, n, k, 2695)
    eng, _ = RG.search_both(X, U, V, 0.3, 0.7)
    assert eng.ldx == ldx
    forced, _ = RG.search_both(X, U, V, 0.3, 0.7, chunk=chunk - 4)
    assert forced.U.cpu().numpy().tobytes() == eng.U.cpu().numpy().tobytes()


def test_two_identical_visits_at_k_64_give_identical_bytes():
    X, U, V = dense_case(70, 45, 64, 2696)
    out = []
    for _ in range(2):
        eng = RG.device_engine(X, U, V)
        rec = [eng.refine_column(kc, 0.3, 0.7) for kc in (0, 63, 32)]
        out.append((rec, eng.U.cpu().numpy().tobytes(), eng._u.cpu().numpy().tobytes(), eng._part[: 3 * 3].cpu().numpy().tobytes()))
    assert out[0] == out[1]


# ---- C4: edges of the GreConD scan --------------------------------------------------------------------------------------------
def scan_case():
    rng = np.random.RandomState(2697)
    X = rng.rand(2049, 40) < 0.3
    X[:100, :16] = False                            # with the first 100 rows as best_u, u_j is empty for a whole candidate group
    X[:, 17] = X[:, 2]
    X[2048, ::3] = True                             # the one real word of the second 64-lane chunk
    ref = G.NumpyConceptEngine(X)
    resid = X & (rng.rand(2049, 40) < 0.7)
    ref.rs_t, ref.pd_t = G.pack_rows(resid.T, ref.W), G.pack_rows((X & ~resid).T, ref.W)
    return ref


@pytest.mark.parametrize("count", [16, 17, 1])
def test_grecond_scan_with_a_full_group_one_more_and_one(count):
    ref = scan_case()
    assert ref.m == 2049 and ref.W > 64             # a bit row needs a second chunk of 64 lanes
    GG.check_point(ref, ref.all_rows, np.arange(count) + 20, 0, f"{count} candidates")
    GG.check_point(scan_case(), ref.all_rows, (np.arange(count) + 3)[::-1].copy(), 50, f"{count} candidates, reversed")


def test_grecond_scan_with_a_group_of_empty_row_sets():
    ref = scan_case()
    first_100 = G.pack_rows((np.arange(2049) < 100)[None, :], ref.W)[0]
    s0, nu0, nv0, _ = G.scan_block(ref.Xt, ref.rs_t, ref.n, first_100, np.arange(40), 0)
    assert (nu0[:16] == 0).all() and (nu0[16:] > 0).any() and (nv0[:16] == ref.n).all() and (s0[:16] == 0).all()
    GG.check_point(ref, first_100, np.arange(40), 0, "first group all empty")
    GG.check_point(scan_case(), first_100, np.arange(16), 0, "only the empty group")


def test_grecond_scan_with_a_single_row_as_best_u():
    for row in (2048, 0):
        ref = scan_case()
        one = G.pack_rows((np.arange(2049) == row)[None, :], ref.W)[0]
        s0, nu0, _, _ = G.scan_block(ref.Xt, ref.rs_t, ref.n, one, np.arange(40), 0)
        assert set(nu0.tolist()) == {0, 1} and nu0.sum() >= 2
        GG.check_point(ref, one, np.arange(40), 0, f"best_u = row {row}")
