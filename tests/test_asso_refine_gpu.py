"""AssoIter and AssoOpt on the device: the kernels of csrc/asso_refine.hip against the NumPy restatements of
tests/test_asso_refine_cpu.py on random bits at ragged shapes, the real classes against the reference's results
(tests/golden/g25_asso_refine.*), and runs at the MovieLens-1M shape that no reference stands behind, held to invariants.

Counts are integers and the decisions are one fp64 expression on them: new columns, j per row, TP, FP and |u| are compared by equality,
the score by equality for dyadic weights and within 1e-12 relative otherwise (a sum in another order, as in test_asso_*).
"""
import contextlib
import io
import time
import types

import numpy as np
import pytest
from scipy.sparse import lil_matrix

from test_asso_refine_cpu import (ITER_CASES, OPT_CASES, check_iter, check_opt, check_score, dyadic, fit_case, load_case, optimal_rows_numpy,
                                  refine_column_numpy, subset_scores)

pytestmark = pytest.mark.gpu


def device_engine(X, U, V):
    from pybmf_amd.asso_refine import AssoRefineEngine
    from pybmf_amd.engine import BitMatrix
    eng = AssoRefineEngine(BitMatrix(np.ascontiguousarray(X, dtype=np.uint8), "cuda:0"))
    eng.load_factors(U, V)
    return eng


def random_case(m, n, k, seed, density=0.2):
    rng = np.random.RandomState(seed)
    U, V = rng.rand(m, k) < min(density, 2.0 / k), rng.rand(n, k) < density
    X = ((U.astype(np.int64) @ V.T.astype(np.int64)) > 0) ^ (rng.rand(m, n) < 0.05)
    U = U ^ (rng.rand(m, k) < 0.1)      # the factors that go in are not the planted ones
    return X, U, V


# ---- fixtures through the real classes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ITER_CASES)
def test_assoiter_reproduces_the_reference(name):
    from pybmf_amd.asso_refine import AssoRefineEngine
    case = load_case(name)
    model = fit_case(case, "AssoIter")
    assert isinstance(model._engine, AssoRefineEngine)
    check_iter(model, case)


@pytest.mark.parametrize("name", OPT_CASES)
def test_assoopt_reproduces_the_reference(name):
    from pybmf_amd.asso_refine import AssoRefineEngine
    case = load_case(name)
    model = fit_case(case, "AssoOpt")
    assert isinstance(model._engine, AssoRefineEngine)
    check_opt(model, case)


# ---- the column kernel --------------------------------------------------------------------------------------------------------
def visit_both(eng, X, U, V, kc, w_fp, w_fn, chunk=None):
    """One visit of column kc on the device and in NumPy; U (host) is updated like the device's masks."""
    take, score, T, F = refine_column_numpy(X, U, V, kc, w_fp, w_fn)
    got = eng.refine_column(kc, w_fp, w_fn, chunk=chunk)
    assert got[1:] == (T, F, int(take.sum())), (kc, got, T, F)
    check_score(got[0], score, dyadic(w_fp, w_fn))
    assert eng.column().tolist() == take.tolist()
    U[:, kc] = take
    return got


@pytest.mark.parametrize("m,n,k,cols,chunks", [(96, 72, 5, (0, 2, 4), (None, 4)), (65, 33, 1, (0,), (None, 8)), (130, 100, 33, (0, 31, 32), (None, 12)),
                                               (70, 1100, 3, (1,), (None, 20))])
@pytest.mark.parametrize("w_fp,w_fn", [(0.5, 0.5), (1.0, 1.0), (0.3, 0.7)])
def test_column_kernel_against_numpy(m, n, k, cols, chunks, w_fp, w_fn):
    X, U0, V = random_case(m, n, k, 100 * k + m)
    for chunk in chunks:            # a forced chunk walks over n in pieces: the same result
        U = U0.copy()
        eng = device_engine(X, U, V)
        for kc in cols + cols[:1]:  # the first column again: it now meets the columns refined since
            visit_both(eng, X, U, V, kc, w_fp, w_fn, chunk)
        Ue, Ve = eng.factor_arrays()
        assert (Ue != 0).tolist() == U.tolist() and (Ve != 0).tolist() == V.tolist()
        P = (U.astype(np.int64) @ V.T.astype(np.int64)) > 0
        assert (np.asarray(eng.prediction().todense()) != 0).tolist() == P.tolist()
        tp, fp = int((X & P).sum()), int((~X & P).sum())
        assert eng.counts("train") == (tp, fp, int(X.sum()) - tp, m * n - int(X.sum()) - fp)
        masks = eng.U.cpu().numpy().view(np.uint32)
        assert not (masks[:, -1] >> np.uint32(k % 32)).any() if k % 32 else True      # mask bits past k stay zero


def test_column_kernel_at_ml1m_shape():
    m, n, k = 6040, 3706, 8
    X, U, V = random_case(m, n, k, 2501, density=0.12)
    eng = device_engine(X, U, V)
    assert eng.ldx == 128
    for kc in (0, 3, 7):
        visit_both(eng, X, U, V, kc, 0.5, 0.5)
    visit_both(eng, X, U, V, 5, 0.3, 0.7, chunk=36)      # 128 words in chunks of 36: a ragged last chunk


def test_two_identical_visits_give_identical_bytes():
    X, U, V = random_case(700, 300, 40, 2502)
    out = []
    for _ in range(2):
        eng = device_engine(X, U, V)
        rec = [eng.refine_column(kc, 0.3, 0.7) for kc in (0, 39, 17)]
        out.append((rec, eng.U.cpu().numpy().tobytes(), eng._part[: 3 * 22].cpu().numpy().tobytes()))
    assert out[0] == out[1]


# ---- the row-search kernel ----------------------------------------------------------------------------------------------------
def search_both(X, U, V, w_fp, w_fn, chunk=None):
    eng = device_engine(X, U, V)
    got = eng.optimal_rows(w_fp, w_fn, chunk=chunk)
    j, U_new, T, F = optimal_rows_numpy(X, V, w_fp, w_fn)
    assert eng.chosen().tolist() == j.tolist()
    assert got[1:] == (T, F, int(U_new.sum()))
    check_score(got[0], w_fn * float(T) - w_fp * float(F), dyadic(w_fp, w_fn))
    assert (eng.factor_arrays()[0] != 0).tolist() == U_new.tolist()
    return eng, j


# k = 12 is what the issue asks for; 13 is the first k with an outer pass, 16 the limit (brute force in NumPy: 65536 x 30 x 40, well under a second)
@pytest.mark.parametrize("m,n,k", [(65, 33, 1), (65, 33, 2), (65, 33, 7), (40, 30, 12), (40, 30, 13), (40, 30, 16)])
@pytest.mark.parametrize("w_fp,w_fn", [(1.0, 1.0), (0.3, 0.7)])
def test_row_search_against_brute_force(m, n, k, w_fp, w_fn):
    X, U, V = random_case(m, n, k, 300 + k, density=0.15)
    search_both(X, U, V, w_fp, w_fn)
    if k in (2, 13):
        search_both(X, U, V, w_fp, w_fn, chunk=4)


def test_row_search_across_chunks_of_a_wide_matrix():
    X, U, V = random_case(33, 1100, 5, 2503)      # 48 words per bit row, in chunks of 20: a ragged last chunk
    search_both(X, U, V, 0.3, 0.7, chunk=20)


def test_row_search_takes_the_first_of_equal_subsets():
    """Duplicate columns of V make whole families of subsets tie; an all-zero row of X makes every subset without a one tie with
    j = 0.  The device must return NumPy's first maximal j in the MSB-first order."""
    rng = np.random.RandomState(2504)
    m, n, k = 48, 40, 10
    base = rng.rand(n, 3) < 0.3
    V = base[:, [0, 1, 0, 2, 1, 0, 2, 2, 1, 0]].copy()
    V[:, 4] = False                                           # an empty factor: with or without it, the same score
    X = ((rng.rand(m, 3) < 0.5).astype(np.int64) @ base.T.astype(np.int64) > 0) ^ (rng.rand(m, n) < 0.03)
    X[7] = False
    U = rng.rand(m, k) < 0.3
    for w_fp, w_fn in ((1.0, 1.0), (0.3, 0.7), (0.0, 1.0)):
        eng, j = search_both(X, U, V, w_fp, w_fn)
        scores, _, _ = subset_scores(X, V, w_fp, w_fn)
        ties = (scores == scores.max(axis=0)[None, :]).sum(axis=0)
        assert ties.min() >= 2 and ties.max() >= 14       # every row has tied subsets
        if w_fp > 0:
            assert j[7] == 0                              # the empty row: nothing beats the empty subset
        # the first of equals uses the later copies of a duplicated factor (low bits of j), never the earlier ones
        assert not ((j >> (k - 1 - 0)) & 1).any() or w_fp == 0.0


def test_limits_are_refused():
    rng = np.random.RandomState(5)
    X = rng.rand(40, 30) < 0.3
    eng = device_engine(X, rng.rand(40, 17) < 0.2, rng.rand(30, 17) < 0.2)
    with pytest.raises(NotImplementedError, match="k <= 16"):
        eng.optimal_rows(1.0, 1.0)
    assert eng.refine_column(16, 0.5, 0.5)[3] >= 0           # the column kernel has no such limit
    from pybmf_amd.models import AssoOpt
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match="k <= 16"):
            AssoOpt(model=types.SimpleNamespace(k=17, U=lil_matrix(rng.rand(40, 17) < 0.2), V=lil_matrix(rng.rand(30, 17) < 0.2), logs={})).fit(
                X.astype(np.uint8), task="reconstruction", show_logs=False, show_result=False, save_model=False)


# ---- MovieLens-1M shape -------------------------------------------------------------------------------------------------------
def test_ml1m_shape_invariants():
    from pybmf_amd.generators import PlantedBooleanOnDevice
    from pybmf_amd.models import Asso, AssoIter, AssoOpt
    m, n, k = 6040, 3706, 8
    kw = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
    X = PlantedBooleanOnDevice(m, n, 10, density=(0.15, 0.15), seed=2410, noise=(0.05, 0.005), noise_seed=2411)[0:m].cpu().numpy()
    Xd = X != 0
    with contextlib.redirect_stdout(io.StringIO()):
        asso = Asso(tau=0.5, k=k, w_fp=0.5)
        asso.fit(X, **kw)
        t0 = time.time()
        it = AssoIter(model=asso, w_fp=0.7)
        it.fit(X, **kw)
        t1 = time.time()
        opt = AssoOpt(model=types.SimpleNamespace(k=k, U=it.U, V=it.V, logs={}), w_fp=1, w_fn=1)
        opt.fit(X, **kw)
        t2 = time.time()
    print(f"ml1m k = {k}: AssoIter {len(it.visits)} visits in {t1 - t0:.2f} s, AssoOpt in {t2 - t1:.2f} s")
    # AssoIter: every logged visit lowers the error strictly; the log is what the visits say
    tp, fp, fn, tn = asso._engine.counts("train")
    errors = [1 - np.float64(tp + tn) / (m * n)] + [v[1] for v in it.visits if v[2]]
    assert all(b < a for a, b in zip(errors, errors[1:]))
    rows = it.logs["refinements"].values.tolist() if "refinements" in it.logs else []
    assert [r[3] for r in rows] == errors[1:] and [r[1] for r in rows] == [v[0] for v in it.visits if v[2]]
    assert [v[2] for v in it.visits][-k:] == [False] * k
    tp_i, fp_i, fn_i, tn_i = it._engine.counts("train")
    assert tp_i + fn_i == tp + fn and tp_i + fp_i + fn_i + tn_i == m * n
    assert 1 - np.float64(tp_i + tn_i) / (m * n) == it.visits[-1][1]
    # AssoOpt: no row's score is below its score before (the row's old subset is one of the 2^k), and j per row is the brute
    # force's.  On this matrix AssoIter's rows may all be optimal already (the planted factors are found nearly exactly, and a row
    # either holds a factor or does not, under any weights), so a second fit starts from AssoIter's U with one cell in ten flipped:
    # a row that lost a factor it holds gives up some 500 true positives, so there the search must do strictly better.
    U0, V = np.asarray(it.U.todense()) != 0, np.asarray(it.V.todense()) != 0
    U0_flipped = U0 ^ (np.random.RandomState(2412).rand(m, k) < 0.1)
    with contextlib.redirect_stdout(io.StringIO()):
        opt2 = AssoOpt(model=types.SimpleNamespace(k=k, U=lil_matrix(U0_flipped), V=it.V, logs={}), w_fp=1, w_fn=1)
        opt2.fit(X, **kw)

    # all 2^k subsets in NumPy, in fp32 (counts below 2^24 are exact there): TP[j, i], FP[j, i] and the score as the reference writes it
    member = ((np.arange(1 << k)[:, None] >> (k - 1 - np.arange(k))[None, :]) & 1).astype(np.float32)
    P = (member @ V.T.astype(np.float32)) > 0
    TP = (P.astype(np.float32) @ Xd.T.astype(np.float32)).astype(np.int64)
    FP = P.sum(axis=1).astype(np.int64)[:, None] - TP
    scores = -1.0 * FP.astype(np.float64) + 1.0 * TP.astype(np.float64)
    j_ref, rows_i = scores.argmax(axis=0), np.arange(m)
    s_ref, tp_ref, fp_ref = scores[j_ref, rows_i], int(TP[j_ref, rows_i].sum()), int(FP[j_ref, rows_i].sum())

    def row_scores(U):
        return scores[(U.astype(np.int64) << (k - 1 - np.arange(k))[None, :]).sum(axis=1), rows_i]
    s0, s0_flipped = row_scores(U0), row_scores(U0_flipped)
    assert (s_ref > s0_flipped).any()                     # the flipped start leaves the search something to find
    for model, before in ((opt, s0), (opt2, s0_flipped)):
        U1 = np.asarray(model.U.todense()) != 0
        assert U1.shape == (m, k) and (np.asarray(model.V.todense()) != 0).tolist() == V.tolist()
        assert model.chosen.tolist() == j_ref.tolist()
        s1 = row_scores(U1)
        assert (s1 >= before).all() and s1.tolist() == s_ref.tolist()
        assert model._engine.counts("train")[:2] == (tp_ref, fp_ref)
        assert float(model.logs["refinements"].values.tolist()[-1][1]) == float(tp_ref - fp_ref)
        bits = ((model.chosen[:, None] >> (k - 1 - np.arange(k))[None, :]) & 1).astype(bool)
        assert bits.tolist() == U1.tolist()
    assert (row_scores(np.asarray(opt2.U.todense()) != 0) > s0_flipped).any()
