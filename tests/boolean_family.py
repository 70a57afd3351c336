"""A seeded family of edge-case Boolean matrices and the parameter grids that the four bit-set models (GreConD, Asso, AssoIter,
AssoOpt) are run through on both engines: the NumPy stand-ins of tests/test_{grecond,asso,asso_refine}_cpu.py and the device engines.
Plain helpers, no tests: tests/test_boolean_family_cpu.py and tests/test_boolean_family_gpu.py import this module the way
test_asso_gpu.py imports test_asso_cpu.

The family (family(); every matrix uint8, fixed RandomState seeds, at most 120 x 90 except the two 2049 shapes):
  zeros, ones (12 x 9), one_cell (1 x 1 = 1), row (1 x 70), col (70 x 1), identity (40 x 40)
  dup       planted rank 4, 60 x 45, noise free; column 7 is a copy of column 3 and row 11 a copy of row 5
  nested    50 x 12, column j holds rows [0, 50 - 4 j): a chain c0 > c1 > ...
  holes     planted rank 4, 64 x 48, 2 % flips, row 9 and column 4 emptied
  blocks    90 x 60, three diagonal blocks of 30 x 20, 1 % of the cells flipped
  low_rank  50 x 40 of Boolean rank 2, fitted with k = 6: a rank the data cannot supply
  b31x63, b32x64, b33x65, b64x128, b65x129, b2049x20, b20x2049   planted rank 3, 3 % flips: on, and one off, the 32-bit word, the
            64-row / 64-candidate tile and the 64-lane chunk of a 65-word bit row (2049 rows)
  split     planted rank 4, 120 x 90, 3 % flips, its ones dealt to train / val / test (70 / 15 / 15 %): the fits carry `extra` truths

The grids, and what was dropped from the full products of the issue's table:
  GreConD   k in {None, 3} x block in {None, 1, 7} on the matrices whose exact decomposition is short (the degenerate ones, identity,
            dup, nested, low_rank).  On a matrix with flipped cells k = None runs until every flipped cell has a factor of its own
            (hundreds of concepts, minutes on the host stand-in), so there k = 3 only.  At the two 2049 shapes block = 1 is dropped
            (one launch per candidate on the host stand-in: 2049 scans per sweep); None and 7 stay, so the result is still compared
            across block sizes.
  Asso      k = the case's k (at most 6; 1 on the matrices one factor reconstructs, 3 on dup and nested: the largest k that both
            recorded parameter sets of tests/golden/make_golden_family.py reach, so that the reference ends without an exception).  tau in {0.3, 0.5} x the four weight pairs at block = None; blocks 1 and 7 at
            (tau 0.5, 0.5 / 0.5) and (tau 0.3, 0.3 / 0.7) only (a block size changes how a sweep is cut up, not what a weight pair
            scores); tau = 1.0 once (nothing is above 1: the candidate list is empty whatever the weights).  zeros keeps one weight
            pair per tau (no candidate, no score).  At b20x2049 (2049 candidates) block = 1 is dropped.
  refiners  AssoIter and AssoOpt start from the stand-in's Asso fit of the same case (tau 0.5, 0.5 / 0.5), and again from that U with
            one cell in ten flipped, under the four weight pairs.  Where that Asso fit keeps no factor (zeros has no candidate; on a
            matrix it reconstructs exactly the tolerance stop truncates the factor) the start is one factor of all ones in U and V.
            zeros keeps the pairs 0.5 / 0.5 and 0 / 1.
  31 .. 33 rows by 63 .. 65 columns are taken as the three pairs (31, 63), (32, 64), (33, 65): each edge value of either dimension
  occurs once; the six mixed pairs add no further word or tile boundary.
"""
import contextlib
import functools
import io

import numpy as np

import test_asso_cpu as A
import test_asso_refine_cpu as R
import test_grecond_cpu as G

WEIGHTS = [(0.5, 0.5), (0.3, 0.7), (1.0, 1.0), (0.0, 1.0)]
BOUNDARY = [(31, 63), (32, 64), (33, 65), (64, 128), (65, 129), (2049, 20), (20, 2049)]
DEGENERATE = ["zeros", "ones", "one_cell", "row", "col"]
SHORT = DEGENERATE + ["identity", "dup", "nested", "low_rank"]      # exact decompositions of a few factors: GreConD runs k = None too
BIG = ["b2049x20", "b20x2049"]


def exact_weights(w_fp, w_fn):
    """Weights whose products with integer counts are exact in fp64: the score is compared with ==, else within 1e-12 relative."""
    return (float(w_fp), float(w_fn)) in ((0.5, 0.5), (1.0, 1.0), (0.0, 1.0))


def planted(m, n, k, density, flips, seed):
    rng = np.random.RandomState(seed)
    U, V = rng.rand(m, k) < density, rng.rand(n, k) < density
    X = (U.astype(int) @ V.astype(int).T) > 0
    if flips:
        X = X ^ (rng.rand(m, n) < flips)
    return X.astype(np.uint8)


def deal(X, seed):
    """The ones of X dealt to three matrices with disjoint cells: 70 % train, 15 % val, 15 % test."""
    lot = np.random.RandomState(seed).rand(*X.shape)
    ones = X != 0
    return tuple(a.astype(np.uint8) for a in (ones & (lot < 0.7), ones & (lot >= 0.7) & (lot < 0.85), ones & (lot >= 0.85)))


@functools.lru_cache(maxsize=None)
def family():
    """{name: dict(X=uint8 matrix, k=rank to fit, X_val / X_test for `split`)}, in a fixed order."""
    fam = {}

    def add(name, X, k, **more):
        X = np.ascontiguousarray(X, dtype=np.uint8)
        X.setflags(write=False)
        fam[name] = dict(more, X=X, k=k, tol=0, shape=list(X.shape))
    add("zeros", np.zeros((12, 9)), 2)
    add("ones", np.ones((12, 9)), 1)
    add("one_cell", np.ones((1, 1)), 1)
    row = np.random.RandomState(2601).rand(1, 70) < 0.75
    row[0, 0], row[0, 1] = False, True
    add("row", row, 1)
    col = np.random.RandomState(2602).rand(70, 1) < 0.75
    col[0, 0], col[1, 0] = False, True
    add("col", col, 1)
    add("identity", np.eye(40), 5)
    dup = planted(60, 45, 4, 0.25, 0.0, 2603)
    dup[:, 7] = dup[:, 3]
    dup[11] = dup[5]
    add("dup", dup, 3)
    add("nested", np.arange(50)[:, None] < (50 - 4 * np.arange(12))[None, :], 3)
    holes = planted(64, 48, 4, 0.25, 0.02, 2604)
    holes[9], holes[:, 4] = 0, 0
    add("holes", holes, 4)
    blocks = np.kron(np.eye(3), np.ones((30, 20))).astype(bool) ^ (np.random.RandomState(2605).rand(90, 60) < 0.01)
    add("blocks", blocks, 3)
    add("low_rank", planted(50, 40, 2, 0.3, 0.0, 2606), 6)
    for i, (m, n) in enumerate(BOUNDARY):
        add(f"b{m}x{n}", planted(m, n, 3, 0.3, 0.03, 2610 + i), 3)
    tr, va, te = deal(planted(120, 90, 4, 0.25, 0.03, 2620), 2621)
    add("split", tr, 4, X_val=va, X_test=te)
    return fam


CASES = list(family())


# ---- grids ------------------------------------------------------------------------------------------------------------------
def grecond_grid(name):
    ks = (None, 3) if name in SHORT else (3,)
    blocks = (None, 7) if name in BIG else (None, 1, 7)
    return [dict(k=k, block=b) for k in ks for b in blocks]


def asso_grid(name):
    pairs = WEIGHTS[:1] if name == "zeros" else WEIGHTS
    grid = [dict(tau=tau, w_fp=w[0], w_fn=w[1], block=None) for tau in (0.3, 0.5) for w in pairs]
    for tau, w in ((0.5, WEIGHTS[0]), (0.3, WEIGHTS[1])):
        grid += [dict(tau=tau, w_fp=w[0], w_fn=w[1], block=b) for b in ((7,) if name == "b20x2049" else (1, 7))]
    return grid + [dict(tau=1.0, w_fp=0.5, w_fn=0.5, block=None)]


def refine_grid(name):
    pairs = [WEIGHTS[0], WEIGHTS[3]] if name == "zeros" else WEIGHTS
    return [dict(flipped=f, w_fp=w[0], w_fn=w[1]) for f in (False, True) for w in pairs]


# ---- fits -------------------------------------------------------------------------------------------------------------------
def record_applies(eng):
    """Wrap eng.apply / eng.truncate (an Asso engine of either kind) so that eng.history keeps every factor as it was applied: the
    model's own U, V lose the factors that a tolerance stop truncates."""
    eng.history = []
    apply, truncate = eng.apply, eng.truncate

    def logged_apply(u, v):
        eng.history.append(("apply", A.unpack(u, eng.m).copy(), A.unpack(v, eng.n).copy()))
        return apply(u, v)

    def logged_truncate(k):
        eng.history.append(("truncate", int(k)))
        return truncate(k)
    eng.apply, eng.truncate = logged_apply, logged_truncate
    return eng


def fit_grecond(name, k, block, device=False):
    case = dict(family()[name], k=k)
    return G.fit_case(case, None if device else G.numpy_engine, block=block)


def fit_asso(name, tau, w_fp, w_fn, block, device=False):
    from pybmf_amd.models import Asso
    case = dict(family()[name], tau=tau, w_fp=w_fp, w_fn=w_fn)
    factory = (lambda model: record_applies(Asso._make_engine(model))) if device else (lambda model: record_applies(A.numpy_engine(model)))
    return A.fit_case(case, factory, block=block)


@functools.lru_cache(maxsize=None)
def refine_start(name, flipped):
    """(U, V) that the refiners import: the stand-in's Asso fit of the case (tau 0.5, 0.5 / 0.5), or one factor of all ones where that
    fit keeps no factor; `flipped`: one cell of U in ten flipped (seeded per case; cell (0, 0) where the draw flips none)."""
    case = family()[name]
    model = fit_asso(name, 0.5, 0.5, 0.5, None)
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    keep = U.any(axis=0) & V.any(axis=0)          # a column that a tolerance stop emptied is no factor
    U, V = U[:, keep], V[:, keep]
    if U.shape[1] == 0:
        U, V = np.ones((case["shape"][0], 1), dtype=bool), np.ones((case["shape"][1], 1), dtype=bool)
    if flipped:
        flips = np.random.RandomState(2630 + CASES.index(name)).rand(*U.shape) < 0.1
        flips[0, 0] |= not flips.any()            # (a U of one or two cells: the draw may flip none)
        U = U ^ flips
    U, V = U.astype(np.uint8), V.astype(np.uint8)
    U.setflags(write=False)
    V.setflags(write=False)
    return U, V


def fit_refine(name, kind, flipped, w_fp, w_fn, device=False):
    U, V = refine_start(name, flipped)
    case = dict(family()[name], U_in=U, V=V, w_fp=w_fp, w_fn=w_fn)
    return R.fit_case(case, kind, None if device else R.numpy_engine)


# ---- what a fit leaves, in a form that two engines' fits are compared in ------------------------------------------------------
def snapshot(model, kind):
    """kind: 'GreConD' / 'Asso' / 'AssoIter' / 'AssoOpt'.  rows: the log without time stamps; score_at: the row position of the one
    float that is a sum over rows (compared by the score rule); everything else is integers, or floats made by the same host
    expression from equal integers."""
    eng = model._engine
    if kind == "GreConD":
        rows, score_at = G.log_rows(model), None
    elif kind == "Asso":
        rows, score_at = A.log_rows(model), 1
    else:
        rows = [r[1:] for r in model.logs["refinements"].values.tolist()] if "refinements" in model.logs else []
        score_at = 1 if kind == "AssoIter" else 0
    out = dict(kind=kind, rows=rows, score_at=score_at, U=np.asarray(model.U.todense()) != 0, V=np.asarray(model.V.todense()) != 0,
               X_pd=np.asarray(model.X_pd.todense()) != 0, counts={name: tuple(int(c) for c in eng.counts(name)) for name in eng.truth},
               factors=tuple(np.asarray(F) != 0 for F in eng.factor_arrays()))
    if kind == "GreConD":
        out["residual_sum"] = int(eng.residual_sum())
    if kind == "Asso":
        out["history"], out["list"] = eng.history, [int(j) for j in eng.list]
    if kind == "AssoIter":
        out["visits"] = [tuple(v) for v in model.visits]
    if kind == "AssoOpt":
        out["chosen"] = [int(j) for j in model.chosen]
    return out


def assert_same_fit(got, want, exact):
    """Two snapshots of the same fit on two engines (or at two block sizes): integers and bits equal, the score by the score rule."""
    assert got["kind"] == want["kind"] and len(got["rows"]) == len(want["rows"])
    at = got["score_at"]
    for g, w in zip(got["rows"], want["rows"]):
        assert len(g) == len(w)
        for i, (a, b) in enumerate(zip(g, w)):
            if i == at:
                R.check_score(a, float(b), exact)
            else:
                assert a == b, (i, a, b)
    for key in ("U", "V", "X_pd"):
        assert got[key].shape == want[key].shape and (got[key] == want[key]).all(), key
    assert got["counts"] == want["counts"]
    for a, b in zip(got["factors"], want["factors"]):
        assert a.shape == b.shape and (a == b).all()
    for key in ("residual_sum", "list", "visits", "chosen"):
        assert got.get(key) == want.get(key), key
    if "history" in want:
        assert len(got["history"]) == len(want["history"])
        for a, b in zip(got["history"], want["history"]):
            assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# ---- the properties that define a correct result, without a stand-in ----------------------------------------------------------
def grecond_invariants(X, rows, U, V, counts, residual_sum, X_pd):
    """rows: G.log_rows of a GreConD fit on X; U, V: one column per log row (every applied factor, a truncated one included).  Every
    factor is a closed rectangle of ones of X, its score is the drop of the residual sum, and no false positive is ever made."""
    Xb = np.asarray(X) != 0
    U, V = np.asarray(U) != 0, np.asarray(V) != 0
    assert U.shape == (Xb.shape[0], len(rows)) and V.shape == (Xb.shape[1], len(rows))
    covered = np.zeros_like(Xb)
    sum_x = resid = int(Xb.sum())
    for f, r in enumerate(rows):
        u, v = U[:, f], V[:, f]
        assert r[0] == f and r[1] >= 1 and [r[2], r[3]] == [int(u.sum()), int(v.sum())]
        assert Xb[np.ix_(u, v)].all()                                            # a rectangle of ones of X
        assert not (Xb[:, v].all(axis=1) & ~u).any() and not (Xb[u].all(axis=0) & ~v).any()   # closed: no row / column can be added
        covered[np.ix_(u, v)] = True
        now = sum_x - int(covered.sum())
        assert r[1] == resid - now                                               # score = the drop of the residual sum
        resid = now
        recall, precision = r[4], r[5]
        assert precision == 1.0 and abs(recall - (sum_x - resid) / sum_x) <= 1e-12   # FP = 0 on train in every row
    assert tuple(counts) == (int(covered.sum()), 0, resid, Xb.size - sum_x) and residual_sum == resid
    assert ((np.asarray(X_pd) != 0) == covered).all()
    return covered


def asso_invariants(X, snap, w_fp, w_fn):
    """Every log row's TP, FP are a dense recount of the factors applied so far, its score is w_fn TP - w_fp FP of them, and the
    scores rise strictly; the final prediction is the product of the factors that are left."""
    Xi = (np.asarray(X) != 0).astype(np.int64)
    rows, factors, i, cut = snap["rows"], [], 0, False

    def product():
        P = np.zeros(Xi.shape, dtype=bool)
        for u, v in factors:
            P |= u[:, None] & v[None, :]
        return P
    for ev in snap["history"]:
        if ev[0] == "truncate":
            factors, cut = factors[: ev[1]], True
            continue
        factors.append((ev[1], ev[2]))
        if not (ev[1].any() or ev[2].any()):         # the filler behind a truncated column
            continue
        r, P = rows[i], product().astype(np.int64)
        tp, fp = int((Xi * P).sum()), int(((1 - Xi) * P).sum())
        assert [int(r[6]), int(r[8]), int(r[10])] == [tp, fp, int(Xi.sum()) - tp]
        R.check_score(r[1], w_fn * float(tp) - w_fp * float(fp), exact_weights(w_fp, w_fn))
        assert r[2] == 0.5 * tp - 0.5 * fp and [r[4], r[5]] == [int(ev[1].sum()), int(ev[2].sum())] and r[4] > 0 and r[5] > 0
        if not cut:
            assert r[3] == sum(int(u.sum()) + int(v.sum()) for u, v in factors) + fp + int(r[10])      # description length
        i += 1
    assert i == len(rows)
    scores = [r[1] for r in rows]
    assert all(b > a for a, b in zip(scores, scores[1:])) and (not scores or scores[0] > 0)
    assert (snap["X_pd"] == product()).all()
    P = snap["X_pd"].astype(np.int64)
    tp, fp = int((Xi * P).sum()), int(((1 - Xi) * P).sum())
    assert snap["counts"]["train"] == (tp, fp, int(Xi.sum()) - tp, Xi.size - int(Xi.sum()) - fp)


def iter_invariants(X, snap, start_U, V):
    """The error falls strictly over the logged visits, the fit ends with k fruitless visits (and not earlier), the log is what the
    visits say, and the last visit's error is the error of the U that is left."""
    Xb, V = np.asarray(X) != 0, np.asarray(V) != 0
    k, visits = V.shape[1], snap["visits"]

    def error(U):
        P = ((np.asarray(U) != 0).astype(np.int64) @ V.T.astype(np.int64)) > 0
        return 1 - np.float64(int((P == Xb).sum())) / Xb.size
    errors = [error(start_U)] + [v[1] for v in visits if v[2]]
    assert all(b < a for a, b in zip(errors, errors[1:]))
    flags = [v[2] for v in visits]
    assert flags[-k:] == [False] * k and all(any(flags[i:i + k]) for i in range(len(flags) - k))
    assert [v[0] for v in visits] == [i % k for i in range(len(visits))]
    assert [r[2] for r in snap["rows"]] == errors[1:] and [r[0] for r in snap["rows"]] == [v[0] for v in visits if v[2]]
    assert error(snap["U"]) == visits[-1][1] and (snap["V"] == V).all()
    tp, fp, fn, tn = snap["counts"]["train"]
    assert 1 - np.float64(tp + tn) / Xb.size == visits[-1][1] and tp + fn == int(Xb.sum()) and tp + fp + fn + tn == Xb.size


def opt_invariants(X, snap, V, w_fp, w_fn):
    """Every row's j is NumPy's brute-force argmax over the 2^k subsets, U is the bits of j, the counts are those of that U."""
    Xb, V = np.asarray(X) != 0, np.asarray(V) != 0
    k = V.shape[1]
    j, U, T, F = R.optimal_rows_numpy(Xb, V, float(w_fp), float(w_fn))
    assert snap["chosen"] == j.tolist() and (snap["U"] == U).all() and (snap["V"] == V).all()
    assert (snap["U"] == (((j[:, None] >> (k - 1 - np.arange(k))[None, :]) & 1) != 0)).all()
    assert snap["counts"]["train"][:2] == (T, F) and len(snap["rows"]) == 1
    R.check_score(snap["rows"][0][0], w_fn * float(T) - w_fp * float(F), exact_weights(w_fp, w_fn))


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield
