"""tests/masked_ref.py (the cell-by-cell fp64 restatements that tests/test_masked_kernels_gpu.py holds the observed-cell kernels to)
against the golden-pinned oracle on a dense scatter of the same cells.  Both sides are fp64 NumPy: every agreement is to 1e-12
relative, no entry left out.  No GPU."""
import numpy as np
import pytest

import masked_ref as R
import oracle as orc

LENGTHS = [0, 1, 2, 3, 5, 8, 17, 33, 40, 64, 65, 70]     # an empty row, rows on both sides of a 64-cell segment, a full row
N = 70
RTOL = 1e-12


def close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * scale, err_msg=what)


def cells(seed, real=False, weights=True):
    rs = np.random.RandomState(seed)
    rows, cols, x, w = R.make_cells(LENGTHS, N, rs, real=real, weights=weights, full_col=11)
    return rs, rows, cols, x, w


def test_make_cells_builds_the_rows_it_was_asked_for():
    rs, rows, cols, x, w = cells(0)
    m = len(LENGTHS)
    assert np.bincount(rows, minlength=m).tolist() == LENGTHS
    key = rows * N + cols
    assert (np.diff(key) > 0).all()                                    # row-major, columns increasing, nothing repeated
    assert (cols[rows == 11] == np.arange(N)).all()
    assert np.bincount(cols, minlength=N)[11] == sum(ln > 0 for ln in LENGTHS)      # the full column
    assert set(np.unique(w)) == set(R.WEIGHTS) and set(np.unique(x)) == {0.0, 1.0}
    _, _, _, xr, wr = cells(0, real=True, weights=False)
    assert wr is None and set(np.unique(xr)) == set(R.REAL_VALUES)
    X, W = R.scatter(rows, cols, x, w, (m, N))
    assert (W != 0).sum() == len(rows) and W.sum() == pytest.approx(w.sum()) and X.sum() == x.sum()


@pytest.mark.parametrize("weights", [False, True])
def test_segments_ref_plain_is_the_masked_product(weights):
    rs, rows, cols, x, w = cells(1, weights=weights)
    m, k = len(LENGTHS), 7
    U, V = rs.rand(m, k), rs.rand(N, k)
    X, W = R.scatter(rows, cols, x, w, (m, N))
    P = U @ V.T
    num, den, sums = R.segments_ref(rows, cols, x, w, U, V, R.LINK_PLAIN, 0.0)
    close(num, (W * X) @ V, "num")
    close(den, (W * P) @ V, "den")
    close(sums, [(W * (X - P) ** 2).sum(), (W * np.abs(X - P)).sum()], "sums")
    assert (num[0] == 0).all() and (den[0] == 0).all()
    # the other orientation: the same cells by column, the factors swapped
    numv, denv, sumsv = R.segments_ref(cols, rows, x, w, V, U, R.LINK_PLAIN, 0.0)
    close(numv, (W * X).T @ U, "num^T")
    close(denv, (W * P).T @ U, "den^T")
    close(sumsv, sums, "sums^T")
    # and the update it feeds, through the oracle's own division step
    reg = 0.7
    close(U * ((num + 3 * reg * U ** 2) / (den + 2 * reg * U ** 3 + reg * U)), orc.penalty_update_U(X, W, U, V, reg), "penalty_update_U")


@pytest.mark.parametrize("lamda", [10.0, 100.0])
def test_segments_ref_sigmoid_reproduces_the_pnlpf_updates(lamda):
    rs, rows, cols, x, w = cells(2)
    m, k = len(LENGTHS), 6
    # (products within ~0.35 of 1/2 at lamda = 100 keep the oracle's own sig (1 - sig) clear of its cancellation: 1 - sig > 1e-15 / 1e-12
    #  needs |s| < 6.9)
    spread = 1.0 if lamda == 10.0 else 0.06
    U = np.sqrt(0.5 / k) * (1 + spread * (rs.rand(m, k) - 0.5))
    V = np.sqrt(0.5 / k) * (1 + spread * (rs.rand(N, k) - 0.5))
    assert np.abs(lamda * (U @ V.T - 0.5)).max() < 6.9
    X, W = R.scatter(rows, cols, x, w, (m, N))
    reg = 0.3

    def step(F, num, den):
        den = den + 2 * reg * F ** 3 + reg * F
        den[den == 0] = orc.EPS
        Fn = F * ((num + 3 * reg * F ** 2) / den)
        Fn[Fn == 0] = orc.EPS
        return Fn

    num, den, sums = R.segments_ref(rows, cols, x, w, U, V, R.LINK_SIGMOID, lamda)
    close(step(U, num, den), orc.pnlpf_update_U(X, W, U, V, reg, lamda), "pnlpf_update_U")
    numv, denv, sumsv = R.segments_ref(cols, rows, x, w, V, U, R.LINK_SIGMOID, lamda)
    close(step(V, numv, denv), orc.pnlpf_update_V(X, W, U, V, reg, lamda), "pnlpf_update_V")
    sig = orc.pnlpf_prediction(U, V, lamda)
    assert 0.5 * sums[0] == pytest.approx(orc.rec_term(X, sig, W), rel=RTOL)
    close(sums, [(W * (X - sig) ** 2).sum(), (W * np.abs(X - sig)).sum()], "sums")
    close(sumsv, sums, "sums^T")
    # the pieces themselves, not only their quotient
    d = sig * (1 - sig)
    close(num, lamda * (W * X * d) @ V, "num")
    close(den, lamda * (W * sig * d) @ V, "den")


def test_segments_ref_kl_reproduces_one_wnmf_kl_update():
    rs, rows, cols, x, w = cells(3, real=True)
    m, k = len(LENGTHS), 5
    assert (x == 0).any() and (x == 5).any()
    U0, V0 = rs.rand(m, k) + 0.05, rs.rand(N, k) + 0.05
    X, W = R.scatter(rows, cols, x, w, (m, N))
    ref = orc.wnmf_kl_fit(X, k, U=U0, V=V0, W=W, max_iter=0, init_method="custom")     # max_iter = 0: exactly one sweep, V then U
    assert ref["n_iter"] == 1
    numv, denv, _ = R.segments_ref(cols, rows, x, w, V0, U0, R.LINK_KL, 0.0)
    assert (denv == 0).all()
    V1 = V0 * (numv / U0.sum(0))                        # the denominator O^T U: the column sums of U under the all-ones matrix
    close(V1, ref["V"], "V after one update")
    num, den, _ = R.segments_ref(rows, cols, x, w, U0, V1, R.LINK_KL, 0.0)
    U1 = U0 * (num / V1.sum(0))
    close(U1, ref["U"], "U after one update")
    close(numv, ((W * X) / (U0 @ V0.T)).T @ U0, "numerator of V")
    close(num, ((W * X) / (U0 @ V1.T)) @ V1, "numerator of U")
    # the objective: sums[0] is TWICE it, sums[1] stays 0.  (The oracle turns the zeros of X into eps first, as the reference does: a
    # term of 1e-14 relative to a cell's p, inside the gate.)
    _, _, sums = R.segments_ref(rows, cols, x, w, U1, V1, R.LINK_KL, 0.0)
    assert 0.5 * sums[0] == pytest.approx(ref["updates"][1][1], rel=RTOL)
    assert 0.5 * sums[0] == pytest.approx(orc.wnmf_kl_error(X.copy(), W, U1, V1), rel=RTOL)
    assert sums[1] == 0.0
    # 0 log 0 = 0 exactly: a zero factor row under stored zeros adds nothing and divides by nothing
    Uz = U1.copy()
    Uz[5] = 0.0
    xz = x.copy()
    xz[rows == 5] = 0.0
    with np.errstate(all="raise"):
        numz, _, sumsz = R.segments_ref(rows, cols, xz, w, Uz, V1, R.LINK_KL, 0.0)
    keep = rows != 5
    _, _, sums_rest = R.segments_ref(rows[keep], cols[keep], xz[keep], w[keep], Uz, V1, R.LINK_KL, 0.0)
    assert (numz[5] == 0).all() and sumsz[0] == sums_rest[0] and np.isfinite(numz).all()


@pytest.mark.parametrize("wset", ["mixed", "non-unit", "mask"])
@pytest.mark.parametrize("lamda", [10.0, 100.0])
def test_thresh_ref_is_the_oracle_objective_and_gradient(wset, lamda):
    rs, rows, cols, x, w = cells(4)
    if wset == "non-unit":                      # w in {0.5, 3} only: w^2 != w at every cell, so a weight taken once cannot pass
        w = rs.choice([0.5, 3.0], size=len(rows))
    elif wset == "mask":
        w = None
    m, k = len(LENGTHS), 6
    U, V = rs.rand(m, k), rs.rand(N, k)
    u, v = 0.45, 0.6
    X, W = R.scatter(rows, cols, x, w, (m, N))
    f, g1, g2 = R.thresh_ref(rows, cols, x, w, U, V, u, v, lamda)
    assert 0.5 * f == pytest.approx(orc.thresh_F(X, W, U, V, u, v, lamda), rel=RTOL)       # thresh_F is half the sum
    close([g1, g2], orc.thresh_dF(X, W, U, V, u, v, lamda), "dF")
    if w is not None:
        once = 0.5 * np.sum(W * (X - orc.stable_sigmoid((U - u) * lamda) @ orc.stable_sigmoid((V - v) * lamda).T) ** 2)
        assert abs(0.5 * f - once) > 1e-3 * abs(once)      # the weight really is squared: w r^2 is another number


def test_counts_ref_is_the_confusion_of_the_observed_cells():
    rs, rows, cols, x, _ = cells(5)
    m = len(LENGTHS)
    bits = np.array([0, 1, 1 << 63, (1 << 63) | 1, 1 << 17], dtype=np.uint64)
    ub, vb = rs.choice(bits, size=m), rs.choice(bits, size=N)
    k = 64
    Ub = ((ub[:, None] >> np.arange(k, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)
    Vb = ((vb[:, None] >> np.arange(k, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)
    pd = orc.boolean_product(Ub, Vb, 0.5, 0.5)
    pd = np.asarray(pd.todense() if hasattr(pd, "todense") else pd)
    tp, fp, fn, tn = R.counts_ref(rows, cols, x, ub, vb)
    assert all(isinstance(c, int) for c in (tp, fp, fn, tn)) and tp + fp + fn + tn == len(rows)
    assert (tp, fp, fn, tn) == tuple(int(c) for c in orc.confusion_counts(x, pd[rows, cols]))
    assert min(tp, fp, fn, tn) > 0
