"""Proof of tests/driver_ref.py, the reference that tests/test_driver_gpu.py holds the MU driver (csrc/api.hip) against.  No GPU.

  * log_row equals the oracle's own functions (penalty_errors, rmse_mae, matrix_scores / boolean_scores) on random inputs;
  * on the dyadic hand-made states of bmf_penalty_finalize every intermediate -- of the definition AND of the kernel's expansion
    0.5 (sum X - 2 <X, U V^T> + <U^T U, V^T V>) -- is exact: recomputed in integer / rational arithmetic and compared with ==;
  * gather_sums adds in an order that differs from np.sum on an ill-conditioned input (the order is part of the contract);
  * the stopping rule at its edges (<= on tol, < on min_diff, > on max_iter, never at iteration 0);
  * the slab sums: the grouped order is the sequential one up to 16 slabs and not beyond; the fp32 sum differs from the fp64 one.
"""
from fractions import Fraction

import numpy as np
import pytest

import driver_ref as R
import oracle as orc


@pytest.mark.parametrize("m,n,k,seed", [(37, 29, 5, 0), (64, 50, 12, 1), (20, 90, 33, 2)])
def test_log_row_equals_the_oracle(m, n, k, seed):
    rs = np.random.RandomState(seed)
    X = (rs.rand(m, n) < 0.25).astype(np.float64)
    U, V = rs.rand(m, k) * 1.2, rs.rand(n, k) * 1.2
    reg = 1.75
    row = R.log_row(X, U, V, 3, reg)
    err, rec, rg = orc.penalty_errors(X, None, U, V, reg)
    rmse, mae = orc.rmse_mae(X, orc.real_product(U, V))
    np.testing.assert_allclose([row[R.ERROR], row[R.REC], row[R.REGERR], row[R.RMSE], row[R.MAE]], [err, rec, rg, rmse, mae], rtol=1e-13)
    counts, scores = orc.matrix_scores(X, orc.boolean_product(U, V, 0.5, 0.5))
    assert tuple(int(row[c]) for c in (R.TP, R.FP, R.FN, R.TN)) == tuple(counts)
    assert orc.boolean_scores(*(int(row[c]) for c in (R.TP, R.FP, R.FN, R.TN))) == tuple(scores)
    assert row[R.ITER] == 3.0 and row[R.REG] == reg and row[R.VALID] == 1.0 and row[R.STOP] == 0.0
    # WNMF mode: no regulariser term, the error is the reconstruction error; MAE off: NaN
    roww = R.log_row(X, U, V, 3, reg, mode=R.MODE_WNMF, with_mae=False)
    assert roww[R.REGERR] == 0.0 and roww[R.ERROR] == roww[R.REC] == row[R.REC] and np.isnan(roww[R.MAE])
    assert R.watched(row, R.MODE_PENALTY) == row[R.REGERR] and R.watched(roww, R.MODE_WNMF) == roww[R.REC]


def _exact(x):
    return Fraction(float(x))


@pytest.mark.parametrize("k,kp", [(5, 32), (33, 64)])
@pytest.mark.parametrize("reg", [0.0, 0.5, 2.0, 3.25])
def test_dyadic_states_are_exact(k, kp, reg):
    """Integer arithmetic on 4 U, 4 V (entries 0..5): every sum below is an integer over a power of two and stays far under 2^53 of its
    unit, so fp64 holds every partial sum in any order, and a product rounded or not (FMA) is the same number."""
    X, U, V = R.dyadic_case(k)
    Xi = X.astype(np.int64)
    U4, V4 = np.rint(4 * U).astype(np.int64), np.rint(4 * V).astype(np.int64)
    assert np.array_equal(U4 / 4.0, U) and np.array_equal(V4 / 4.0, V) and U4.max() == 5 and V4.max() == 5
    P16 = U4 @ V4.T                                   # 16 U V^T
    Res16 = 16 * Xi - P16                             # 16 (X - U V^T)
    a = Fraction(int((Xi * P16).sum()), 16)
    sq = Fraction(int((Res16 * Res16).sum()), 256)
    ab = Fraction(int(np.abs(Res16).sum()), 16)
    ru = Fraction(int(((U4 * U4 - 4 * U4) ** 2).sum()), 256)     # (U^2 - U) = (U4^2 - 4 U4) / 16
    rv = Fraction(int(((V4 * V4 - 4 * V4) ** 2).sum()), 256)
    GU16, GV16 = U4.T @ U4, V4.T @ V4
    b = Fraction(int((GU16 * GV16).sum()), 256)
    sum_x, cells = int(Xi.sum()), X.shape[0] * X.shape[1]
    # the identity the kernel relies on, exactly
    assert sq == sum_x - 2 * a + b
    # every intermediate fits: all terms are multiples of 2^-8 and the sums of their magnitudes are below 2^53 * 2^-8
    assert max(int(np.abs(Res16 * Res16).sum()), int((GU16 * GV16).sum()), int((Xi * P16).sum()) * 16) < 2 ** 45

    inp = R.finalize_inputs(X, U, V, kp)
    comm = inp["comm"]
    assert _exact(comm[0]) == a and _exact(comm[1]) == ru and _exact(comm[4]) == ab and _exact(comm[5]) == sq and _exact(inp["scal0"]) == rv
    G = comm[8:].reshape(kp, kp)
    assert np.array_equal(G[:k, :k] * 16, GU16) and np.count_nonzero(G) == np.count_nonzero(GU16)
    assert np.array_equal(inp["GV64"].reshape(kp, kp)[:k, :k] * 16, GV16)
    assert np.array_equal(G.astype(np.float32).astype(np.float64), G)     # (the fp32 copy the next V update takes loses nothing here)

    # the kernel's expansion, step by step in fp64, lands on the exact values
    bf = float(np.dot(comm[8:], inp["GV64"]))
    assert _exact(bf) == b
    rec_k = 0.5 * (float(sum_x) - 2.0 * comm[0] + bf)
    assert _exact(rec_k) == sq / 2
    reg_k = reg * (0.5 * comm[1] + 0.5 * inp["scal0"])
    assert _exact(reg_k) == Fraction(reg) * (ru + rv) / 2
    assert _exact(rec_k + reg_k) == sq / 2 + Fraction(reg) * (ru + rv) / 2

    # and the definition (driver_ref.log_row) gives the same, with ==
    row = R.log_row(X, U, V, 4, reg)
    assert _exact(row[R.REC]) == sq / 2 and _exact(row[R.REGERR]) == Fraction(reg) * (ru + rv) / 2
    assert _exact(row[R.ERROR]) == sq / 2 + Fraction(reg) * (ru + rv) / 2
    assert row[R.TP] == comm[2] and row[R.FP] == comm[3] and row[R.FN] == sum_x - comm[2] and row[R.TN] == cells - sum_x - comm[3]
    # RMSE, MAE: one correctly rounded divide (and square root) of exact operands
    assert row[R.RMSE] == np.sqrt(np.float64(float(sq)) / np.float64(cells)) and row[R.MAE] == float(ab) / cells
    assert abs(Fraction(float(row[R.RMSE])) ** 2 - sq / cells) <= 4 * Fraction(float(np.spacing(row[R.RMSE]))) * Fraction(float(row[R.RMSE]))
    # thresholds are strict: the entries equal to 0.5 are NOT set (they exist in both factors)
    assert (U == 0.5).any() and (V == 0.5).any()


def test_gather_order_matters():
    """thread t adds blocks t, t + 256, ...; then the halving tree.  On an ill-conditioned input that is not np.sum, and not the
    sequential sum either -- so a gather that adds in another order is visible to the == of the GPU test."""
    rs = np.random.RandomState(3)
    nb = 700
    x = rs.randn(nb) * 10.0 ** rs.randint(-8, 9, size=nb)
    part = np.stack([x, x[::-1]], axis=1)
    dot, regu, regv = R.gather_sums(part, part[:300])
    exact = sum(Fraction(float(v)) for v in x)
    seq = 0.0
    for v in x:
        seq += v
    assert regu != seq and (regu != float(np.sum(x)) or dot != float(np.sum(x[::-1])))
    assert abs(Fraction(regu) - exact) < Fraction(1, 10 ** 4) and abs(Fraction(dot) - exact) < Fraction(1, 10 ** 4)
    # by hand, without the helper: 256 strided partial sums, then the tree
    sh = [0.0] * 256
    for t in range(256):
        for b in range(t, nb, 256):
            sh[t] += x[b]
    o = 128
    while o:
        for t in range(o):
            sh[t] += sh[t + o]
        o //= 2
    assert regu == sh[0]
    # fewer blocks than threads (the small shapes): the tree alone; exact inputs give the exact sum
    small = np.arange(1.0, 5.0)
    assert R.gather_sums(np.stack([small, 2 * small], axis=1), np.stack([3 * small, small], axis=1)) == (20.0, 10.0, 30.0)
    assert regv == R.gather_sums(part[:300], part[:300])[1]


def test_stop_rule_edges():
    tol, inf = 0.125, np.inf
    up = lambda x: float(np.nextafter(x, inf))      # noqa: E731
    dn = lambda x: float(np.nextafter(x, -inf))     # noqa: E731
    # tol: <=
    assert R.stop_rule(1, tol, 9.0, tol, 0.0, 100) is True
    assert R.stop_rule(1, up(tol), 9.0, tol, 0.0, 100) is False
    # min_diff: <
    assert R.stop_rule(2, 0.0, 2.0, -1.0, 2.0, 100) is False
    assert R.stop_rule(2, 0.0, dn(2.0), -1.0, 2.0, 100) is True
    assert R.stop_rule(2, 1.0, 1.0, -1.0, 0.0, 100) is False      # min_diff = 0 never stops, not even on a zero difference
    # max_iter: >
    assert R.stop_rule(7, 1.0, 9.0, -1.0, 0.0, 7) is False
    assert R.stop_rule(8, 1.0, 9.0, -1.0, 0.0, 7) is True
    # iteration 0 never stops
    assert R.stop_rule(0, 0.0, 0.0, 1e9, 1e9, -1) is False
    # the oracle's own restatement of early_stop() agrees on all of them
    for it, w, prev, t, md, mi in [(1, tol, 9.0, tol, 0.0, 100), (1, up(tol), 9.0, tol, 0.0, 100), (2, 0.0, 2.0, -1.0, 2.0, 100),
                                   (2, 0.0, dn(2.0), -1.0, 2.0, 100), (7, 1.0, 9.0, -1.0, 0.0, 7), (8, 1.0, 9.0, -1.0, 0.0, 7)]:
        go = orc.should_continue({"tol": t, "max_iter": mi, "min_diff": md}, error=w, diff=abs(prev - w), n_iter=it)
        assert R.stop_rule(it, w, prev, t, md, mi) == (not go)


def test_slab_sum_orders():
    rs = np.random.RandomState(4)
    slabs = (rs.randn(21, 64) * 10.0 ** rs.randint(-6, 7, size=(21, 64))).astype(np.float32)
    for count in (1, 2, 5, 7, 9, 16):
        assert np.array_equal(R.slab_sum_grouped(slabs[:count]), R.slab_sum_seq(slabs[:count]))
    assert not np.array_equal(R.slab_sum_f32(slabs[:7]), R.slab_sum_seq(slabs[:7]))
    # 17 .. 32 slabs: pairs first.  Half an ulp of 2^60 twice: lost one by one (ties to even), kept when added as a pair
    s = np.zeros((18, 1), dtype=np.float32)
    s[:5, 0] = [2.0 ** 60, 0.0, 128.0, 128.0, -(2.0 ** 60)]
    assert R.slab_sum_seq(s)[0] == 0.0 and R.slab_sum_grouped(s)[0] == 256.0
    assert R.slab_sum_grouped(s[:16])[0] == 0.0
    # NaN in an unused slot never reaches the sum of the used ones
    slabs[9:] = np.nan
    assert np.isfinite(R.slab_sum_seq(slabs[:9])).all()
