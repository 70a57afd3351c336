"""tests/objective_ref.py proved on the CPU: the exact inputs are exact in every number format and summation order the kernels use,
the references agree with the oracle's dense definitions and with the reference's own numbers (golden g4), the bit packers agree with
tests/bits_ref.py, and the restated launch arithmetic gives the paths the GPU tests name."""
import json
import os

import numpy as np
import pytest

import bits_ref as br
import objective_ref as R
import oracle as orc

SHAPES = [(130, 70, 27), (130, 70, 61), (20, 70, 5), (300, 200, 8), (257, 129, 64), (64, 64, 1)]


def bf16_hi(a32):
    """round-to-nearest-even bf16 of fp32 values, as fp32"""
    u = np.ascontiguousarray(a32, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return r.view(np.float32)


@pytest.mark.parametrize("rows,k,salt", [(130, 27, 1), (70, 61, 4), (300, 1, 2), (1000, 64, 5), (5000, 8, 1)])
def test_exact_factors_survive_every_operand_format(rows, k, salt):
    F = R.exact_factor(rows, k, salt)
    assert F.min() >= 0 and (k <= 4 or F.min() == 0) and F.max() <= 1 and np.array_equal(F * 8, np.rint(F * 8))
    nz = (F != 0).sum(1)
    assert nz.min() >= 1 and nz.max() <= 4 and (F[:, k - 1] != 0).all()
    assert set(np.nonzero(F.any(0))[0]) == set(range(k))            # every latent column is used by some row
    f32 = F.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), F)
    for scale in (1.0, -2.0):                                       # the MAE kernels scale U by -X_ONE = -2
        assert np.array_equal((f32 * np.float32(scale)).astype(np.float16).astype(np.float64), F * scale)
        hi = bf16_hi(f32 * np.float32(scale))
        assert np.array_equal(hi.astype(np.float64), F * scale)    # the bf16 hi part is the value, so the lo part is zero
        assert not (f32 * np.float32(scale) - hi).any()
    # the values differ from row to row: no two neighbouring rows are equal
    assert (np.abs(np.diff(F, axis=0)).sum(1) > 0).all()


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_exact_sums_in_fp32_any_order_and_fp64(m, n, k):
    c = R.exact_case(m, n, k)
    X = R.x_block(np.arange(m), np.arange(n))
    U32, V32 = c["U"].astype(np.float32), c["V"].astype(np.float32)
    # the product in fp32, latent dimension forwards and backwards, and in fp64
    P1 = np.zeros((m, n), np.float32)
    P2 = np.zeros((m, n), np.float32)
    for l in range(k):
        P1 += U32[:, l:l + 1] * V32[:, l][None, :]
        P2 += U32[:, k - 1 - l:k - l] * V32[:, k - 1 - l][None, :]
    P64 = c["U"] @ c["V"].T
    assert np.array_equal(P1, P2) and np.array_equal(P1.astype(np.float64), P64)
    assert P64.max() <= 4 and np.array_equal(P64 * 64, np.rint(P64 * 64))
    r = X.astype(np.float32) - P1
    assert np.abs(r).max() <= 4
    # a lane's partial: 64 consecutive cells (the longest any kernel keeps in fp32), forwards and backwards, |r| (and 2 |r|, the MAE
    # kernels' X_ONE scale) by additions, r^2 by an fma chain (emulated: every partial of the chain is checked to be representable)
    flat = np.concatenate([r.ravel(), np.zeros((-r.size) % 64, np.float32)]).reshape(-1, 64)
    tot = {}
    for name, order in (("fwd", range(64)), ("bwd", range(63, -1, -1))):
        a = np.zeros(flat.shape[0], np.float32)
        a2 = np.zeros(flat.shape[0], np.float32)
        s = np.zeros(flat.shape[0], np.float32)
        s64 = np.zeros(flat.shape[0])
        for e in order:
            a = a + np.abs(flat[:, e])
            a2 = a2 + np.float32(2) * np.abs(flat[:, e])
            s64 = s64 + flat[:, e].astype(np.float64) ** 2
            s = s64.astype(np.float32)
            assert np.array_equal(s.astype(np.float64), s64)        # the fma chain never rounds
        assert np.array_equal(a2, 2 * a)
        tot[name] = (float(a.astype(np.float64).sum()), float(s.astype(np.float64).sum()))
    assert tot["fwd"] == tot["bwd"] == (c["s_abs"], c["s_sq"])
    R64 = X.astype(np.float64) - P64
    assert (float(np.abs(R64).sum()), float((R64 * R64).sum())) == (c["s_abs"], c["s_sq"])
    assert R.dense_sums(R.x_block, m, n, c["U"], c["V"], chunk=37) == (c["s_abs"], c["s_sq"])     # the chunking does not matter


def test_a_wrong_pairing_of_bits_and_product_cells_moves_the_sum():
    m, n, k = 130, 70, 27
    c = R.exact_case(m, n, k)
    X = R.x_block(np.arange(m), np.arange(n)).astype(np.float64)
    P = c["U"] @ c["V"].T
    base = np.abs(X - P).sum()
    assert base == c["s_abs"]
    for Xw in (np.roll(X, 1, axis=1), np.roll(X, 1, axis=0), np.roll(X, 4, axis=1), np.roll(X, 32, axis=0), X[::-1], X[:, ::-1]):
        assert np.abs(Xw - P).sum() != base
    sq = X[:64, :64]
    assert np.abs(sq.T - P[:64, :64]).sum() != np.abs(sq - P[:64, :64]).sum()
    # one cell dropped or counted twice, anywhere: the sum moves unless the cell's residual is 0, which is rare
    assert (np.abs(X - P) == 0).mean() < 0.05
    assert 0.25 < X.mean() < 0.375 and len(np.unique(np.abs(X - P))) > 60


def test_bit_packers():
    m, n = 130, 70
    X = R.x_block(np.arange(m), np.arange(n))
    w = R.x_words(m, n, 256, 4)
    assert np.array_equal(w[:m, :4], br.pack_rows(X, n)[:, :4]) and not w[m:].any()
    assert np.array_equal(np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:m, :n], X)
    assert np.array_equal(R.x_words(m, n, 256, 4, chunk=7), w)
    p = R.x_words(m, n, 256, 4, poison=True)
    bits = np.unpackbits(p.view(np.uint8), axis=1, bitorder="little")
    assert np.array_equal(bits[:m, :n], X) and bits[m:].all() and bits[:, n:].all()
    t = R.xt_words(m, n, 128, 8)
    assert np.array_equal(np.unpackbits(t.view(np.uint8), axis=1, bitorder="little")[:n, :m], X.T)
    assert br.popcount(t) == br.popcount(w) == int(X.sum())
    assert np.array_equal(R.xt_words(m, n, 128, 8, chunk=9), t)
    # the tiled copy: the index formula of the kernels that read it (csrc/mae.hip)
    rows, ld = 512, 32
    src = np.arange(rows * ld, dtype=np.uint32).reshape(rows, ld)
    til = R.tile_bits(src).ravel()
    j, wd = np.meshgrid(np.arange(rows), np.arange(ld), indexing="ij")
    idx = (((j >> 8) * (ld >> 4) + (wd >> 4)) * 256 + (j & 255)) * 16 + (wd & 15)
    assert np.array_equal(til[idx], src)
    F = R.pad_factor(np.ones((3, 2)), 5, 4, fill=7.0)
    assert np.array_equal(F, [[1, 1, 0, 0]] * 3 + [[7, 7, 7, 7]] * 2)


def test_real_x_is_exact_and_keeps_the_residual_bound():
    m, n, k = 150, 200, 27
    X = R.real_x(m, n)
    assert np.array_equal(X * 8, np.rint(X * 8)) and X.max() <= 1.875 and X.min() == 0
    c = R.exact_case(m, n, k)
    r = X - c["U"] @ c["V"].T
    assert np.abs(r).max() <= 4 and np.array_equal(r * 64, np.rint(r * 64))


def test_thresh_reference_against_the_oracle_and_golden_g4(golden_dir):
    z = np.load(os.path.join(golden_dir, "g4_threshold.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g4_threshold.json")))
    X = np.unpackbits(z["X_bits"], axis=1, bitorder="little")[:, :int(z["shape"][1])].astype(np.float64)
    for lam in (10, 100):
        for i, j in ((0, 0), (2, 3), (4, 4), (1, 4)):
            u, v = meta["grid_u"][i], meta["grid_v"][j]
            out, _ = R.thresh_ref(X, z["U"], z["V"], u, v, lam)
            assert float(out[1]) / 2 == pytest.approx(z[f"F_grid_lam{lam}"][i, j], rel=1e-12)
            assert float(out[1]) / 2 == pytest.approx(orc.thresh_F(X, None, z["U"], z["V"], u, v, lam), rel=1e-12)
            dF = orc.thresh_dF(X, None, z["U"], z["V"], u, v, lam)
            np.testing.assert_allclose(out[2:4].astype(np.float64), dF, rtol=1e-10, atol=1e-10 * np.abs(dF).max())
            np.testing.assert_allclose(out[2:4].astype(np.float64), z[f"dF_grid_lam{lam}"][i, j], rtol=1e-10,
                                       atol=1e-10 * np.abs(dF).max())
            Us = orc.stable_sigmoid((z["U"] - u) * lam)
            assert float(out[0]) == pytest.approx(np.abs(X - Us @ orc.stable_sigmoid((z["V"] - v) * lam).T).sum(), rel=1e-12)
    # fp64 instead of longdouble: the same numbers to fp64 accuracy
    o64, _ = R.thresh_ref(X, z["U"], z["V"], 0.4, 0.55, 100, dtype=np.float64)
    o80, _ = R.thresh_ref(X, z["U"], z["V"], 0.4, 0.55, 100)
    np.testing.assert_allclose(o64, o80.astype(np.float64), rtol=1e-12)


def test_sigmoid_pair_at_the_edges():
    lam = 10.0
    for x in (0.0, 0.375):
        F = R.transform_inputs(x, lam, np.float64)
        s, d = R.sigmoid_pair((F.astype(np.longdouble) - np.longdouble(x)) * lam, lam)
        assert np.isfinite(s).all() and np.isfinite(d).all() and (s >= 0).all() and (s <= 1).all() and (d >= 0).all()
        assert s[0] == 0.5 and d[0] == lam / 4
        z = (F - x) * lam
        small = np.abs(z) < 30
        np.testing.assert_allclose(d[small].astype(np.float64), orc.thresh_dXdx(F[small], x, lam), rtol=1e-13)
        np.testing.assert_allclose(s.astype(np.float64), orc.stable_sigmoid(z), rtol=1e-13, atol=1e-320)
    F0 = R.transform_inputs(0.0, lam, np.float64)
    assert F0[9] == 1e-300 and F0[10] == -1e-300 and F0[-2] > 0 > F0[-1] and abs(F0[-1]) == 5e-324


@pytest.mark.parametrize("m,n,k", [(150, 300, 1), (150, 300, 17), (150, 300, 33), (70, 45, 64)])
def test_saturated_thresholding_inputs_are_exact(m, n, k):
    c = R.sat_case(m, n, k)
    X = R.x_block(np.arange(m), np.arange(n))
    for dtype in (np.longdouble, np.float64):
        out, (Us, dUs, Vs, dVs) = R.thresh_ref(X, c["U"], c["V"], R.SAT_X, R.SAT_X, R.SAT_LAM, dtype=dtype)
        assert np.array_equal(Us.astype(np.float64), c["Us"]) and np.array_equal(dUs.astype(np.float64), c["dUs"])
        assert np.array_equal(Vs.astype(np.float64), c["Vs"]) and np.array_equal(dVs.astype(np.float64), c["dVs"])
        assert np.array_equal(out.astype(np.float64), c["out"])
    # the same inputs rounded to fp32 (bmf_thresh_eval takes fp32 factors) are the same numbers
    assert np.array_equal(c["U"].astype(np.float32).astype(np.float64), c["U"])
    assert set(np.unique(c["Us"])) <= {0.0, 0.5, 1.0} and c["out"][2] != 0 and c["out"][3] != 0
    assert np.array_equal(c["out"] * 16, np.rint(c["out"] * 16)) and c["out"][1] < 2.0 ** 30


def test_restated_launch_plans():
    # values worked out by hand from the rules in the docstrings
    assert R.residual_plan(130, 70) == (3, 1)             # 2 row blocks -> up to 512 groups, 3 tiles
    assert R.residual_plan(100, 27) == (1, 1)
    assert R.residual_plan(128, 65606) == (684, 3)        # 1 row block, 2051 tiles over 1024 groups: 3 each, 683 full + one of 2
    assert R.residual_plan(8192, 1083) == (12, 3)         # 64 row blocks -> 16 groups, 34 tiles: 3 each, 11 full + one of 1
    assert R.residual_plan(8192, 1051) == (11, 3)         # 33 tiles: no short group
    assert R.mae_plan(16384, 6400) == (34, 3) and R.mae_plan(16384, 3136) == (25, 2) and R.mae_plan(16384, 9280) == (37, 4)
    assert R.mae_plan(256 * 9, 128) == (2, 1)
    assert R.tiled_plan(64, 64 * 17) == (2, 9) and R.tiled_plan(192, 64 * 23) == (2, 12) and R.tiled_plan(192, 64 * 9) == (1, 9)
    assert R.tiled_plan(384, 1024) == (2, 8) and R.tiled_plan(64, 64) == (1, 1) and R.tiled_plan(64 * 2048, 64 * 64) == (1, 64)
