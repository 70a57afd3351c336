"""tests/link_ref.py (the fp64 restatements that tests/test_link_kernels_gpu.py holds the dense link kernels to) against the
golden-pinned oracle, the split restatement against its own claims, and the case tables against the launch arithmetic.  Both sides of
every pin are fp64 NumPy: agreement to 1e-12 relative, no entry left out.  No GPU.

Mutations of link_ref.py, each tried against this file and reverted: dropping the `lam` factor of g1 in link_cells fails
test_pass_ref_reproduces_the_pnlpf_updates; selecting |r| (sums[0]) or r^2 (sums[1]) by the observed pattern in sums_ref fails
test_sums_ref_is_the_oracle_scores_whatever_the_pattern; writing the KL term as X log(X / P) - X + P without the zero rule fails
test_sums_ref_kl_objective_is_wnmf_kl_error (nan from 0 log 0)."""
import numpy as np
import pytest

import link_ref as R
import oracle as orc

RTOL = 1e-12


def close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * scale, err_msg=what)


def pattern(rs, shape):
    return (rs.rand(*shape) < 0.6).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pins
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_sigmoid_parts_is_the_stable_sigmoid():
    S = np.concatenate([np.linspace(-700, 700, 2801), [-1e-3, 0.0, 1e-3, 36.0, 37.0, 38.0]])
    sig, d = R.sigmoid_parts(S)
    np.testing.assert_allclose(sig, orc.stable_sigmoid(S), rtol=RTOL, atol=0)
    near = np.abs(S) < 6.9                       # where 1 - sig keeps twelve digits
    np.testing.assert_allclose(d[near], (sig * (1 - sig))[near], rtol=RTOL, atol=0)
    # beyond S ~ 37 the fp64 product sig (1 - sig) is 0; d is exp(-|S|) to the last digit there
    far = S >= 38.0
    assert ((sig * (1 - sig))[far] == 0).all() and (d[np.abs(S) < 700] > 0).all()
    np.testing.assert_allclose(d[far], np.exp(-S[far]), rtol=1e-15, atol=0)
    assert np.array_equal(d, R.sigmoid_parts(-S)[1])


@pytest.mark.parametrize("lam", [1.0, 10.0])
def test_pass_ref_reproduces_the_pnlpf_updates(lam):
    rs = np.random.RandomState(11)
    m, n, k = 37, 45, 6
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    U = np.sqrt(0.5 / k) * (1 + rs.rand(m, k) - 0.5)
    V = np.sqrt(0.5 / k) * (1 + rs.rand(n, k) - 0.5)
    assert np.abs(lam * (U @ V.T - 0.5)).max() < 6.9       # the oracle's own sig (1 - sig) is good to 1e-12 here
    num, den = R.pass_ref(X, U, V, R.LINK_SIGMOID, lam)
    numv, denv = R.pass_ref(X.T, V, U, R.LINK_SIGMOID, lam)
    close(U * (num / den), orc.pnlpf_update_U(X, None, U, V, 0.0, lam), "pnlpf_update_U at reg = 0")
    close(V * (numv / denv), orc.pnlpf_update_V(X, None, U, V, 0.0, lam), "pnlpf_update_V at reg = 0")
    sig = orc.pnlpf_prediction(U, V, lam)       # the pieces themselves, not only their quotient
    d = sig * (1 - sig)
    close(num, lam * (X * d) @ V, "num")
    close(den, lam * (sig * d) @ V, "den")
    close(numv, lam * (X * d).T @ U, "num^T")
    close(denv, lam * (sig * d).T @ U, "den^T")


def test_pass_ref_reproduces_one_wnmf_kl_update():
    rs = np.random.RandomState(12)
    m, n, k = 37, 45, 5
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    U0, V0 = rs.rand(m, k) + 0.05, rs.rand(n, k) + 0.05
    Uo, Vo = orc.wnmf_kl_update(X, None, U0, V0)           # V first, then U with the new V
    numv, denv = R.pass_ref(X.T, V0, U0, R.LINK_KL, 0.0)
    assert denv is None
    V1 = V0 * (numv / R.colsum_ref(U0))                    # the denominator O^T U: the column sums of U
    close(V1, Vo, "V after one update")
    num, _ = R.pass_ref(X, U0, V1, R.LINK_KL, 0.0)
    close(U0 * (num / R.colsum_ref(V1)), Uo, "U after one update")
    close(numv, (X / (U0 @ V0.T)).T @ U0, "numerator of V")
    close(num, (X / (U0 @ V1.T)) @ V1, "numerator of U")
    close(R.colsum_ref(U0), (np.ones((1, m)) @ U0)[0], "column sums")
    # RULE kl_zero_product: a zero factor row under x = 1 cells adds nothing and divides by nothing
    Uz = U0.copy()
    Uz[3] = 0.0
    assert X[3].sum() > 0
    with np.errstate(all="raise"):
        numz, _ = R.pass_ref(X, Uz, V0, R.LINK_KL, 0.0)
        numzv, _ = R.pass_ref(X.T, V0, Uz, R.LINK_KL, 0.0)
    keep = np.arange(m) != 3
    assert (numz[3] == 0).all() and np.array_equal(numz[keep], R.pass_ref(X[keep], Uz[keep], V0, R.LINK_KL, 0.0)[0])
    close(numzv, R.pass_ref(X[keep].T, V0, Uz[keep], R.LINK_KL, 0.0)[0], "the zero row adds nothing to the other factor's numerator")


@pytest.mark.parametrize("link,lam", [(R.LINK_SIGMOID, 10.0), (R.LINK_KL, 0.0)])
def test_sums_ref_is_the_oracle_scores_whatever_the_pattern(link, lam):
    rs = np.random.RandomState(13)
    m, n, k = 37, 45, 6
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    U, V = rs.rand(m, k) * 0.6 + 0.05, rs.rand(n, k) * 0.6 + 0.05
    pred = orc.pnlpf_prediction(U, V, lam) if link == R.LINK_SIGMOID else orc.real_product(U, V)
    rmse, mae = orc.rmse_mae(X, pred)
    for O in (None, pattern(rs, (m, n)), np.zeros((m, n))):
        s = R.sums_ref(X, U, V, link, lam, O)
        assert s[0] == pytest.approx(mae * m * n, rel=RTOL) and s[1] == pytest.approx(rmse ** 2 * m * n, rel=RTOL)
        if link == R.LINK_SIGMOID:
            assert s[2] == 0.0
            assert 0.5 * s[1] == pytest.approx(orc.rec_term(X, pred, None), rel=RTOL)


def test_sums_ref_kl_objective_is_wnmf_kl_error():
    rs = np.random.RandomState(14)
    m, n, k = 37, 45, 5
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    U, V = rs.rand(m, k) + 0.05, rs.rand(n, k) + 0.05
    O = pattern(rs, (m, n))
    # (the oracle turns the zeros of X into eps first, as the reference does: 1e-14 relative to a cell's p, inside the gate)
    assert R.sums_ref(X, U, V, R.LINK_KL, 0.0)[2] == pytest.approx(orc.wnmf_kl_error(X.copy(), None, U, V), rel=RTOL)
    assert R.sums_ref(X, U, V, R.LINK_KL, 0.0, O)[2] == pytest.approx(orc.wnmf_kl_error(X.copy(), O, U, V), rel=RTOL)
    assert R.sums_ref(X, U, V, R.LINK_KL, 0.0, np.zeros((m, n)))[2] == 0.0
    assert abs(R.sums_ref(X, U, V, R.LINK_KL, 0.0, O)[2] - R.sums_ref(X, U, V, R.LINK_KL, 0.0)[2]) > 1.0     # the pattern matters
    # RULE kl_floor: p = 0 under x = 1 gives -1 - log(1e-37), under x = 0 it gives 0
    t = R.kl_cells(np.array([1.0, 0.0]), np.array([0.0, 0.0]))
    assert t[0] == pytest.approx(-1.0 - np.log(1e-37), rel=1e-15) and t[1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the split restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_rounding_restatements_agree_with_an_independent_conversion():
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(15)
    x = (rs.standard_normal(20000) * np.ldexp(1.0, rs.randint(-30, 30, size=20000))).astype(np.float32)
    x[:6] = [0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39]      # ties to even both ways, a subnormal
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    assert np.array_equal(R.bf16_value(want).view(np.uint32), want.astype(np.uint32) << 16)
    y = (x * np.float32(2.0 ** -16)).astype(np.float32)                       # into the fp16 range, subnormals included
    assert np.array_equal(y.astype(np.float16).view(np.uint16), torch.from_numpy(y).to(torch.float16).view(torch.int16).numpy().view(np.uint16))


def test_the_permutation_is_a_bijection_on_every_32_row_block():
    for rows_pad in R.SPLIT_ROWS:
        src = R.perm_rows(rows_pad).reshape(rows_pad // 32, 32)
        assert np.array_equal(np.sort(src, axis=1), np.arange(rows_pad).reshape(-1, 32))
    # position (q, h, t) holds row (r & 3) + 8 (r >> 2) + 4 h with r = 8 q + t
    src = R.perm_rows(64)
    for q in range(2):
        for h in range(2):
            for t in range(8):
                r = 8 * q + t
                assert src[1, q, h, t] == 32 + (r & 3) + 8 * (r >> 2) + 4 * h


@pytest.mark.parametrize("name", R.SPLIT_SETS)
@pytest.mark.parametrize("kp", [32, 64])
def test_split_words_reproduce_the_factor_to_the_claimed_bits(kp, name):
    A, B = R.split_factor(128, kp, name, 0), R.split_factor(32, kp, name, 1)
    S, T, invC = R.pair_scales(A, B)
    a, b = R.column_maxima(A).astype(np.float64), R.column_maxima(B).astype(np.float64)
    live = (a > 0) & (b > 0)
    if name == "zero":
        assert not live.any() and invC == 1.0 and not S.any() and not T.any()
    else:
        assert live.sum() == kp - (2 if name == "dead" else 0)
        C = (S.astype(np.float64) * T)[live]
        assert (C == 1.0 / float(invC)).all()                               # S_k T_k = C for every live pair
        assert ((a * S)[live] >= 2.0 ** 14).all() and ((a * S)[live] < 2.0 ** 15).all() and ((b * T)[live] <= 2.0 ** 15).all()
        assert (b * T)[live].max() >= 2.0 ** 13                             # the dominant pair uses the range in both factors
    wa, wb = R.split_words(A, S), R.split_words(B, T)
    va16, vab = R.split_values(wa, kp, S)
    vb16, vbb = R.split_values(wb, kp, T)
    # fp16 pair: 2^-22 of the column's maximum (hi to 2^-11, lo to 2^-11 of what is left); in factor B, whose columns sit lower, also
    # the subnormal spacing 2^-25 of a scaled entry -- times a_k S_k <= 2^15 that is 2^-10 / C of the product
    assert (np.abs(va16 - A)[:, live] <= 2.0 ** -22 * a[live]).all()
    assert (np.abs(vb16 - B)[:, live] * a[live] <= 2.0 ** -22 * (a * b)[live] + 2.0 ** -10 * float(invC)).all()
    assert not va16[:, ~live].any() and not vb16[:, ~live].any()           # RULE dead_column
    for w, s in ((wa, S), (wb, T)):
        dead = np.broadcast_to(s == 0, (w["hi"].size // kp, kp)).ravel()
        assert not w["hi"][dead].any() and not w["lo"][dead].any()
    # bf16 pair: 2^-16 of the entry itself (in fact 2^-18), dead columns included -- the contraction does not use the scales
    assert (np.abs(vab - A) <= 2.0 ** -16 * np.abs(A)).all() and (np.abs(vbb - B) <= 2.0 ** -16 * np.abs(B)).all()
    if name == "span":
        lo = wb["lo"].view(np.float16).astype(np.float64)
        assert ((lo != 0) & (np.abs(lo) < 2.0 ** -14)).any()               # the case really has subnormal lo addends
    # the single scale of bmf_link_split
    head, S1 = R.single_header(A)
    mx = float(np.abs(A).max())
    if mx > 0:
        assert 2.0 ** 14 <= mx * float(S1) < 2.0 ** 15
        v16, _ = R.split_values(R.split_words(A, S1), kp, S1)
        assert (np.abs(v16 - A) <= 2.0 ** -22 * mx).all()
    else:
        assert S1 == 1.0 and head.tolist() == [R.f32_word(1.0), R.f32_word(1.0), 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case tables reach every launch path
# ---------------------------------------------------------------------------------------------------------------------------------------
def plans(transposed=False):
    return [R.pass_plan(c, r) if transposed else R.pass_plan(r, c) for r, c, _ in R.PASS_CASES]


def test_case_table_reaches_every_launch_path():
    P = plans()
    one_slab = {p["slabs"][0] for p in P if p["splits"] == 1}
    assert 1 in one_slab                                                    # prologue and epilogue alone, fetch(min(1, ntile - 1)) clamped
    assert 2 in one_slab                                                    # one trip of the loop
    assert 3 in one_slab                                                    # the ring of three buffers used once each
    assert 4 in one_slab                                                    # the first wrap of the ring
    assert 7 in one_slab                                                    # two wraps and one more
    assert any(p["slabs"] == [9, 9] for p in P)                             # two equal slabs
    assert any(p["splits"] >= 3 and p["slabs"][-1] < p["slabs"][0] for p in P)      # three or more slabs, a shorter last one
    assert any(p["slabs"] == [9, 8] for p in P)                             # two slabs, the second shorter
    assert {p["row_blocks"] for p in P} == {1, 2}                           # 1 and 2 row blocks
    assert {0, 31, 32, 127} <= {p["last_row_pos"] for p in P}               # the last valid row at 0, 31, 32 and 127 of its block
    assert any(p["row_blocks"] == 2 and p["last_row_pos"] == 0 for p in P)  # a second block holding one row
    assert {1, 16, 17, 31, 32} <= {p["ragged"] for p in P}                  # valid columns of the last column tile
    ks = {(R.kp_of(k), k < R.kp_of(k)) for _, _, k in R.PASS_CASES}
    assert ks == {(32, True), (32, False), (64, True), (64, False)}         # kp 32 and 64, with k < kp and k = kp
    # the other orientation (rows and cols swapped, X^T) adds row blocks up to 33 and keeps to one slab
    T = plans(transposed=True)
    assert max(p["row_blocks"] for p in T) == 33 and all(p["splits"] == 1 for p in T) and {1, 2, 4, 5} <= {p["slabs"][0] for p in T}


def test_case_table_matches_the_shapes_the_split_rule_was_read_for():
    for r in R.GRID_ROWS:
        for c, tiles in zip(R.GRID_COLS, (1, 2, 3, 4, 5, 7)):
            assert R.pass_plan(r, c)["slabs"] == [tiles]
    assert R.pass_plan(130, 545)["slabs"] == [9, 9]
    assert R.pass_plan(130, 515)["slabs"] == [9, 8]
    assert R.pass_plan(130, 4100)["slabs"] == [9] * 14 + [3]
    # the rule itself at sizes where it decides differently: a full last round ends the search early
    assert R.splits_for(100000, 20000) == 3 and R.splits_for(20000, 100000) == 3 and R.splits_for(128 * 512, 4096) == 1


def test_colsum_table_reaches_every_choice_of_partial_blocks():
    got = {(rows, out): R.colsum_blocks(rows, out) for rows in R.COLSUM_ROWS for out in R.COLSUM_OUT_ROWS}
    assert got[(1, 2)] == (1, 1) and got[(63, 128)] == (1, 63) and got[(64, 128)] == (1, 64)      # one block
    assert got[(65, 128)] == (2, 33) and got[(129, 128)] == (3, 43)                                  # one block per 64 rows, a short last one
    assert got[(129, 2)] == (1, 129) and got[(33000, 2)] == (1, 33000)                               # limited by out_rows / 2
    assert got[(33000, 128)] == (64, 516)                                                            # limited by out_rows / 2, many blocks
    assert got[(33000, 1152)] == (508, 65)                                                           # limited by 512, then spread evenly
    assert all(R.colsum_blocks(rows, 1) is None for rows in R.COLSUM_ROWS)                           # out_rows = 1 is refused
    assert all(v is not None and 2 * v[0] <= max(out, 2) for (rows, out), v in got.items())         # the partials fit into `out`


def test_localisation_table_hits_every_position_and_every_tile():
    i = np.arange(R.LOCAL_ROWS)
    for tiles in R.LOCAL_TILES:
        pi = R.local_pi(tiles)
        assert pi.min() >= 0 and pi.max() < 32 * tiles
        assert len({(r, c) for r, c in zip(i % 32, pi % 32)}) == 1024        # every (row, column) position of the 32 x 32 tile
        assert set(pi // 32) == set(range(tiles))                            # every tile index of the sweep
        for wave_rows in range(0, R.LOCAL_ROWS, 32):                         # every wave sees every tile index but never a full row of ones
            assert set(pi[wave_rows:wave_rows + 32] // 32) == set(range(tiles))
        assert R.pass_plan(R.LOCAL_ROWS, 32 * tiles)["slabs"] == [tiles]


# ---------------------------------------------------------------------------------------------------------------------------------------
# no case is degenerate
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,k", R.PASS_CASES)
def test_cases_are_not_degenerate(rows, cols, k):
    X = R.make_X(rows, cols)
    both = lambda a: a.size < 2 or (a.any() and not a.all())
    assert both(X[rows - 1]) and both(X[:, cols - 1]) and both(X[:, 32 * ((cols - 1) // 32):])      # last row, last column, ragged tile
    assert X[rows - 1, cols - 1] == 1 and X[0, 0] == 1
    if R.empty_row(rows) is not None:
        assert not X[R.empty_row(rows)].any() and R.empty_row(rows) not in (0, rows - 1)
    # saturation: at lam = 300 cells beyond |s| = 40 on both sides, cells near 0, and cells past the exp2 clamp (s < -100 ln 2)
    U, V = R.make_factors(rows, cols, k, "saturating")
    s = 300.0 * (U.astype(np.float64) @ V.astype(np.float64).T - 0.5)
    assert abs(s[0, 0]) < 1e-3
    if rows >= 32 and cols >= 33:
        assert (s > 40).any() and (s < -40).any() and (np.abs(s) < 2).any() and (s < -70).any()
        P = s / 300.0 + 0.5
        assert P.min() < 0.05 and P.max() > 1.5
    # KL: an all-zero factor row with x = 1 cells in it, in both orientations; every other product is positive and clear of P's error
    U, V = R.make_factors(rows, cols, k, "zero_rows")
    assert not U[R.ZROW].any() and not V[R.ZCOL].any() and X[R.ZROW].sum() >= 1 and X[:, R.ZCOL].sum() >= 1
    for name in ("moderate", "unbalanced", "zero_rows"):
        U, V = (a.astype(np.float64) for a in R.make_factors(rows, cols, k, name))
        P = U @ V.T
        zero = np.zeros_like(P, dtype=bool)
        if name == "zero_rows":
            zero[R.ZROW], zero[:, R.ZCOL] = True, True
        assert (P[zero] == 0).all() and (P[~zero] > 4 * R.P_REL * R.product_scale(U, V)).all()
        if name == "unbalanced":
            assert not U[:, 1].any() and V[:, 1].all()                      # a dead column pair
            au, av = np.abs(U).max(0), np.abs(V).max(0)                     # two lopsided pairs, one each way round
            assert au[0] < 1e-3 * au.max() and av[0] > 1e3 * np.median(av) and au[k - 1] > 1e3 * np.median(au) and av[k - 1] < 1e-3 * av.max()
