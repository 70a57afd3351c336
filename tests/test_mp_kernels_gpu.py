"""The kernels of MessagePassing (csrc/mp.hip) against the NumPy restatement (tests/mp_ref.py): the cell pass bit for bit on every
register tier, the sums within the bound of two summation orders, the decisions, and the counter-based start bit for bit."""
import numpy as np
import pytest

import mp_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 65), (33, 130), (70, 64), (129, 257)]
KS = [1, 2, 3, 8, 9, 16, 17, 33, 64]
U53 = 2.0 ** -53


def pattern_70(m, n, rs):
    """70 % of the cells, one empty row and one empty column."""
    pat = rs.rand(m, n) < 0.7
    pat[rs.randint(m)] = False
    pat[:, rs.randint(n)] = False
    return pat


make_engine = R.make_engine


def load_state(eng, Xi, Ups, PhiH, PsiH):
    """The oracle's arrays (m, k), (n, k), (m, n, k) into the engine's layout; the padding columns stay 0."""
    import torch
    n = eng.n
    eng.Phi.zero_()
    eng.Psi.zero_()
    eng.Ups.zero_()
    eng.Phi[:, :, :n] = torch.from_numpy(np.ascontiguousarray(PhiH.transpose(2, 0, 1))).to(eng.device)
    eng.Psi[:, :, :n] = torch.from_numpy(np.ascontiguousarray(PsiH.transpose(2, 0, 1))).to(eng.device)
    eng.Xi.copy_(torch.from_numpy(np.ascontiguousarray(Xi)).to(eng.device))
    eng.Ups[:, :n] = torch.from_numpy(np.ascontiguousarray(Ups.T)).to(eng.device)
    eng._started = True


def random_state(m, n, k, scale, pattern, rs, ties=False):
    if scale == 0:
        return np.zeros((m, k)), np.zeros((n, k)), np.zeros((m, n, k)), np.zeros((m, n, k))
    Xi, Ups = scale * rs.standard_normal((m, k)), scale * rs.standard_normal((n, k))
    PhiH, PsiH = scale * rs.standard_normal((m, n, k)), scale * rs.standard_normal((m, n, k))
    if ties and k >= 2:      # factor 1 repeats factor 0 and both lead: Gamma_0 == Gamma_1 are the two top values of (nearly) every cell
        Xi[:, 0] += 10 * scale
        Ups[:, 0] += 10 * scale
        for A in (Xi, Ups, PhiH, PsiH):
            A[..., 1] = A[..., 0]
    if pattern is not None:
        PhiH, PsiH = PhiH * pattern[:, :, None], PsiH * pattern[:, :, None]
    return Xi, Ups, PhiH, PsiH


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_step(eng, X, pattern, state, what):
    Xi, Ups, PhiH, PsiH = state
    load_state(eng, Xi, Ups, PhiH, PsiH)
    d = eng.step()
    A, B = R.cell_pass(X, pattern, Xi, Ups, PhiH, PsiH, eng.co1, eng.co0, eng.lr)
    gA, gB = eng.messages()
    assert same_bytes(gA, A) and same_bytes(gB, B), (what, float(np.abs(gA - A).max()), float(np.abs(gB - B).max()))
    assert not eng.Phi[:, :, eng.n:].any().item() and not eng.Psi[:, :, eng.n:].any().item(), what      # the padding columns
    if pattern is not None:
        assert not gA[~pattern].any() and not gB[~pattern].any(), what
    return d, A, B


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m,n", SHAPES)
def test_cell_pass_bit_for_bit(m, n, k):
    rs = np.random.RandomState(1000 * m + 10 * n + k)
    X = rs.rand(m, n) < 0.4
    for pattern in (None, pattern_70(m, n, rs)):
        eng = make_engine(X, k, pattern)
        for scale in (1e-2, 1.0, 30.0, 0):
            check_step(eng, X, pattern, random_state(m, n, k, scale, pattern, rs), (m, n, k, pattern is not None, scale))
        if k >= 2:
            state = random_state(m, n, k, 1.0, pattern, rs, ties=True)
            G = R.mn(R.mn((state[0][:, None] - state[2]) + (state[1][None] - state[3]), state[0][:, None] - state[2]), state[1][None] - state[3])
            assert (G[..., 0] == G[..., 1]).all() and (G[..., 0] == G.max(axis=2)).any()                       # equal top values do occur
            check_step(eng, X, pattern, state, (m, n, k, pattern is not None, "ties"))


@pytest.mark.parametrize("k", [3, 16, 33])
@pytest.mark.parametrize("value", [0, 1])
def test_cell_pass_on_constant_matrices(k, value):
    m, n = 33, 130
    rs = np.random.RandomState(50 + k + value)
    X = np.full((m, n), bool(value))
    for pattern in (None, pattern_70(m, n, rs)):
        eng = make_engine(X, k, pattern)
        check_step(eng, X, pattern, random_state(m, n, k, 1.0, pattern, rs), (k, value))


def sum_bounds(PhiH, PsiH, cx, cy):
    """2 (N - 1) 2^-53 sum |terms| per marginal, N = the hats of the row / column and the prior: the bound on the difference of two
    summation orders of the same N terms (each order is within (N - 1) u sum |terms| of the exact sum)."""
    m, n, _ = PhiH.shape
    return (2 * n * U53 * (np.abs(PhiH).sum(axis=1) + abs(cx)), 2 * m * U53 * (np.abs(PsiH).sum(axis=0) + abs(cy)))


def check_marginals(eng, PhiH, PsiH, Xi_old, Ups_old, d, what):
    Xi, Ups = R.marginals(PhiH, PsiH, eng.cx, eng.cy)
    bx, bu = sum_bounds(PhiH, PsiH, eng.cx, eng.cy)
    gXi, gUps = eng.marginals()
    ex, eu = np.abs(gXi - Xi), np.abs(gUps - Ups)
    print(f"{what}: |Xi - oracle| max {ex.max():.3e} (bound {bx.max():.3e}), |Ups - oracle| max {eu.max():.3e} (bound {bu.max():.3e})")
    assert (ex <= bx).all() and (eu <= bu).all(), what
    d_ref = max(np.abs(Xi - Xi_old).max(), np.abs(Ups - Ups_old).max())
    assert abs(d - d_ref) <= max(bx.max(), bu.max()) + 2 * U53 * d_ref, (what, d, d_ref)
    # d is exactly the largest change of the kernel's own marginals
    assert d == max(np.abs(gXi - Xi_old).max(), np.abs(gUps - Ups_old).max()), what
    U, V = eng.decisions()
    assert np.array_equal(U, gXi > 0) and np.array_equal(V, gUps > 0), what


@pytest.mark.parametrize("k", [1, 9, 16, 64])
@pytest.mark.parametrize("m,n", SHAPES)
def test_sums_d_and_decisions(m, n, k):
    import torch
    from pybmf_amd._lib import check, lib, ptr
    rs = np.random.RandomState(7 * m + n + k)
    X = rs.rand(m, n) < 0.4
    for pattern in (None, pattern_70(m, n, rs)):
        eng = make_engine(X, k, pattern)
        for scale in (1e-2, 30.0):
            Xi, Ups, PhiH, PsiH = random_state(m, n, k, scale, pattern, rs)
            # bmf_mp_reduce on the hats as they stand
            load_state(eng, Xi, Ups, PhiH, PsiH)
            with torch.cuda.device(eng.device):
                check(lib.bmf_mp_reduce(ptr(eng.Phi), ptr(eng.Psi), m, n, k, eng.ldn, eng.cx, eng.cy, ptr(eng.work), ptr(eng.Xi), ptr(eng.Ups),
                                        ptr(eng._d_dev), ptr(eng.ubits), ptr(eng.vbits), eng._stream), "bmf_mp_reduce")
                d = float(eng._d_dev.cpu().numpy()[0])
            check_marginals(eng, PhiH, PsiH, Xi, Ups, d, ("reduce", m, n, k, pattern is not None, scale))
            # ... and the sums a step leaves, of the hats it wrote
            d, A, B = check_step(eng, X, pattern, (Xi, Ups, PhiH, PsiH), ("step", m, n, k))
            check_marginals(eng, A, B, Xi, Ups, d, ("step", m, n, k, pattern is not None, scale))


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 12345])
@pytest.mark.parametrize("masked", [False, True])
def test_start_is_the_hash_fill(seed, masked):
    m, n, k = 33, 130, 5
    rs = np.random.RandomState(3)
    X = rs.rand(m, n) < 0.4
    pattern = pattern_70(m, n, rs) if masked else None
    eng = make_engine(X, k, pattern)
    eng.Phi.fill_(7.0)         # start() writes every plane element, the padding included
    eng.Psi.fill_(7.0)
    eng.start(seed)
    Ph, Ps = R.start_hats(m, n, k, seed, eng.init_scale, pattern)
    gA, gB = eng.messages()
    assert same_bytes(gA, Ph) and same_bytes(gB, Ps)
    assert not eng.Phi[:, :, n:].any().item() and not eng.Psi[:, :, n:].any().item()
    Xi, Ups = R.marginals(Ph, Ps, eng.cx, eng.cy)
    bx, bu = sum_bounds(Ph, Ps, eng.cx, eng.cy)
    gXi, gUps = eng.marginals()
    assert (np.abs(gXi - Xi) <= bx).all() and (np.abs(gUps - Ups) <= bu).all()


def test_engine_refuses_what_does_not_fit(monkeypatch):
    import torch
    X = np.zeros((8, 8), dtype=bool)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 1 << 40))
    need = 2 * 8 * 64 * 3 * 8 + 8 * (1 * 8 * 3 + 1 * 3 * 64 + 1 + 1)
    with pytest.raises(NotImplementedError, match=f"take {need} bytes"):
        make_engine(X, 3, None)
