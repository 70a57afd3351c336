"""The incremental Boolean cover count: bmf_cover_delta (csrc/cover.hip) through the C ABI against NumPy on unpacked words, and the MU
loop that keeps running TP / FP totals (bmf_penalty_state.ubits_prev / vbits_prev) against the same loop with a full count per
iteration and against a NumPy recount from the factors.  Integers throughout: every count must be equal.

Kernel cases: rows 64 / 192 / 1024 (one block row; three; sixteen), words 4 / 12 / 124 (narrow chunks: lanes and segments masked),
128 / 640 (one chunk, one and three segments), 644 / 1284 (two and three chunk columns sharing their rows), kp 32 with k = 1, 8 and
kp 64 with k = 33, 64, and the dirty sets none / first row / last row / one row per wave / ~5 % / all.  Padding words hold ones, so a
read beyond `words` shows up in the counts.  Run with -s to see the per-iteration dirty fractions of the loop cases."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)


def popcount(a):
    """set bits per element of a uint32 array"""
    return POP16[a & 0xFFFF].astype(np.int64) + POP16[a >> 16]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib as L
    return L, torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def product_rows(u, colw, k):
    """P[i] = OR of colw[l] over the bits l set in u[i]: (rows, words) uint32"""
    P = np.zeros((u.shape[0], colw.shape[1]), np.uint32)
    for l in range(k):
        sel = ((u >> np.uint64(l)) & np.uint64(1)).astype(bool)
        P[sel] |= colw[l][None, :]
    return P


def random_words(rs, rows, k, density):
    bits = rs.rand(rows, k) < density
    return (bits.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def kernel_case(rows, words, kp, k):
    """X, the bit-columns, a new and an old word for EVERY row (all different), and each row's (TP, |P|) under either word."""
    rs = np.random.RandomState(1000 * rows + 10 * words + k)
    ld, ldcb = words + 4, words + 8
    X = np.full((rows, ld), 0xFFFFFFFF, np.uint32)
    X[:, :words] = rs.randint(0, 1 << 32, (rows, words), dtype=np.uint64).astype(np.uint32)
    colw = np.full((kp, ldcb), 0xFFFFFFFF, np.uint32)
    colw[:, :words] = (rs.randint(0, 1 << 32, (kp, words), dtype=np.uint64) & rs.randint(0, 1 << 32, (kp, words), dtype=np.uint64)
                       & rs.randint(0, 1 << 32, (kp, words), dtype=np.uint64)).astype(np.uint32)   # density 1/8
    new, old = random_words(rs, rows, k, 0.3), random_words(rs, rows, k, 0.3)
    old[new == old] ^= np.uint64(1)
    new[1], old[1] = np.uint64(0), old[1] | np.uint64(1)      # a word that goes to zero
    old[2], new[2] = np.uint64(0), new[2] | np.uint64(1)      # ... and one that comes from zero
    assert (new != old).all() and int(max(new.max(), old.max())) < (1 << k)
    per = {}
    for name, u in (("new", new), ("old", old)):
        P = product_rows(u, colw[:, :words], k)
        tp, pp = popcount(X[:, :words] & P).sum(axis=1), popcount(P).sum(axis=1)
        per[name] = (tp, pp - tp)
    for a in (X, colw, new, old):
        a.setflags(write=False)
    return dict(X=X, colw=colw, new=new, old=old, per=per, ld=ld, ldcb=ldcb)


def dirty_sets(rows):
    rs = np.random.RandomState(rows)
    per_wave = np.array([16 * ((5 * w) % (rows // 16)) + w for w in range(16)])   # row r belongs to wave r % 16 of its block
    some = np.flatnonzero(rs.rand(rows) < 0.05)
    return {"none": np.array([], np.int64), "first": np.array([0]), "last": np.array([rows - 1]), "per_wave": per_wave,
            "five_percent": some if some.size else np.array([rows // 2]), "all": np.arange(rows), "zero_words": np.array([1, 2])}


def call_delta(L, bits, ld, words, rows, rb, rbp, colw, ldcb, kp, counts, src=None, dst=None, n=0, stop=None):
    L.check(L.lib.bmf_cover_delta(L.ptr(bits), ld, words, rows, L.ptr(rb), L.ptr(rbp), L.ptr(colw), ldcb, kp, L.ptr(counts), L.ptr(src), L.ptr(dst), n,
                                  L.ptr(stop), stream()), "bmf_cover_delta")


ROWS, WORDS, KS = (64, 192, 1024), (4, 12, 124, 128, 640, 644, 1284), ((32, 1), (32, 8), (64, 33), (64, 64))


@pytest.mark.parametrize("kp,k", KS)
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("rows", ROWS)
def test_delta_kernel_exact(env, rows, words, kp, k):
    """counts += (TP(new) - TP(old), FP(new) - FP(old)) over exactly the rows whose word differs, for every dirty set; the copy lands,
    rowbits_prev stays; a set stop word moves nothing."""
    L, d = env
    c = kernel_case(rows, words, kp, k)
    X, colw, new = dev(c["X"]), dev(c["colw"]), dev(c["new"])
    (tp_n, fp_n), (tp_o, fp_o) = c["per"]["new"], c["per"]["old"]
    src = dev(np.arange(1, 778, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    for name, D in dirty_sets(rows).items():
        prev_h = c["new"].copy()
        prev_h[D] = c["old"][D]
        prev = dev(prev_h)
        want = (int((tp_n[D] - tp_o[D]).sum()), int((fp_n[D] - fp_o[D]).sum()))
        counts = torch.tensor([7, 11, 13, 17], dtype=torch.int64, device=d)
        dst = torch.full((777 + 3,), -5, dtype=torch.int64, device=d)
        call_delta(L, X, c["ld"], words, rows, new, prev, colw, c["ldcb"], kp, counts, src, dst, 777)
        got = counts.cpu().numpy()
        assert (int(got[0]) - 7, int(got[1]) - 11) == want and (got[2], got[3]) == (13, 17), (name, got, want)
        assert torch.equal(dst[:777], src) and (dst[777:] == -5).all(), name
        assert np.array_equal(prev.cpu().numpy().view(np.uint64), prev_h), name      # rowbits_prev is never written
        if name == "all":
            assert want != (0, 0) or k == 1
            stop = torch.ones(1, dtype=torch.int32, device=d)
            dst.fill_(-5)
            call_delta(L, X, c["ld"], words, rows, new, prev, colw, c["ldcb"], kp, counts, src, dst, 777, stop)
            assert np.array_equal(counts.cpu().numpy(), got) and (dst == -5).all()
            stop.zero_()
            call_delta(L, X, c["ld"], words, rows, new, prev, colw, c["ldcb"], kp, counts, None, None, 0, stop)   # stop word 0, no copy: counts again
            got2 = counts.cpu().numpy()
            assert (int(got2[0]) - 7, int(got2[1]) - 11) == (2 * want[0], 2 * want[1])


def test_changed_word_same_product(env):
    """Two identical bit-columns: a row that trades one for the other is dirty and contributes exactly zero."""
    L, d = env
    rows, words, kp, k = 192, 644, 32, 8
    c = kernel_case(rows, words, kp, k)
    colw_h = c["colw"].copy()
    colw_h[1] = colw_h[0]
    new_h, prev_h = c["new"].copy(), c["new"].copy()
    new_h[70], prev_h[70] = np.uint64(0b101), np.uint64(0b110)
    counts = torch.tensor([7, 11, 13, 17], dtype=torch.int64, device=d)
    call_delta(L, dev(c["X"]), c["ld"], words, rows, dev(new_h), dev(prev_h), dev(colw_h), c["ldcb"], kp, counts)
    assert counts.cpu().tolist() == [7, 11, 13, 17]


def test_negative_and_positive_blocks(env):
    """Rows of one block lose their whole product, rows of another gain one: the signed block totals meet in the 64-bit counters as
    two's complement, whether the sum ends above or below zero."""
    L, d = env
    rows, words, kp, k = 1024, 128, 64, 64      # 16 row groups of 64 rows at most: rows 0..63 and 320..383 are in different blocks
    c = kernel_case(rows, words, kp, k)
    (tp_n, fp_n), (tp_o, fp_o) = c["per"]["new"], c["per"]["old"]
    lose, gain = np.arange(3, 40), np.arange(330, 350)
    new_h, prev_h = c["new"].copy(), c["new"].copy()
    new_h[lose], prev_h[lose] = np.uint64(0), c["old"][lose] | np.uint64(1 << 40)
    prev_h[gain] = np.uint64(0)
    P_lose = product_rows(prev_h[lose], c["colw"][:, :words], k)
    tp_l = popcount(c["X"][lose, :words] & P_lose).sum()
    fp_l = popcount(P_lose).sum() - tp_l
    want = (int(tp_n[gain].sum() - tp_l), int(fp_n[gain].sum() - fp_l))
    assert want[0] < 0 and want[1] < 0 and tp_n[gain].sum() > 0
    X, colw, new, prev = dev(c["X"]), dev(c["colw"]), dev(new_h), dev(prev_h)
    for base in (0, 1 << 40):
        counts = torch.tensor([base, base, 13, 17], dtype=torch.int64, device=d)
        call_delta(L, X, c["ld"], words, rows, new, prev, colw, c["ldcb"], kp, counts)
        assert counts.cpu().tolist() == [base + want[0], base + want[1], 13, 17]


def pack_rows(B):
    """(rows, cols) 0/1 -> (rows, cols / 32) uint32, column 32 w + b at bit b of word w"""
    return np.ascontiguousarray(np.packbits(np.ascontiguousarray(B, dtype=np.uint8), axis=1, bitorder="little")).view(np.uint32)


def words_of(B):
    k = B.shape[1]
    return (B.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def cover_numpy(X, Ub, Vb):
    """(TP, FP) of the Boolean product of two 0/1 factor matrices against the 0/1 matrix X"""
    P = (Ub.astype(np.float32) @ Vb.astype(np.float32).T) > 0
    tp = int(np.count_nonzero(P & (X != 0)))
    return tp, int(np.count_nonzero(P)) - tp


def test_two_passes_equal_a_recount(env):
    """Column pass on X^T with U's old bit-columns, then row pass on X with V's new ones: their sum is TP / FP (new) - TP / FP (old)."""
    L, d = env
    m, n, k, kp = 256, 384, 20, 32
    rs = np.random.RandomState(5)
    X = (rs.rand(m, n) < 0.3).astype(np.uint8)
    Uo, Vo = rs.rand(m, k) < 0.08, rs.rand(n, k) < 0.08
    Un, Vn = Uo ^ (rs.rand(m, k) < 0.02), Vo ^ (rs.rand(n, k) < 0.02)
    colbits = lambda F: np.vstack([pack_rows(F.T), np.zeros((kp - k, F.shape[0] // 32), np.uint32)])   # noqa: E731
    counts = torch.zeros(4, dtype=torch.int64, device=d)
    call_delta(L, dev(pack_rows(X.T)), m // 32, m // 32, n, dev(words_of(Vn)), dev(words_of(Vo)), dev(colbits(Uo)), m // 32, kp, counts)
    call_delta(L, dev(pack_rows(X)), n // 32, n // 32, m, dev(words_of(Un)), dev(words_of(Uo)), dev(colbits(Vn)), n // 32, kp, counts)
    (tp1, fp1), (tp0, fp0) = cover_numpy(X, Un, Vn), cover_numpy(X, Uo, Vo)
    assert (tp1, fp1) != (tp0, fp0)
    assert counts.cpu().tolist() == [tp1 - tp0, fp1 - fp0, 0, 0]


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
ITERS = 40
SHAPES = {"narrow": (1000, 500, 8), "one_chunk": (2048, 20480, 64), "two_chunks": (1536, 20608, 64)}


@functools.lru_cache(maxsize=None)
def loop_problem(shape):
    """Planted factors + flip noise, and a start whose planted entries lie on both sides of the threshold over a noise floor: row words
    keep changing for tens of iterations at k = 8, column words at k = 64 (an fp64 restatement of the loop on the CPU chose it)"""
    m, n, k = SHAPES[shape]
    rs = np.random.RandomState(m + n)
    dens = 0.2 if k <= 8 else 0.067
    Ub, Vb = rs.rand(m, k) < dens, rs.rand(n, k) < dens
    X = ((Ub.astype(np.float32) @ Vb.astype(np.float32).T) > 0)
    X = (X ^ np.where(X, rs.rand(m, n) < 0.05, rs.rand(m, n) < 0.01)).astype(np.uint8)
    U0 = Ub * (0.05 + 0.5 * rs.rand(m, k)) + 0.15 * rs.rand(m, k) + 1e-6
    V0 = Vb * (0.05 + 0.5 * rs.rand(n, k)) + 0.15 * rs.rand(n, k) + 1e-6
    U1 = Ub * (0.2 + 0.6 * rs.rand(m, k)) + 0.05 * rs.rand(m, k) + 1e-6     # a second start, for the re-base case
    V1 = Vb * (0.2 + 0.6 * rs.rand(n, k)) + 0.05 * rs.rand(n, k) + 1e-6
    X.setflags(write=False)
    return X, U0, V0, U1, V1


REGS = [1.0 * 1.05 ** t for t in range(ITERS + 2)]
PANELS = {"i8x3": dict(panel="i8", terms=3), "f16x2": dict(panel="f16", terms=2)}


def make_engine(L, X, k, panel, delta):
    from pybmf_amd.engine import BitMatrix, MUEngine
    eng = MUEngine(BitMatrix(X, "cuda:0"), k=k, mode=L.MODE_PENALTY, with_mae=False, tol=-1.0, min_diff=-1.0, max_iter=ITERS + 1,
                   cover_delta=delta, **PANELS[panel])
    assert (eng.st.ubits_prev is not None) == delta and (eng.st.vbits_prev is not None) == delta
    return eng


def tp_fp(L, eng):
    log, stop = eng.read_log()
    assert stop == 0
    return log[:, [L.LOG_TP, L.LOG_FP]].astype(np.int64)


def recount(X, eng):
    U, V = eng.factors()
    return cover_numpy(X, U > 0.5, V > 0.5)


@pytest.mark.parametrize("panel", list(PANELS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_loop_totals_equal_full_count(env, shape, panel):
    """40 iterations: every TP / FP of the log equals the full-count engine's, and at iterations 1, 15, 25, 40 a NumPy recount."""
    L, d = env
    X, U0, V0, _, _ = loop_problem(shape)
    k = SHAPES[shape][2]
    a, b = make_engine(L, X, k, panel, True), make_engine(L, X, k, panel, False)
    for e in (a, b):
        e.load_factors(U0, V0)
        e.prepare(REGS[0])
    b.run(REGS[1:ITERS + 1], it0=1)
    assert tuple(tp_fp(L, a)[0]) == recount(X, a)
    dirty_rows, dirty_cols = [], []
    for it in range(1, ITERS + 1):
        ub, vb = a.ubits.clone(), a.vbits.clone()
        a.run([REGS[it]], it0=it)
        dirty_rows.append(int((a.ubits != ub).sum()))
        dirty_cols.append(int((a.vbits != vb).sum()))
        if it in (1, 15, 25, 40):
            assert tuple(tp_fp(L, a)[it]) == recount(X, a), it
    print(shape, panel, "dirty rows per iteration:", dirty_rows, "dirty columns:", dirty_cols)
    ta, tb = tp_fp(L, a), tp_fp(L, b)
    assert ta.shape == tb.shape == (ITERS + 1, 2) and np.array_equal(ta, tb), np.flatnonzero((ta != tb).any(axis=1))
    ua, va = a.factors()
    ub_, vb_ = b.factors()
    assert np.array_equal(ua, ub_) and np.array_equal(va, vb_)
    # the case proves something only if words changed: in some iteration both a row and a column, and not only in the first
    assert any(r > 0 and c > 0 for r, c in zip(dirty_rows, dirty_cols))
    assert sum(r > 0 for r in dirty_rows) >= 2 and sum(c > 0 for c in dirty_cols) >= 2
    assert len(set(map(tuple, ta))) >= 3


@pytest.mark.parametrize("panel", list(PANELS))
def test_loop_prepare_twice_and_rebase(env, panel):
    """prepare() twice counts once; load_factors -> prepare in mid-run re-bases the totals on the new factors."""
    L, d = env
    shape = "two_chunks"
    X, U0, V0, U1, V1 = loop_problem(shape)
    k = SHAPES[shape][2]
    a, b = make_engine(L, X, k, panel, True), make_engine(L, X, k, panel, False)
    for e in (a, b):
        e.load_factors(U0, V0)
        e.prepare(REGS[0])
        e.prepare(REGS[0])
        e.run(REGS[1:9], it0=1)
    assert np.array_equal(tp_fp(L, a), tp_fp(L, b)) and tuple(tp_fp(L, a)[0]) == cover_numpy(X, U0 > 0.5, V0 > 0.5)
    assert tuple(tp_fp(L, a)[8]) == recount(X, a)
    for e in (a, b):
        e.load_factors(U1, V1)
        e.prepare(REGS[0])
        e.run(REGS[1:13], it0=1)
    ta, tb = tp_fp(L, a), tp_fp(L, b)
    assert np.array_equal(ta, tb) and tuple(ta[0]) == cover_numpy(X, U1 > 0.5, V1 > 0.5) and tuple(ta[12]) == recount(X, a)
    assert len(set(map(tuple, ta))) >= 3


@pytest.mark.parametrize("panel", list(PANELS))
def test_loop_stepwise_equals_run(env, panel):
    """bmf_penalty_update_head / _xtu / _finalize, one call each per iteration, against bmf_penalty_run."""
    L, d = env
    shape = "one_chunk"
    X, U0, V0, _, _ = loop_problem(shape)
    k = SHAPES[shape][2]
    a, b = make_engine(L, X, k, panel, True), make_engine(L, X, k, panel, True)
    for e in (a, b):
        e.load_factors(U0, V0)
        e.prepare(REGS[0])
    n_it = 12
    a.run(REGS[1:n_it + 1], it0=1)
    for it in range(1, n_it + 1):
        b.local_update_head(REGS[it])
        b.local_xtu_block(-1)
        b.finalize(it, REGS[it])
    ta, tb = tp_fp(L, a), tp_fp(L, b)
    assert ta.shape == (n_it + 1, 2) and np.array_equal(ta, tb) and tuple(tb[n_it]) == recount(X, b)
    assert len(set(map(tuple, ta))) >= 3
