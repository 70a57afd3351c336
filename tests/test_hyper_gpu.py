"""Hyper on the device: the kernels of csrc/hyper.hip against the NumPy restatement of tests/hyper_ref.py, the device miner against the
stand-in miner, Hyper.fit() against the reference's results (tests/golden/g30_hyper.*) and against the stand-in engine of
tests/test_hyper_cpu.py at the family's boundary shapes, and the bound on host reads.

Everything is integers and bits: every comparison is equality.  Outputs are pre-filled with a marker; rows and slots that a launch
must not write keep it.
"""
import ctypes as C

import numpy as np
import pytest

import hyper_ref as H
from test_hyper_cpu import CASES, NumpyHyperEngine, check_fit, fit_case, load_case, log_rows, numpy_engine

pytestmark = pytest.mark.gpu

MARK = -7
# the shapes of boolean_family.BOUNDARY with a min_support at which the stand-in fit takes a second or less (lower ones make the
# planted blocks' subsets frequent: thousands of itemsets)
BOUNDARY = [(31, 63, 0.5), (32, 64, 0.35), (33, 65, 0.6), (64, 128, 0.6), (65, 129, 0.4), (2049, 20, 0.3), (20, 2049, 0.9)]
ROWS = [31, 32, 33, 2049]
COUNTS = [1, 63, 64, 65]


def planted(m, n, k, density, flips, seed):
    rng = np.random.RandomState(seed)
    U, V = rng.rand(m, k) < density, rng.rand(n, k) < density
    X = (U.astype(int) @ V.astype(int).T) > 0
    if flips:
        X = X ^ (rng.rand(m, n) < flips)
    return X.astype(np.uint8)


def boundary_matrix(i):
    """The family's planted matrix of BOUNDARY[i].  At 2049 columns only every 16th column (2048 among them) keeps its ones: every
    non-empty column becomes a factor of its own there, and a fit costs the host some 20 ms per factor on either engine."""
    m, n, _ = BOUNDARY[i]
    X = planted(m, n, 3, 0.3, 0.03, 2610 + i)
    if n > 1000:
        X[:, np.arange(n) % 16 != 0] = 0
    return X


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def words(a):
    return dev(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def vp(t):
    return C.c_void_p(t.data_ptr())


def marked(shape, dtype=None):
    import torch
    return torch.full(shape, MARK, dtype=dtype or torch.int32, device="cuda:0")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def data():
    """Per row count m: a 12-column matrix (column 10 is empty, column 11 a copy of column 0), its bit rows and a residual in which
    columns 2 and 3 are empty."""
    out = {}
    for m in ROWS:
        X = np.random.RandomState(3200 + m).rand(m, 12) < 0.8
        X[:, 10], X[:, 11] = False, X[:, 0]
        X[m - 1, :10] = True                       # the last row, the last used bit of the last used word, is in every tidset
        R = X & (np.random.RandomState(3300 + m).rand(m, 12) < 0.5)
        R[:, 2:4] = False
        W = H.words_of(m)
        x_t, rs_t = H.pack_rows(X.T, W), H.pack_rows(R.T, W)
        for a in (x_t, rs_t):
            a.setflags(write=False)
        out[m] = (X, x_t, rs_t, W)
    return out


def itemsets_for(count):
    """`count` itemsets over 12 columns, lengths 1, 2 and 7 in turn; with the empty column 10 (an empty tidset) and with columns 2, 3
    only (a residual that is empty on I) among them when there is room."""
    rng = np.random.RandomState(3400 + count)
    sets = [sorted(rng.choice(10, size=(1, 2, 7)[i % 3], replace=False).tolist()) for i in range(count)]
    if count > 2:
        sets[1], sets[2] = [4, 10], [2, 3]
    return sets


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("m", ROWS)
def test_level_kernel(data, m, count):
    from pybmf_amd._lib import check, lib
    X, x_t, _, W = data[m]
    rng = np.random.RandomState(3500 + m + count)
    n_prev = 9
    prev = x_t[rng.randint(0, 12, n_prev)] & x_t[rng.randint(0, 12, n_prev)]
    pairs = np.stack([rng.randint(0, n_prev, count), rng.randint(0, 12, count)], axis=1).astype(np.int32)
    want_tid, want_cnt = H.level_step(prev, x_t, pairs)
    if count > 1:                                  # a pair outside the arrays gives an empty row
        pairs[0] = (n_prev, 3)
        want_tid[0], want_cnt[0] = 0, 0
    out, cnt = marked((count + 2, W)), marked((count + 2,))
    pd, xd, prd = words(prev), words(x_t), dev(pairs)          # (held: a pointer alone does not keep a tensor alive)
    check(lib.bmf_hyper_level(vp(pd), n_prev, vp(xd), 12, W, vp(prd), count, vp(out), vp(cnt), None), "bmf_hyper_level")
    out, cnt = host(out), host(cnt)
    assert (out[count:] == MARK).all() and (cnt[count:] == MARK).all()
    assert np.array_equal(out[:count].view(np.uint32), want_tid) and np.array_equal(cnt[:count], want_cnt)
    assert not H.unpack_rows(out[:count].view(np.uint32), W * 32)[:, m:].any()          # padding bits stay zero


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("m", ROWS)
def test_eval_and_commit_kernels(data, m, count):
    from pybmf_amd._lib import check, lib
    X, x_t, rs_t, W = data[m]
    sets = itemsets_for(count)
    n_cand = count + 3                             # three candidates that no launch names
    sets_all = sets + [[0], [1, 5], [6]]
    padded = H.pad_items(sets_all)
    tid = np.array([np.bitwise_and.reduce(x_t[I], axis=0) for I in sets_all], dtype=np.uint32)
    ids = np.random.RandomState(3600 + m + count).permutation(count).astype(np.int32)
    want_T, want_nT, want_s = H.evaluate(tid, rs_t, padded, ids)
    if count > 2:
        assert not tid[1].any() and tid[2].any() and want_nT[list(ids).index(2)] == 0 and want_nT.any()
    scratch, rec = marked((n_cand, W)), marked((n_cand, 2))
    td, rd, itd, idd = words(tid), words(rs_t), dev(padded), dev(ids)          # (held: a pointer alone does not keep a tensor alive)
    check(lib.bmf_hyper_eval(vp(td), vp(rd), 12, W, vp(itd), padded.shape[1], vp(idd), count, n_cand, vp(scratch), vp(rec), None), "bmf_hyper_eval")
    got_T, got_rec = host(scratch), host(rec)
    assert (got_T[count:] == MARK).all() and (got_rec[count:] == MARK).all()
    assert np.array_equal(got_T[ids].view(np.uint32), want_T)
    assert np.array_equal(got_rec[ids, 0], want_nT) and np.array_equal(got_rec[ids, 1], want_s)
    assert not H.unpack_rows(got_T[:count].view(np.uint32), W * 32)[:, m:].any()
    # the hand count of the definition, on the dense matrices
    R = H.unpack_rows(rs_t[:12], m).T
    for i in ids[:5]:
        rows = X[:, sets[i]].all(axis=1) & R[:, sets[i]].any(axis=1)
        assert got_rec[i, 0] == rows.sum() and got_rec[i, 1] == R[np.ix_(rows, sets[i])].sum()
    # commit: every second listed candidate; the others, and the three unnamed ones, keep the marker
    some = np.sort(ids[::2])
    committed = marked((n_cand, W))
    sd = dev(some)
    check(lib.bmf_hyper_copy(vp(scratch), n_cand, vp(sd), vp(committed), n_cand, vp(sd), W, len(some), None), "bmf_hyper_copy")
    got = host(committed)
    rest = np.setdiff1d(np.arange(n_cand), some)
    assert np.array_equal(got[some], got_T[some]) and (got[rest] == MARK).all()
    assert np.array_equal(host(scratch), got_T)


def test_copy_kernel_compacts_and_skips_bad_ids():
    from pybmf_amd._lib import check, lib
    W = 20
    src = np.random.RandomState(3700).randint(0, 2 ** 31, (7, W)).astype(np.int32)
    dst = marked((5, W))
    a, b = np.array([6, 0, 7, 3, -1], dtype=np.int32), np.array([0, 4, 1, 5, 2], dtype=np.int32)     # pairs 2, 3 and 4 are outside
    sd, ad, bd = dev(src), dev(a), dev(b)
    check(lib.bmf_hyper_copy(vp(sd), 7, vp(ad), vp(dst), 5, vp(bd), W, 5, None), "bmf_hyper_copy")
    got = host(dst)
    assert np.array_equal(got[0], src[6]) and np.array_equal(got[4], src[0]) and (got[1:4] == MARK).all()


# ---- the miner --------------------------------------------------------------------------------------------------------------
def device_engine(X, extra=None):
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.hyper import HyperEngine
    return HyperEngine(BitMatrix(np.ascontiguousarray(X, dtype=np.uint8), "cuda:0"), {k: BitMatrix(v, "cuda:0") for k, v in (extra or {}).items()})


def check_miner(X, min_support):
    eng = device_engine(X)
    sets = eng.mine(min_support)
    want_sets, want_counts = H.mine(X, min_support)
    assert sets == want_sets and eng.support_counts == want_counts
    assert eng.itemsets == [[j] for j in range(X.shape[1])] + want_sets and eng.n_cand == len(eng.itemsets)
    x_t = H.pack_rows((X != 0).T, eng.W)
    want_tid = np.array([np.bitwise_and.reduce(x_t[I], axis=0) for I in eng.itemsets], dtype=np.uint32)
    assert np.array_equal(eng.tidsets(), want_tid)
    return eng


@pytest.mark.parametrize("name", [c for c in CASES if c != "g"])
def test_miner_on_the_fixture_matrices(name):
    case = load_case(name)
    eng = check_miner(case["X"], case["min_support"])
    assert eng.itemsets[eng.n:] == case["itemsets"] and eng.support_counts == case["itemset_counts"]


def test_miner_at_2049_rows_and_on_one_column():
    eng = check_miner(boundary_matrix(5), 0.3)
    assert len(eng.itemsets) > 20 + 50 and max(len(I) for I in eng.itemsets) >= 3
    check_miner(load_case("g")["X"], 0.5)
    check_miner(boundary_matrix(5), 0.9)           # nothing frequent beyond singletons


def test_engine_refuses_what_does_not_fit(monkeypatch):
    import torch
    eng = device_engine(boundary_matrix(5))
    free = torch.cuda.mem_get_info("cuda:0")[0]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, free))
    with pytest.raises(NotImplementedError, match=r"candidates"):
        eng.mine(0.3)


# ---- fits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_device_fit_reproduces_the_reference(name):
    case = load_case(name)
    model, raised = fit_case(case)
    check_fit(model, raised, case)
    eng = model._engine
    if model.T:         # the committed row of the last accepted head is the T it was accepted with
        assert [int(t) for t in np.nonzero(H.unpack_rows(eng._factors[-1][0][None, :], eng.m)[0])[0]] == model.T[-1]


@pytest.mark.parametrize("i", range(len(BOUNDARY)))
def test_device_fit_against_the_stand_in_at_the_boundary_shapes(i):
    m, n, min_support = BOUNDARY[i]
    case = dict(X=boundary_matrix(i), min_support=min_support)
    got, got_raised = fit_case(case)
    want, want_raised = fit_case(case, numpy_engine)
    assert got_raised == want_raised and log_rows(got) == log_rows(want) and len(log_rows(want)) >= 10
    assert got.T == want.T and got.I == want.I and got.k == want.k
    for a, b in ((got.U, want.U), (got.V, want.V), (got.X_pd, want.X_pd)):
        assert a.shape == b.shape and (a != b).nnz == 0
    ge, we = got._engine, want._engine
    assert ge.itemsets == we.itemsets and ge.support_counts == we.support_counts
    assert ge.counts("train") == we.counts("train") and ge.residual_sum() == we.residual_sum()
    for a, b in zip(ge.bit_matrices(), we.bit_matrices()):
        assert np.array_equal(a[:n], b[:n]) and not a[n:].any()
    assert np.array_equal(ge.tidsets(), we.tidsets())
    for cid in (0, n - 1, ge.n_cand - 1):
        assert np.array_equal(ge.committed_T(cid), we.committed_T(cid))
    for a, b in zip(ge.factor_arrays(), we_factor_arrays(we)):
        assert np.array_equal(a, b)


def we_factor_arrays(we):
    fs = we._factors
    U = np.array([H.unpack_rows(u[None, :], we.m)[0] for u, _ in fs], dtype=np.uint8).reshape(len(fs), we.m).T
    V = np.array([H.unpack_rows(v[None, :], we.n)[0] for _, v in fs], dtype=np.uint8).reshape(len(fs), we.n).T
    return U, V


def test_split_fit_reads_once_per_extra_data_set():
    case = load_case("h")
    model, raised = fit_case(case)
    eng, rows = model._engine, len(case["log"]["rows"])
    assert set(eng.truth) == {"train", "val", "test"}
    assert eng.reads <= 4 * rows + 4
    want = NumpyHyperEngine(case["X"], {"val": case["X_val"], "test": case["X_test"]})
    want.pd_t = eng.bit_matrices()[1][: want.n].copy()
    for name in ("train", "val", "test"):
        assert tuple(eng.counts(name)) == tuple(want.counts(name))


def test_host_reads_are_bounded_by_the_log_rows_not_by_iter():
    """Case a: the reference evaluates the head more than 2000 times; the device is read a few times per factor."""
    case = load_case("a")
    model, _ = fit_case(case)
    rows = case["log"]["rows"]
    assert sum(r[1] for r in rows) > 2000
    assert model._engine.reads <= 4 * len(rows) + 4
