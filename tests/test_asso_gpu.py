"""Asso on the device: the kernels of csrc/asso.hip against the NumPy stand-in of tests/test_asso_cpu.py on the recorded sweeps and on
ragged shapes, Asso.fit() against the reference's results (tests/golden/g24_asso.*), and one run at the MovieLens-1M shape that no
reference stands behind, held to the invariants of any correct Asso.

Counts are integers and the scores are one fp64 expression on them: every comparison of device against stand-in is equality.
"""
import contextlib
import io
import time

import numpy as np
import pytest

from test_asso_cpu import (CASES, DYADIC, NumpyAssoEngine, check_fit, engine_at_point, expected_sweep, fit_case, load_case, log_rows,
                           score_block, unpack)

pytestmark = pytest.mark.gpu


def device_engine(X):
    from pybmf_amd.asso import AssoEngine
    from pybmf_amd.engine import BitMatrix
    return AssoEngine(BitMatrix(np.ascontiguousarray(X, dtype=np.uint8), "cuda:0"))


class DeviceAt:
    """engine_at_point's engine class for the device: AssoEngine from a dense matrix."""
    def __new__(cls, X):
        return device_engine(X)


def ragged(m, n, density, seed, empty_cols=()):
    rng = np.random.RandomState(seed)
    U, V = rng.rand(m, 5) < 0.3, rng.rand(n, 5) < 0.3
    X = ((U.astype(int) @ V.astype(int).T) > 0) ^ (rng.rand(m, n) < density)
    X[:, list(empty_cols)] = False
    return X.astype(np.uint8)


def sweep_both(eng, ref, cands, best_score, w_fp, w_fn):
    """One launch over `cands` on the device and the stand-in's answer; asserts they agree to the bit; returns the device's output."""
    tp_d, fp_d = eng.row_counts()
    tp_r, fp_r = ref.row_counts()
    assert tp_d.tolist() == tp_r.tolist() and fp_d.tolist() == fp_r.tolist()
    eng.set_list(cands)
    ref.set_list(cands)
    import torch
    with torch.cuda.device(eng.device):
        eng._cand[: len(cands)].copy_(torch.from_numpy(np.ascontiguousarray(cands, dtype=np.int32)))
    eng.launch_score(0, len(cands), float(best_score), float(w_fp), float(w_fn))
    T, F, score, rec = eng.launch_results(len(cands))
    T0, F0, score0, vectors0, first0 = score_block(ref.X, ref.pd, ref.basis, ref.m, cands, tp_r, fp_r, float(w_fp), float(w_fn), best_score)
    assert T.tolist() == T0.tolist() and F.tolist() == F0.tolist()
    assert score.tobytes() == score0.tobytes()
    assert rec[0] == first0
    if first0 >= 0:
        assert rec[1] == cands[first0] and rec[2:3].view(np.float64)[0] == score0[first0] and [rec[3], rec[4]] == [T0[first0], F0[first0]]
    else:
        assert rec[1] == -1 and rec[2:3].view(np.float64)[0] == float(best_score) and [rec[3], rec[4]] == [0, 0]
    return T, F, score, rec, vectors0


@pytest.mark.parametrize("name", CASES)
def test_basis_against_the_recorded_candidates(name):
    case = load_case(name)
    eng = device_engine(case["X"])
    assert eng.build_basis(case["tau"]) == len(case["kept"])
    assert eng.list.tolist() == case["kept"].tolist()
    assert eng.basis_rows().tolist() == case["basis"].tolist()
    assert int(np.unpackbits(eng.basis.cpu().numpy().view(np.uint8)).sum()) == int(case["basis"].sum())      # padding bits stay zero


@pytest.mark.parametrize("m,n,empty", [(70, 45, (3,)), (300, 100, ()), (1000, 130, (0, 129)), (33, 64, (63,)), (513, 515, (514,))])
def test_basis_at_ragged_shapes(m, n, empty):
    X = ragged(m, n, 0.05, 40 + n, empty)
    Xi = X.astype(np.int64)
    Cm = Xi.T @ Xi
    s = np.diag(Cm).astype(np.float64)
    eng = device_engine(X)
    for tau in (0.0, 0.3, 0.5, 1.0 - 2.0 ** -40, 1.0):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = (Cm.astype(np.float64) / s[:, None] > tau) & (s[:, None] > 0)
        count = eng.build_basis(tau)
        assert eng.basis_rows().tolist() == want.astype(np.uint8).tolist(), tau
        assert count == int(want.any(axis=1).sum()) and eng.list.tolist() == np.nonzero(want.any(axis=1))[0].tolist()
        for c in empty:
            assert c not in eng.list
    assert eng.build_basis(1.0) == 0          # nothing is above 1
    assert eng.build_basis(1.0 - 2.0 ** -40) == int((X.sum(axis=0) > 0).sum())      # just below 1: every column that is not empty keeps its diagonal


@pytest.mark.parametrize("name", ["a", "b"])
def test_score_pick_column_at_the_recorded_sweeps(name):
    case = load_case(name)
    w_fp, w_fn = case["weights"]
    for p in case["points"]:
        eng, ref = engine_at_point(DeviceAt, case, p), engine_at_point(NumpyAssoEngine, case, p)
        T, F, score, rec, vectors = sweep_both(eng, ref, p["list"], p["best_score"], w_fp, w_fn)
        want_T, want_F = expected_sweep(case, p)
        assert T.tolist() == want_T.tolist() and F.tolist() == want_F.tolist()
        assert score.tolist() == p["scores"].tolist() and rec[0] == p["winner"]
        for block in (None, 1, 7):
            assert eng.best(p["best_score"], w_fp, w_fn, block=block) == ref.best(p["best_score"], w_fp, w_fn, block=block)
        for i in (0, p["winner"], len(p["list"]) - 1):
            u, v = eng.column(int(p["list"][i]), w_fp, w_fn)
            assert unpack(u, eng.m).tolist() == (p["vectors"][i] != 0).tolist() and not unpack(u, eng.W * 32)[eng.m:].any()
            assert unpack(v, eng.n).tolist() == (case["basis"][p["list"][i]] != 0).tolist()


@pytest.mark.parametrize("m,n,w_fp,w_fn", [(70, 45, 0.5, 0.5), (300, 100, 0.3, 0.7), (1000, 130, 1.0, 1.0), (65, 515, 0.45, 0.8),
                                           (129, 1030, 0.5, 0.5)])
def test_score_on_random_predictions_at_ragged_shapes(m, n, w_fp, w_fn):
    X = ragged(m, n, 0.05, 70 + n, (1,))
    rng = np.random.RandomState(m)
    eng, ref = device_engine(X), NumpyAssoEngine(X)
    assert eng.build_basis(0.35) == ref.build_basis(0.35) and eng.basis.cpu().numpy().view(np.uint32).tobytes() == ref.basis.tobytes()
    full = ref.list.copy()
    for density in (0.0, 0.1, 0.6):
        pd = (rng.rand(m, n) < density).astype(np.uint8)
        eng.load_prediction(pd)
        ref.load_prediction(pd)
        for cands, best in ((full, 0.0), (full[::3][::-1].copy(), 50.0), (full[:1], 1e9), (np.arange(n, dtype=np.int32), -1e9)):
            T, F, score, rec, vectors = sweep_both(eng, ref, cands, best, w_fp, w_fn)
            j = int(cands[len(cands) // 2])
            u, v = eng.column(j, w_fp, w_fn)
            assert unpack(u, m).tolist() == vectors[len(cands) // 2].tolist() and v.tobytes() == ref.basis[j].tobytes()
        for block in (None, 5, 64, 100):
            eng.set_list(full)
            ref.set_list(full)
            assert eng.best(0.0, w_fp, w_fn, block=block) == ref.best(0.0, w_fp, w_fn, block=block)
    # a factor joins the prediction: bits, counts and the truncation back
    for e in (eng, ref):
        e.truncate(0)
    hit = eng.best(0.0, w_fp, w_fn)
    assert hit is not None and hit == ref.best(0.0, w_fp, w_fn)
    u, v = eng.column(hit[1])
    for e in (eng, ref):
        e.apply(u, v)
    assert eng.pd.cpu().numpy().view(np.uint32).tobytes() == ref.pd.tobytes() and eng.counts("train") == ref.counts("train")
    eng.truncate(0)
    assert eng.counts("train")[:2] == (0, 0) and eng.n_factors == 0


def test_two_identical_launches_give_identical_bytes():
    X = ragged(700, 300, 0.05, 91)
    eng = device_engine(X)
    eng.build_basis(0.3)
    eng.load_prediction((np.random.RandomState(3).rand(700, 300) < 0.2).astype(np.uint8))
    import torch
    cands = eng.list.copy()
    eng.row_counts()
    eng._cand[: len(cands)].copy_(torch.from_numpy(cands))
    out = []
    for _ in range(2):
        eng._work.zero_()
        eng.launch_score(0, len(cands), 10.0, 0.3, 0.7)
        torch.cuda.synchronize()
        used = (-(-700 // 64)) * len(cands) * 2
        out.append([eng._work[:used].cpu().numpy().tobytes()] + [a.tobytes() for a in eng.launch_results(len(cands))])
        out[-1].append(eng.basis.cpu().numpy().tobytes())
        eng.build_basis(0.3)
    assert out[0] == out[1]


@pytest.mark.parametrize("name", CASES)
def test_fit_reproduces_the_reference(name):
    case = load_case(name)
    t0 = time.time()
    model = fit_case(case)
    wall = time.time() - t0
    print(f"asso fit {name}: {len(log_rows(model))} rows, {model.U.shape[1]} factors kept, {wall:.2f} s")
    from pybmf_amd.asso import AssoEngine
    assert isinstance(model._engine, AssoEngine)
    check_fit(model, case, exact_score=name in DYADIC)


@pytest.mark.parametrize("block", [1, 7, 40])
def test_block_size_on_the_device(block):
    for name in ("a", "c"):
        case = load_case(name)
        check_fit(fit_case(case, block=block), case)


def recount_with_cover_kernel(bits, U, V):
    """(TP, FP) of U o V^T against the bits of X by bmf_cover_count: independent of the Asso kernels and of the prediction bits."""
    import torch
    from pybmf_amd import _lib as L
    k = U.shape[1]
    kp = 32
    rowbits = np.zeros(bits.m_pad, np.uint64)
    rowbits[: bits.m] = (U.astype(np.uint64) * (1 << np.arange(k, dtype=np.uint64))).sum(axis=1)
    vcol = np.zeros((kp, bits.n_pad), np.uint8)
    vcol[:k, : bits.n] = V.T
    colbits = np.packbits(vcol, axis=1, bitorder="little").view(np.int32)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    ud, vd = torch.from_numpy(rowbits.view(np.int64)).to("cuda:0"), torch.from_numpy(colbits).to("cuda:0")
    L.check(L.lib.bmf_cover_count(L.ptr(bits.bits), bits.m_pad, bits.ldx, bits.n_pad // 32, L.ptr(ud), L.ptr(vd), bits.n_pad // 32, kp,
                                  L.ptr(counts), None, None), "bmf_cover_count")
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    return int(got[0]), int(got[1])


def test_ml1m_shape_invariants():
    from pybmf_amd.generators import PlantedBooleanOnDevice
    from pybmf_amd.models import Asso
    m, n, k = 6040, 3706, 8
    X = PlantedBooleanOnDevice(m, n, 10, density=(0.15, 0.15), seed=2410, noise=(0.05, 0.005), noise_seed=2411)
    w_fp, w_fn = 0.5, 0.5
    models = []
    for block in (None, 1000):
        with contextlib.redirect_stdout(io.StringIO()):
            model = Asso(tau=0.5, k=k, w_fp=w_fp)
            t0 = time.time()
            model.fit(X, task="reconstruction", show_logs=False, show_result=False, save_model=False, block=block)
            wall = time.time() - t0
        print(f"asso ml1m: k = {k}, block {block}: fit {wall:.2f} s, {model._engine.list.size} candidates left")
        models.append(model)
    model = models[0]
    rows = log_rows(model)
    assert len(rows) == k and log_rows(models[1]) == rows
    assert (models[0].U != models[1].U).nnz == 0 and (models[0].V != models[1].V).nnz == 0
    U, V = np.asarray(model.U.todense()) != 0, np.asarray(model.V.todense()) != 0
    assert U.shape == (m, k) and V.shape == (n, k)
    scores = [r[1] for r in rows]
    assert scores[0] > 0 and all(b > a for a, b in zip(scores, scores[1:]))           # best_score strictly increasing
    bits = model._engine.bits
    for f, r in enumerate(rows):
        tp, fp = recount_with_cover_kernel(bits, U[:, : f + 1], V[:, : f + 1])
        assert [int(r[6]), int(r[8])] == [tp, fp]                                         # the log's TP / FP
        assert r[1] == w_fn * tp - w_fp * fp == r[2]                                     # score = coverage of the whole prediction
        assert [r[4], r[5]] == [int(U[:, f].sum()), int(V[:, f].sum())] and r[4] > 0 and r[5] > 0
        assert r[3] == U[:, : f + 1].sum() + V[:, : f + 1].sum() + fp + int(r[10])        # description length
    tp, fp, fn, tn = model._engine.counts("train")
    assert (tp, fp) == recount_with_cover_kernel(bits, U, V) and tp + fn == int(bits.sum_local) and tp + fp + fn + tn == m * n
    assert scores[-1] == w_fn * tp - w_fp * fp
