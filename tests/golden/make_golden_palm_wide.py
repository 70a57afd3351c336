#!/usr/bin/env python3
"""Golden g34: the proximal models ELBMF and PRIMP of the reference at a rank 64 < k <= 128 (PyBMF/models/ELBMF.py:110-210,
PyBMF/models/PRIMP.py:51-160), made the way g14 / g15 are (make_golden.py): the classes do not run as shipped, so the module-level
functions and the class's own iPALM loop are driven with init_model's working steps done by hand.

    python tests/golden/make_golden_palm_wide.py      ->  g34_palm_wide.npz, g34_palm_wide_steps.npz, g34_palm_wide.json

(two archives to keep each below the size limit of a committed file: the inputs and the loops in the first, the single steps in the
second.)

Matrices: X is 3k x 2k, k disjoint 3 x 2 blocks of ones with 1 % of the cells flipped; the start is 0.7 planted + 0.2 uniform (the
uniform part on a grid of 1/256: the fixture stores the grid indices as bytes, `start_of` rebuilds the start exactly).  k = 65 (one
real column in the second 64-column block), 72, 128.

The prox jumps at 0.5, and a start that puts a cell on the jump amplifies any rounding a thousandfold.  So that no recorded decision
hangs on a rounding, a start is kept only if, in every ELBMF loop case run from it,
  * no entry of U or V is within 1e-3 of 0.5 at any iteration (ten times the gate the device is held to: the Boolean counts can then
    be compared exactly), and
  * three reruns with the start scaled entry-wise by 1 + 1e-6 N(0, 1) give the same counts at every iteration, final factors within
    1e-5 (relative Frobenius) and stop at the same iteration;
otherwise the next seed is tried.  The early-stop case additionally has |gap - gap_last| <= 0.95 min_diff at the stopping iteration
and >= 1.05 min_diff at every iteration before it.  The margins found are recorded in the json.

Recorded factors are stored as fp32 (2^-24 relative, far below the 1e-5 / 1e-4 they are compared at); everything that is an
input is exact.
"""
import importlib
import json
import os

import numpy as np

from make_golden import FIT_KW, HERE, df_rows, load_reference, quiet

MARGIN, JITTER, JITTER_TOL = 1e-3, 1e-6, 1e-5
LOOP = dict(reg_l1=0.01, reg_l2=0.02, reg_growth=1.05)
STEP_PARAMS = ((0.01, 0.02, 0.0), (0.01, 0.5, 0.0), (0.05, 0.02, 0.1), (0.0, 0.0, 0.3))          # g14's
MASKED_STEP_PARAMS = (("W01", 0.01, 0.02, 0.0), ("W01", 0.02, 0.3, 0.2), ("Wr", 0.01, 0.02, 0.0), ("Wr", 0.0, 0.1, 0.15))   # g15's
PRIMP_STEP_PARAMS = ((0.01, 0.0, 1.0, 0.0), (0.05, 0.0, 1.3, 1e-4), (0.02, 0.1, 2.0, 0.2))       # g14's


class Reject(Exception):
    pass


def relf(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def planted(k):
    return np.kron(np.eye(k), np.ones((3, 1))), np.kron(np.eye(k), np.ones((2, 1)))


def matrix(k):
    rs = np.random.RandomState(3400 + k)
    PU, PV = planted(k)
    X = PU @ PV.T
    return np.where(rs.rand(3 * k, 2 * k) < 0.01, 1 - X, X)


def start_of(k, gU, gV):
    """The start from its stored grid indices (uint8): 0.7 planted + 0.2 g / 256."""
    PU, PV = planted(k)
    return 0.7 * PU + 0.2 * gU.astype(np.float64) / 256.0, 0.7 * PV + 0.2 * gV.astype(np.float64) / 256.0


def prev_of(U0, gP):
    """The previous iterate of the single steps from its stored offsets (int16 in -128 .. 128): U0 + 0.05 g / 64."""
    return U0 + 0.05 * gP.astype(np.float64) / 64.0


def start(k, seed):
    rs = np.random.RandomState(seed)
    gU, gV = rs.randint(0, 256, (3 * k, k)).astype(np.uint8), rs.randint(0, 256, (2 * k, k)).astype(np.uint8)
    return start_of(k, gU, gV) + (gU, gV)


def run_loop(E, X_train, U0, V0, W, beta, max_iter, min_diff):
    """The class's own loop (g14 / g15's recipe) with every iterate recorded: (model, min |entry - 0.5| over all iterates)."""
    from PyBMF.models.ContinuousModel import ContinuousModel
    near = [np.inf]
    real_update = E.update_U

    def recording_update(*a, **kw):
        Fn, Fl = real_update(*a, **kw)
        near[0] = min(near[0], float(np.abs(np.asarray(Fn) - 0.5).min()))
        return Fn, Fl
    with quiet():
        mdl = E.ELBMF(k=U0.shape[1], U=U0.copy(), V=V0.copy(), W=W, init_method="custom", beta=beta, max_iter=max_iter, min_diff=min_diff, tol=0.0, **LOOP)
    E.update_U = recording_update
    try:
        with quiet():
            mdl.check_params(**FIT_KW)
            mdl.load_dataset(X_train=X_train.copy(), X_val=None, X_test=None)
            ContinuousModel.init_model(mdl)
            mdl.init_UV()
            mdl._to_dense()
            mdl.U[mdl.U == 0] = np.finfo(float).eps
            mdl.V[mdl.V == 0] = np.finfo(float).eps
            mdl.iPALM()
    finally:
        E.update_U = real_update
    return mdl, near[0]


def loop_case(E, X_train, U0, V0, W, beta, max_iter, min_diff, jitter_seed):
    """One recorded loop with its margins checked; raises Reject when the start does not keep them."""
    mdl, near = run_loop(E, X_train, U0, V0, W, beta, max_iter, min_diff)
    if near < MARGIN:
        raise Reject(f"an entry {near:.2e} from 0.5")
    log = df_rows(mdl.logs["updates"])
    rows = np.array(log["rows"], dtype=np.float64)
    U, V = np.asarray(mdl.U, dtype=np.float64), np.asarray(mdl.V, dtype=np.float64)
    rs = np.random.RandomState(jitter_seed)
    moved = 0.0
    for _ in range(3):
        Uj, Vj = U0 * (1 + JITTER * rs.standard_normal(U0.shape)), V0 * (1 + JITTER * rs.standard_normal(V0.shape))
        mj, _ = run_loop(E, X_train, Uj, Vj, W, beta, max_iter, min_diff)
        rj = np.array(df_rows(mj.logs["updates"])["rows"], dtype=np.float64)
        if rj.shape != rows.shape:
            raise Reject("the jittered run stops at another iteration")
        if not np.array_equal(rj[:, 7:], rows[:, 7:]):
            raise Reject("the jittered run has other counts")
        moved = max(moved, relf(np.asarray(mj.U), U), relf(np.asarray(mj.V), V))
    if moved > JITTER_TOL:
        raise Reject(f"the jittered factors move by {moved:.1e}")
    from scipy.sparse import csr_matrix
    from make_golden import counts_of
    Xc = mdl.X_train if hasattr(mdl.X_train, "tocsr") else csr_matrix(mdl.X_train)
    meta = {"beta": beta, "max_iter": max_iter, "min_diff": min_diff, "n_iter": int(rows.shape[0]), "updates": log,
            "counts": counts_of(None, Xc, mdl.X_pd), "min_dist_to_half": near, "jitter_moved": moved}
    return U, V, meta


def find_start(E, k, cases, first_seed):
    """The first seed whose start keeps the margins in every loop case of `cases` (name -> (X_train, W, beta, max_iter, min_diff))."""
    rejected = []
    for seed in range(first_seed, first_seed + 40):
        U0, V0, gU, gV = start(k, seed)
        try:
            got = {name: loop_case(E, Xt, U0, V0, W, beta, it, md, 7000 + seed) for name, (Xt, W, beta, it, md) in cases.items()}
            return seed, U0, V0, gU, gV, got, rejected
        except Reject as e:
            rejected.append({"seed": seed, "why": str(e)})
    raise RuntimeError(f"k={k}: no seed keeps the margins: {rejected}")


def main():
    import torch
    from scipy.sparse import csr_matrix
    PyBMF = load_reference()   # noqa: F841
    E = importlib.import_module("PyBMF.models.ELBMF")
    P = importlib.import_module("PyBMF.models.PRIMP")
    out, steps, meta = {}, {}, {"margin": MARGIN, "jitter": JITTER, "jitter_tol": JITTER_TOL, "loop": LOOP, "ks": [65, 72, 128]}
    f32 = lambda A: np.asarray(A, dtype=np.float64).astype(np.float32)   # noqa: E731

    for k in (65, 72, 128):
        X = matrix(k)
        m, n = X.shape
        cases = {"palm": (X, "full", 0.0, 12, 1e-8), "ipalm": (X, "full", 0.2, 12, 1e-8)}
        if k == 72:
            rs = np.random.RandomState(3472)
            W01 = (rs.rand(m, n) < 0.6).astype(np.float64)
            W01[7, :] = 0.0        # an unobserved row and column
            W01[:, 11] = 0.0
            Wr = W01 * rs.choice([0.5, 1.0, 2.0], size=(m, n))
            r, c = np.nonzero(W01)
            Xs = csr_matrix((X[r, c], (r, c)), shape=X.shape)   # W='mask': the stored entries, explicit zeros included (g15)
            cases["mpalm"] = (Xs, "mask", 0.0, 12, 1e-8)
            cases["mipalm"] = (Xs, "mask", 0.2, 12, 1e-8)
        seed, U0, V0, gU, gV, got, rejected = find_start(E, k, cases, 100 * k)
        if k == 72:
            # c. a loop that stops early: min_diff from the gap sequence of a run that does not stop, with a 5 % margin on either side
            free, _ = run_loop(E, X, U0, V0, "full", 0.0, 40, 0.0)
            gaps = np.array(df_rows(free.logs["updates"])["rows"], dtype=np.float64)[:, 3]
            d = np.abs(np.diff(np.concatenate([[np.inf], gaps])))
            stop_at = next(t for t in range(4, 36) if d[t] / 0.9 * 1.05 <= d[:t].min())
            md = float(d[stop_at] / 0.9)
            U, V, mc = loop_case(E, X, U0, V0, "full", 0.0, 40, md, 7900)
            assert mc["n_iter"] == stop_at + 1 < 40 and d[stop_at] <= 0.95 * md and d[stop_at - 1] >= 1.05 * md
            mc.update(stop_iter=int(stop_at), diff_at_stop=float(d[stop_at]), diff_before=float(d[stop_at - 1]))
            got["stop"] = (U, V, mc)
        out[f"k{k}_X"], out[f"k{k}_U0_grid"], out[f"k{k}_V0_grid"] = np.packbits(X.astype(np.uint8), axis=1), gU, gV
        meta[f"k{k}"] = {"shape": [m, n, k], "seed": seed, "rejected_seeds": rejected}
        for name, (U, V, mt) in got.items():
            out[f"k{k}_{name}_U"], out[f"k{k}_{name}_V"] = f32(U), f32(V)
            meta[f"k{k}"][name] = mt
        if k != 72:
            continue
        # a. ELBMF single steps (all-ones mask), d. under a 0/1 mask and under real weights
        rs = np.random.RandomState(3473)
        gP = rs.randint(-128, 129, U0.shape).astype(np.int16)
        U_prev = prev_of(U0, gP)
        out["k72_U_prev_grid"], out["k72_W01"], out["k72_Wr_levels"] = gP, np.packbits(W01.astype(np.uint8), axis=1), np.round(Wr * 2).astype(np.uint8)
        ones = np.ones((m, n))
        for i, (l1, l2, beta) in enumerate(STEP_PARAMS):
            Un, Ul = E.update_U(X, U0.copy(), V0.copy(), ones, l1, l2, beta, U_prev.copy())
            assert np.array_equal(Ul, U0)
            Vn, _ = E.update_U(X.T, V0.copy(), Un, ones.T, l1, l2, beta, V0.copy())
            steps[f"k72_step{i}_U"], steps[f"k72_step{i}_V"] = f32(Un), f32(Vn)
        meta["steps"] = [{"reg_l1": a, "reg_l2": b, "beta": c_} for a, b, c_ in STEP_PARAMS]
        for i, (wn, l1, l2, beta) in enumerate(MASKED_STEP_PARAMS):
            Wm = W01 if wn == "W01" else Wr
            Un, _ = E.update_U(X, U0.copy(), V0.copy(), Wm, l1, l2, beta, U_prev.copy())
            Vn, _ = E.update_U(X.T, V0.copy(), U0.copy(), Wm.T, l1, l2, beta, V0.copy())
            steps[f"k72_mstep{i}_U"], steps[f"k72_mstep{i}_V"] = f32(Un), f32(Vn)
        meta["masked_steps"] = [{"W": w, "reg_l1": a, "reg_l2": b, "beta": c_} for w, a, b, c_ in MASKED_STEP_PARAMS]
        # e. PRIMP
        Xt, Ua = torch.from_numpy(X.copy()), torch.from_numpy(U_prev.copy())
        for i, (l1, l2, tau, beta) in enumerate(PRIMP_STEP_PARAMS):
            Un = P.elbmf_step_ipalm(Xt, torch.from_numpy(U0.copy()), torch.from_numpy(V0.T.copy()), Ua.clone(), l1, l2, tau, beta)
            steps[f"k72_pstep{i}_U"] = f32(Un.numpy())
        meta["primp_steps"] = [{"l1reg": a, "l2reg": b, "tau": c_, "beta": d_} for a, b, c_, d_ in PRIMP_STEP_PARAMS]
        for tag, beta in (("primp64", 1e-4), ("primp64_b0", 0.0)):
            with quiet():
                U, Vt = P.elbmf_ipalm(Xt, torch.from_numpy(U0.copy()), torch.from_numpy(V0.T.copy()), 0.01, 0, lambda t: 1.02 ** t, 25, 1e-8, beta, None)
            out[f"k72_{tag}_U"], out[f"k72_{tag}_Vt"] = f32(U.numpy()), f32(Vt.numpy())
            Ur, Vr = P.proxelbmfnn(U, 0.5, 0 * 1e12).round(), P.proxelbmfnn(Vt, 0.5, 0 * 1e12).round()
            out[f"k72_{tag}_Ur"], out[f"k72_{tag}_Vtr"] = np.packbits(Ur.numpy().astype(np.uint8), axis=1), np.packbits(Vr.numpy().astype(np.uint8), axis=1)
            meta[tag] = {"beta": beta, "maxiter": 25, "fn_final": float((Xt - U @ Vt).norm() ** 2)}
        with quiet():
            Ur, Vr = P.primp(Xt.float(), k, l1reg=0.01, maxiter=25, beta=1e-4, seed=3)
        torch.manual_seed(3)
        out["k72_primp_seed3_U0"], out["k72_primp_seed3_Vt0"] = torch.rand(m, k).numpy(), torch.rand(k, n).numpy()
        out["k72_primp_seed3_Ur"], out["k72_primp_seed3_Vtr"] = (np.packbits(Ur.numpy().astype(np.uint8), axis=1),
                                                                   np.packbits(Vr.numpy().astype(np.uint8), axis=1))
        meta["torch_version"] = torch.__version__

    np.savez_compressed(os.path.join(HERE, "g34_palm_wide.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "g34_palm_wide_steps.npz"), **steps)
    with open(os.path.join(HERE, "g34_palm_wide.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("g34:", os.path.getsize(os.path.join(HERE, "g34_palm_wide.npz")), "+", os.path.getsize(os.path.join(HERE, "g34_palm_wide_steps.npz")), "bytes;", {k: meta[f"k{k}"]["seed"] for k in (65, 72, 128)})


if __name__ == "__main__":
    main()
