#!/usr/bin/env python3
"""Golden g35: the link models of the reference -- PNLPF (PyBMF/models/PNLPF.py:61-91) and WNMF with the Kullback-Leibler loss
(PyBMF/models/WNMF.py:111-129, error :143-145) -- at a rank 64 < k <= 128, through the loader of make_golden.py.

    python tests/golden/make_golden_link_wide.py      ->  g35_link_wide.npz, g35_link_wide.json

Cases (small planted Boolean matrices, 90 x 70; masks, weights and the train / val / test split by the recipes of g10 / g13 / g16 /
g18 / g20):
    a  PNLPF    k = 65   W='full'
    b  PNLPF    k = 72   W='mask', task='prediction', with X_val / X_test
    c  PNLPF    k = 128  W='full'
    d  PNLPF    k = 72   W='mask' on a csr with explicit zeros (an unobserved row and column), plus single update_V / update_U steps
                         under a real weight matrix (from d's start)
    e  WNMF-KL  k = 72   W='full'                                   (the whole matrix and the start of b)
    f  WNMF-KL  k = 128  the default W='mask' on a dense Boolean matrix     (the matrix and the start of c)
    g  WNMF-KL  k = 72   a real weight matrix                        (the matrix and the start of e)
The Kullback-Leibler cases take the starts of b and c so that the archive stays below the size limit of a committed file.

PNLPF: 5 iterations, reg = 1, reg_growth = 1.2, link_lamda = 10, the start is the reference's 'normal' + 'balance' init of a seed.
PNLPF logs Boolean counts every iteration and they are compared exactly, so no recorded count may hang on a rounding.  Seeds are
screened here, on the CPU, from the reference alone; a case is written only if
  * no entry of U or V lies within 3e-4 of 0.5 at any iterate (three times the 1e-4 gate the device is held to).  The iterates come
    from replaying the loop with the reference's module-level update_V / update_U; the replay is asserted to land on the class's factors;
  * three jittered replays -- every update's numerators and denominators scaled entry-wise by 1 + 1e-6 N(0, 1), i.e. the updated factor
    by their ratio -- threshold to the same bits (so the same counts) at every iteration and move the final factors by less than a third
    of the gate (relative Frobenius).
The margins found are recorded in the json.  Starts are stored as fp64 (exact inputs), final factors as fp32.
"""
import json
import os
import sys

import numpy as np

from make_golden import FIT_KW, HERE, df_rows, load_reference, quiet

MARGIN, GATE, JITTER, MAX_SEEDS = 3e-4, 1e-4, 1e-6, 4000
M, N = 90, 70
PNLPF_KW = dict(reg=1.0, reg_growth=1.2, link_lamda=10, max_iter=4)      # n_iter > max_iter ends the loop: 5 iterations
KL_ITERS = 5
STEP_PARAMS = ((1.5, 10.0), (0.7, 4.0))


class Reject(Exception):
    pass


def relf(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def planted(seed, kt=8, density=0.22, flip=0.03):
    rs = np.random.RandomState(seed)
    A = (rs.rand(M, kt) < density).astype(int)
    B = (rs.rand(N, kt) < density).astype(int)
    X = np.minimum(A @ B.T, 1).astype(np.float64)
    f = rs.rand(M, N) < flip
    X[f] = 1 - X[f]
    for i in np.flatnonzero(X.sum(1) == 0):      # (g13: the reference divides 0 / 0 on an all-zero row or column under W='mask')
        X[i, i % N] = 1.0
    for j in np.flatnonzero(X.sum(0) == 0):
        X[j % M, j] = 1.0
    return X


def stage(model, task, X_train, X_val=None, X_test=None):
    kw = dict(FIT_KW)
    kw["task"] = task
    model.check_params(**kw)
    model.load_dataset(X_train=X_train.copy(), X_val=None if X_val is None else X_val.copy(), X_test=None if X_test is None else X_test.copy())
    model.init_model()
    return np.array(model.U, dtype=np.float64), np.array(model.V, dtype=np.float64)


def replay(mod, X, W, U, V, jitter_rs=None):
    """The loop of the class with the reference's module-level updates; every iterate, the start included."""
    reg, its = np.float64(PNLPF_KW["reg"]), [(U, V)]
    for _ in range(PNLPF_KW["max_iter"] + 1):
        V = mod.update_V(X=X, W=W, U=U, V=V, reg=reg, link_lamda=PNLPF_KW["link_lamda"])
        if jitter_rs is not None:
            V = V * (1 + JITTER * jitter_rs.standard_normal(V.shape)) / (1 + JITTER * jitter_rs.standard_normal(V.shape))
        U = mod.update_U(X=X, W=W, U=U, V=V, reg=reg, link_lamda=PNLPF_KW["link_lamda"])
        if jitter_rs is not None:
            U = U * (1 + JITTER * jitter_rs.standard_normal(U.shape)) / (1 + JITTER * jitter_rs.standard_normal(U.shape))
        its.append((np.asarray(U), np.asarray(V)))
        reg = min(reg * np.float64(PNLPF_KW["reg_growth"]), np.float64(1e10))
    return its


def pnlpf_case(PNLPF, mod, k, W, task, sets, first_seed):
    """The first seed from `first_seed` whose run keeps the margins: (U0, V0, model, margins)."""
    tried = 0
    for seed in range(first_seed, first_seed + MAX_SEEDS):
        tried += 1
        try:
            with quiet():
                mdl = PNLPF(k=k, W=W, init_method="normal", normalize_method="balance", seed=seed, **PNLPF_KW)
                U0, V0 = stage(mdl, task, *sets)
                its = replay(mod, mdl.X_train, mdl.W, U0, V0)
            near = min(min(float(np.abs(U - 0.5).min()), float(np.abs(V - 0.5).min())) for U, V in its)
            if not near >= MARGIN:
                raise Reject(f"an entry {near:.2e} from 0.5")
            moved = 0.0
            rs = np.random.RandomState(9000 + seed)
            for _ in range(3):
                with quiet():
                    jit = replay(mod, mdl.X_train, mdl.W, U0, V0, rs)
                for (U, V), (Uj, Vj) in zip(its, jit):
                    if not (np.array_equal(U > 0.5, Uj > 0.5) and np.array_equal(V > 0.5, Vj > 0.5)):
                        raise Reject("a jittered replay thresholds to other bits")
                moved = max(moved, relf(jit[-1][0], its[-1][0]), relf(jit[-1][1], its[-1][1]))
            if not moved < GATE / 3:
                raise Reject(f"the jittered factors move by {moved:.1e}")
            with quiet():
                mdl._fit()
            rows = df_rows(mdl.logs["updates"])["rows"]
            if len(rows) != len(its):
                raise Reject("the class stops at another iteration than the replay")
            assert relf(mdl.U, its[-1][0]) < 1e-12 and relf(mdl.V, its[-1][1]) < 1e-12, "the replay does not land on the class's factors"
            return U0, V0, mdl, {"seed": seed, "seeds_tried": tried, "min_dist_to_half": near, "jitter_moved": moved}
        except Reject:
            continue
    raise RuntimeError(f"k={k} W={W} {task}: no seed among {MAX_SEEDS} keeps the margins; shrink the matrix, do not lower the margin")


def main():
    from scipy.sparse import csr_matrix
    load_reference()
    from PyBMF.models import PNLPF, WNMF
    mod = sys.modules["PyBMF.models.PNLPF"]
    f32 = lambda A: np.asarray(A, dtype=np.float64).astype(np.float32)   # noqa: E731
    out = {"shape": np.array([M, N])}
    meta = {"margin": MARGIN, "gate": GATE, "jitter": JITTER, "pnlpf": dict(PNLPF_KW), "kl_max_iter": KL_ITERS - 1, "cases": {}}

    def record_pnlpf(name, k, W, task, U0, V0, mdl, margins):
        out.update({f"{name}_U0": U0, f"{name}_V0": V0, f"{name}_U": f32(mdl.U), f"{name}_V": f32(mdl.V)})
        meta["cases"][name] = {"model": "PNLPF", "k": k, "W": W, "task": task, "updates": df_rows(mdl.logs["updates"]),
                               "boolean": df_rows(mdl.logs["boolean"]), "final_reg": float(mdl.reg), **margins}

    # a, c: W='full' on a dense matrix
    for name, k, xseed in (("a", 65, 3501), ("c", 128, 3503)):
        X = planted(xseed)
        out[f"{name}_X"] = np.packbits(X.astype(np.uint8), axis=1)
        U0, V0, mdl, mg = pnlpf_case(PNLPF, mod, k, "full", "reconstruction", (X,), 100 * k)
        record_pnlpf(name, k, "full", "reconstruction", U0, V0, mdl, mg)

    # b: W='mask', task='prediction', X_val / X_test (g20's split by cell: the stored entries are ones AND explicit zeros)
    Xb = planted(3502)
    rs = np.random.RandomState(3512)
    part = rs.rand(M, N)
    sets = {}
    for nm, lo, hi in (("train", 0.0, 0.35), ("val", 0.35, 0.43), ("test", 0.43, 0.52)):
        r, c = np.nonzero((part >= lo) & (part < hi))
        sets[nm] = csr_matrix((Xb[r, c], (r, c)), shape=(M, N))
        assert sets[nm].nnz == r.size
        out.update({f"b_{nm}_rows": r.astype(np.int32), f"b_{nm}_cols": c.astype(np.int32), f"b_{nm}_vals": Xb[r, c].astype(np.uint8)})
    out["b_X"] = np.packbits(Xb.astype(np.uint8), axis=1)
    U0, V0, mdl, mg = pnlpf_case(PNLPF, mod, 72, "mask", "prediction", (sets["train"], sets["val"], sets["test"]), 7200)
    record_pnlpf("b", 72, "mask", "prediction", U0, V0, mdl, mg)
    Ub0, Vb0 = U0, V0

    # d: W='mask' on a csr with explicit zeros, an unobserved row and column (g16), and single steps under a real weight matrix
    Xd = planted(3504)
    rs = np.random.RandomState(3514)
    obs = rs.rand(M, N) < 0.35
    obs[3, :] = False
    obs[:, 8] = False
    r, c = np.nonzero(obs)
    Xs = csr_matrix((Xd[r, c], (r, c)), shape=(M, N))
    assert Xs.nnz == r.size
    out.update(d_rows=r.astype(np.int32), d_cols=c.astype(np.int32), d_vals=Xd[r, c].astype(np.uint8), d_X=np.packbits(Xd.astype(np.uint8), axis=1))
    U0, V0, mdl, mg = pnlpf_case(PNLPF, mod, 72, "mask", "reconstruction", (Xs,), 7300)
    record_pnlpf("d", 72, "mask", "reconstruction", U0, V0, mdl, mg)
    Wr = obs * rs.choice([0.5, 1.0, 2.0], size=(M, N))
    out["d_Wr_levels"] = np.round(Wr * 2).astype(np.uint8)        # Wr = levels / 2
    for i, (reg, lam) in enumerate(STEP_PARAMS):
        with quiet():
            Vn = mod.update_V(X=Xd, W=Wr, U=U0, V=V0, reg=np.float64(reg), link_lamda=lam)
            Un = mod.update_U(X=Xd, W=Wr, U=U0, V=Vn, reg=np.float64(reg), link_lamda=lam)
        out[f"d_step{i}_V"], out[f"d_step{i}_U"] = f32(Vn), f32(Un)
    meta["cases"]["d"]["steps"] = [{"reg": a, "link_lamda": b} for a, b in STEP_PARAMS]

    # e, f, g: WNMF with the Kullback-Leibler loss from the starts of b and c (no Boolean counts in its log: nothing to screen)
    Xc = np.unpackbits(out["c_X"], axis=1)[:, :N].astype(np.float64)
    rs = np.random.RandomState(3518)
    ob = rs.rand(M, N) < 0.7
    ob |= Xb != 0
    Wg = ob * rs.choice([0.5, 1.0, 2.0], size=(M, N))
    out["g_Wr_levels"] = np.round(Wg * 2).astype(np.uint8)
    for name, k, X, U0, V0, W in (("e", 72, Xb, Ub0, Vb0, "full"), ("f", 128, Xc, out["c_U0"], out["c_V0"], "mask"), ("g", 72, Xb, Ub0, Vb0, "weights")):
        with quiet():
            w = WNMF(k=k, U=U0.copy(), V=V0.copy(), W="full" if W == "weights" else W, beta_loss="kullback-leibler", init_method="custom",
                     max_iter=KL_ITERS - 1)
            stage(w, "reconstruction", X)
            if W == "weights":      # (g18: the reference's init_W cannot take a matrix; W is replaced before the loop runs)
                w.W = Wg.copy()
            w._fit()
        out[f"{name}_U"], out[f"{name}_V"] = f32(w.U), f32(w.V)
        meta["cases"][name] = {"model": "WNMF-KL", "k": k, "W": W, "task": "reconstruction", "start": "b" if k == 72 else "c",
                               "updates": df_rows(w.logs["updates"])}

    np.savez_compressed(os.path.join(HERE, "g35_link_wide.npz"), **out)
    with open(os.path.join(HERE, "g35_link_wide.json"), "w") as f:
        json.dump(meta, f, indent=1)
    size = os.path.getsize(os.path.join(HERE, "g35_link_wide.npz"))
    assert size < (1 << 20), size
    print("g35:", size, "bytes;", {n: (c.get("seed"), c.get("seeds_tried"), c.get("min_dist_to_half")) for n, c in meta["cases"].items()})


if __name__ == "__main__":
    main()
