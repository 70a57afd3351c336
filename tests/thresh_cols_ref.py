"""The NumPy statement of BinaryMFThresholdExColumnwise: the dense product Us Vs^T, F, dF, bounds, counts, metrics and a fit that runs
this package's ``solvers.line_search`` / ``limit_step_size`` on them and keeps the margin of every Armijo and curvature comparison.
Plain helpers, no tests; tests/test_thresh_cols_cpu.py, test_thresh_cols_kernels_gpu.py and test_thresh_cols_gpu.py hold the kernels and
the model to it.

Definitions (those of DESIGN 9.3; the reference's module is absent, the scalar model and the notebook's record define it):
  Us[i][c]  = sigmoid(lamda (U[i][c] - us[c])), dUs = lamda Us (1 - Us); likewise Vs, dVs with vs
  F(x)      = 1/2 || X - Us Vs^T ||^2, x = [us, vs]
  dF[c]     = sum_i ((R Vs) * dUs)[i][c], dF[k + c] = sum_j ((R^T Us) * dVs)[j][c], R = X - Us Vs^T   (the scalar model's sign)
  bounds    per column [min + 1e-6, max - 1e-6]
  search    line_search(maxiter=50), limit_step_size, stop when n_iter > max_iter or |new F - old F| < min_diff
  scores    Recall, Precision, Accuracy, F1 from the integer counts of ((U > us) @ (V > vs).T > 0) against X
"""
import numpy as np

from pybmf_amd.solvers import line_search, limit_step_size

METRICS = ["Recall", "Precision", "Accuracy", "F1"]
C1, C2 = 0.1, 0.4   # line_search's defaults


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def transform(F, thr, lam):
    S = sigmoid(lam * (np.asarray(F, dtype=np.float64) - np.asarray(thr, dtype=np.float64)[None, :]))
    return S, lam * S * (1.0 - S)


def F(X, U, V, x, lam):
    k = U.shape[1]
    Us, _ = transform(U, x[:k], lam)
    Vs, _ = transform(V, x[k:], lam)
    R = X - Us @ Vs.T
    return 0.5 * float((R * R).sum())


def dF(X, U, V, x, lam):
    k = U.shape[1]
    Us, dUs = transform(U, x[:k], lam)
    Vs, dVs = transform(V, x[k:], lam)
    R = X - Us @ Vs.T
    return np.concatenate([((R @ Vs) * dUs).sum(axis=0), ((R.T @ Us) * dVs).sum(axis=0)])


def bounds(U, V):
    eps = 1e-6
    return (np.concatenate([U.min(axis=0) + eps, V.min(axis=0) + eps]), np.concatenate([U.max(axis=0) - eps, V.max(axis=0) - eps]))


def product(U, V, us, vs):
    """Boolean product of the thresholded factors (fp32 sums of 0 / 1 products are exact integers below 2^24 terms)."""
    return ((U > np.asarray(us)[None, :]).astype(np.float32) @ (V > np.asarray(vs)[None, :]).astype(np.float32).T) > 0


def counts(X, P):
    Xb = np.asarray(X) != 0
    tp, fp, fn = int((P & Xb).sum()), int((P & ~Xb).sum()), int((~P & Xb).sum())
    return tp, fp, fn, Xb.size - tp - fp - fn


def scores(tp, fp, fn, tn):
    n_gt, n_pd = tp + fn, tp + fp
    recall = np.float64(tp) / n_gt if n_gt > 0 else 0
    precision = np.float64(tp) / n_pd if n_pd > 0 else 0
    accuracy = np.float64(tp + tn) / (tp + fp + fn + tn)
    s = precision + recall
    return [recall, precision, accuracy, 2 * precision * recall / s if s > 0 else 0]


def fit(X, U, V, us, vs, lam, min_diff=1e-3, max_iter=100, extra=None):
    """The search of the scalar model on the columnwise objective.  Returns the rows of the log (x, F, counts and scores per data set),
    n_iter, the evaluation counts line_search reports per iteration, how many steps limit_step_size shortened, and the smallest margins:
    `armijo` / `curvature` = min over every comparison of |lhs - rhs| / max(|fk|, 1), `entry` = min distance of a factor entry to a
    logged threshold of its column."""
    X = np.asarray(X, dtype=np.float64)
    k = U.shape[1]
    sets = {"train": X}
    sets.update({name: np.asarray(Y, dtype=np.float64) for name, Y in (extra or {}).items()})
    out = {"x": [], "F": [], "counts": {s: [] for s in sets}, "scores": {s: [] for s in sets}, "evals": [], "clamped": 0,
           "armijo": np.inf, "curvature": np.inf, "entry": np.inf}

    def log(x, fval):
        out["x"].append(x.copy())
        out["F"].append(fval)
        P = product(U, V, x[:k], x[k:])
        for s, Y in sets.items():
            c = counts(Y, P)
            out["counts"][s].append(c)
            out["scores"][s].append(scores(*c))
        out["entry"] = min(out["entry"], float(np.abs(U - x[:k][None, :]).min()), float(np.abs(V - x[k:][None, :]).min()))

    f = lambda x: F(X, U, V, x, lam)        # noqa: E731
    g = lambda x: dF(X, U, V, x, lam)       # noqa: E731
    n_iter = 0
    x_last = np.concatenate([np.asarray(us, dtype=np.float64), np.asarray(vs, dtype=np.float64)])
    p_last = -g(x_last)
    log(x_last, f(x_last))
    x_min, x_max = bounds(U, V)
    improving = True
    while improving:
        n_iter += 1
        xk, pk = x_last, p_last
        fk, slope0 = f(xk), float(np.dot(g(xk), pk))
        scale = max(abs(fk), 1.0)
        lead = int(np.argmax(np.abs(pk)))

        def f_seen(x):   # line_search's Armijo test on this value: f(x) - fk <= alpha c1 slope0
            val = f(x)
            alpha = (x[lead] - xk[lead]) / pk[lead]
            if alpha != 0:
                out["armijo"] = min(out["armijo"], abs(val - fk - alpha * C1 * slope0) / scale)
            return val

        def g_seen(x):   # its curvature test on this gradient: <g, pk> >= c2 slope0
            val = g(x)
            if not np.array_equal(x, xk):
                out["curvature"] = min(out["curvature"], abs(float(np.dot(val, pk)) - C2 * slope0) / scale)
            return val

        alpha, fc, gc, new_fval, old_fval, _ = line_search(f=f_seen, myfprime=g_seen, xk=xk, pk=pk, maxiter=50)
        x_last = xk + alpha * pk
        x_last, alpha2 = limit_step_size(x_min=x_min, x_max=x_max, x_last=x_last, xk=xk, pk=pk, alpha=alpha)
        out["clamped"] += int(alpha2 != alpha)
        p_last = -g(x_last)
        new_fval = f(x_last)
        diff = abs(new_fval - old_fval)
        out["evals"].append((fc, gc))
        log(x_last, new_fval)
        improving = not (n_iter > max_iter or diff < min_diff)
    out["n_iter"] = n_iter
    return out


# ---- the fit fixtures ----------------------------------------------------------------------------------------------------------------
BLOCKS = {5: (14, 9), 17: (8, 5), 33: (6, 4), 64: (3, 2)}     # k -> block size: 70 x 45 up to 198 x 132
FIXTURES = [(5, 10), (17, 10), (33, 10), (64, 10), (17, 5), (33, 5), (64, 5)]   # (k, lamda)
MAX_ITER = 6
MARGIN = 1e-7
_fixtures = {}


def draw(k, seed):
    """k disjoint all-ones blocks with 2 % of the cells flipped; U = (0.7 P + 0.3 rand) * scale_c, scale_c ~ U(0.5, 3) per column,
    start thresholds U(0.35, 0.65) * scale; likewise V."""
    br, bc = BLOCKS[k]
    rs = np.random.RandomState(seed)
    X = np.kron(np.eye(k), np.ones((br, bc))) != 0
    X = (X ^ (rs.rand(*X.shape) < 0.02)).astype(np.uint8)
    Pu, Pv = np.kron(np.eye(k), np.ones((br, 1))), np.kron(np.eye(k), np.ones((bc, 1)))
    su, sv = rs.uniform(0.5, 3.0, size=k), rs.uniform(0.5, 3.0, size=k)
    U = (0.7 * Pu + 0.3 * rs.rand(*Pu.shape)) * su
    V = (0.7 * Pv + 0.3 * rs.rand(*Pv.shape)) * sv
    us, vs = rs.uniform(0.35, 0.65, size=k) * su, rs.uniform(0.35, 0.65, size=k) * sv
    return X, U, V, us, vs


def eligible(ref, lam):
    enough = ref["n_iter"] >= 3 if lam == 10 else ref["clamped"] >= 1
    return enough and min(ref["armijo"], ref["curvature"], ref["entry"]) >= MARGIN


def fixture(k, lam):
    """(X, U, V, us, vs, ref) of the first of at most 20 seeds whose restated fit meets the conditions; built once, left unchanged."""
    if (k, lam) not in _fixtures:
        for seed in range(20):
            X, U, V, us, vs = draw(k, seed)
            ref = fit(X, U, V, us, vs, lam, max_iter=MAX_ITER)
            if eligible(ref, lam):
                for a in (X, U, V, us, vs):
                    a.setflags(write=False)
                _fixtures[(k, lam)] = (X, U, V, us, vs, ref)
                break
        else:
            raise AssertionError(f"no eligible seed for the fit fixture k={k}, lamda={lam}")
    return _fixtures[(k, lam)]
