"""The NumPy statement of SimpleThreshold's search: grids, trial order, draws, counts, metrics and the best pick.  Plain helpers, no
tests; tests/test_simple_threshold_cpu.py, test_thresh_grid_kernels_gpu.py and test_simple_threshold_gpu.py hold the model and the
kernels to it.  Nothing here imports pybmf_amd: the counts of a trial are formed as ((U > u) @ (V > v).T > 0) against X.

Definitions (those of the issue; the reference's module is absent, its notebooks are the record):
  grid        np.linspace(F.min(), F.max(), n_grid, endpoint=False); columnwise: per column
  exhaustive  trial t = a * n_grid + b is (u_a, v_b), iter = t + 1
  randomised  idx = RandomState(seed).randint(0, n_grid, size=(n_trials, 2)); columnwise size=(n_trials, 2, k), [t, 0, c] = U's column c
  best        the first trial, in order, strictly greater in by_metric than every one before it (and never beaten after)
  metrics     Recall, Precision, Accuracy, F1 from TP, FP, FN, TN; a ratio with an empty denominator is 0
"""
import numpy as np

METRICS = ["Recall", "Precision", "Accuracy", "F1"]


def grid(F, n_grid, columnwise=False):
    F = np.asarray(F, dtype=np.float64)
    if columnwise:
        return np.stack([np.linspace(F[:, c].min(), F[:, c].max(), n_grid, endpoint=False) for c in range(F.shape[1])], axis=1)
    return np.linspace(F.min(), F.max(), n_grid, endpoint=False)


def product(Ub, Vb):
    """Boolean product of two Boolean factors (fp32 sums of 0 / 1 products are exact integers below 2^24 terms)."""
    return (Ub.astype(np.float32) @ Vb.astype(np.float32).T) > 0


def counts_of(X, Ub, Vb):
    """(TP, FP) of the Boolean product against the 0 / 1 matrix X."""
    P, Xb = product(Ub, Vb), np.asarray(X) != 0
    return int((P & Xb).sum()), int((P & ~Xb).sum())


def metrics_of(tp, fp, sum_x, cells):
    fn = sum_x - tp
    tn = cells - tp - fp - fn
    recall = tp / (tp + fn) if tp + fn > 0 else 0
    precision = tp / (tp + fp) if tp + fp > 0 else 0
    accuracy = (tp + tn) / cells
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0
    return [recall, precision, accuracy, f1]


def trial_thresholds(U, V, n_grid=None, columnwise=False, randomize=False, n_trials=100, seed=None):
    """[(thr_u, thr_v)] per trial, in trial order: floats, or k-vectors when columnwise."""
    if n_grid is None:
        n_grid = 10 if randomize else 40
    if columnwise and not randomize:
        raise NotImplementedError("n_grid^(2k) trials")
    gu, gv = grid(U, n_grid, columnwise), grid(V, n_grid, columnwise)
    if not randomize:
        return [(gu[t // n_grid], gv[t % n_grid]) for t in range(n_grid * n_grid)]
    rng = np.random.RandomState(seed)
    k = np.asarray(U).shape[1]
    if not columnwise:
        idx = rng.randint(0, n_grid, size=(n_trials, 2))
        return [(gu[idx[t, 0]], gv[idx[t, 1]]) for t in range(n_trials)]
    idx = rng.randint(0, n_grid, size=(n_trials, 2, k))
    return [(np.array([gu[idx[t, 0, c], c] for c in range(k)]), np.array([gv[idx[t, 1, c], c] for c in range(k)])) for t in range(n_trials)]


def best_of(values):
    best, at = None, None
    for t, v in enumerate(values):
        if at is None or v > best:
            best, at = v, t
    return at


def search(X, U, V, by_metric="F1", extra=None, **kw):
    """The whole search.  Returns dict(thresholds=[(u, v)], counts={set: int64 [T][2]}, metrics={set: [T][4]}, best=index, margin=
    by_metric of the best trial minus the largest value among the trials whose counts differ from its counts (inf when none does))."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    thr = trial_thresholds(U, V, **kw)
    sets = {"train": np.asarray(X)}
    sets.update(extra or {})
    # thresholded factors are shared by the trials that name the same threshold
    cache = {}

    def bits(F, t, tag):
        key = (tag, np.asarray(t, dtype=np.float64).tobytes())
        if key not in cache:
            cache[key] = F > t
        return cache[key]
    counts, metrics = {}, {}
    pcache = {}
    for name, Xs in sets.items():
        Xb = np.asarray(Xs) != 0
        sum_x, cells = int(Xb.sum()), Xb.size
        rows = []
        for u, v in thr:
            key = (np.asarray(u, dtype=np.float64).tobytes(), np.asarray(v, dtype=np.float64).tobytes())
            if key not in pcache:
                pcache[key] = product(bits(U, u, "u"), bits(V, v, "v"))
            P = pcache[key]
            rows.append((int((P & Xb).sum()), int((P & ~Xb).sum())))
        counts[name] = np.array(rows, dtype=np.int64)
        metrics[name] = [metrics_of(tp, fp, sum_x, cells) for tp, fp in rows]
    col = METRICS.index(by_metric)
    vals = [row[col] for row in metrics["train"]]
    best = best_of(vals)
    # the runner-up: the best value among the trials whose COUNTS differ from the best trial's.  Trials with the same counts (grid
    # points between two neighbouring factor values give the same bits) have the same value to the last bit in any implementation,
    # and among them "the first" is not a matter of rounding; a near-tie between different counts would be.
    top = tuple(counts["train"][best])
    others = [v for v, c in zip(vals, counts["train"]) if tuple(c) != top]
    margin = vals[best] - max(others) if others else float("inf")
    return dict(thresholds=thr, counts=counts, metrics=metrics, best=best, margin=margin)
