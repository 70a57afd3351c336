"""SimpleThreshold -- grid search over the pair of thresholds (u, v) that binarise given real factors U, V, scored by the Boolean
cover min(1, (U > u) @ (V > v)^T) against X.  The start the reference's tutorials give ``BinaryMFThreshold``
(``examples/ex06_1_BinaryMFThreshold.ipynb`` on NMFSklearn factors, ``examples/ex05_3_FastStep.ipynb`` on FastStep factors).

The reference's module ``PyBMF/models/SimpleThreshold.py`` is not in its tree; what the notebooks stored is the record: the
constructor, the printed parameters and their defaults (``W : full``, ``n_trials : 100``, ``solver : grid-search``, ``init_method :
custom``, ``n_grid : 10`` for the randomised search), "grid search with 1600 trials in total" at ``n_grid=40``, the log
``logs['updates']`` with columns time, iter, u, v and Recall, Precision, Accuracy, F1 under train, a 1-based ``iter``, a u-major
trial order on equal-step grids that start at the factor minimum, and the results ``u``, ``v`` (``us``, ``vs`` when columnwise).

THIS BUILD'S DEFINITIONS (consistent with every recorded fact; where the record is silent they are this build's choice):
  grid        ``np.linspace(F.min(), F.max(), n_grid, endpoint=False)`` over the entries of the dense factor, for U and V each: it
              starts at the minimum, as the recorded values do, and leaves the maximum out because F > max is the empty factor.
              Columnwise: one such grid per column, from that column's minimum and maximum.
  exhaustive  (``randomize=False, columnwise=False``) trial t = a * n_grid + b is (u_a, v_b); ``iter`` = t + 1.
  randomised  ``idx = self.rng.randint(0, n_grid, size=(n_trials, 2))``, trial t is (u_idx[t,0], v_idx[t,1]); columnwise:
              ``size=(n_trials, 2, k)``, ``idx[t, 0, c]`` the index into column c's U grid; ``self.rng`` = ``RandomState(seed)``.
  columnwise without randomize: NotImplementedError (n_grid^(2k) trials).
  best trial  the first, in trial order, whose ``by_metric`` on train is strictly greater than every one before it.
  metrics     from the integer counts by ``utils.scores_from_counts`` (a ratio with an empty denominator is 0).
  n_grid=None means 40 for the exhaustive grid and 10 for the randomised search.

A trial is one Boolean cover count; the thresholded factors of a grid are nested sets, so all trials of the exhaustive search share
one pass over X (``pybmf_amd/thresh_grid.py``, csrc/thresh_grid.hip); the randomised searches run on the pair-list kernel.
After ``fit``: ``u``, ``v`` (floats) or ``us``, ``vs`` (tuples), ``U``, ``V`` as given, ``X_pd`` at the best trial, ``logs['updates']``
with one row per trial (val / test column groups when those sets are given, scored by the same kernels on their own bits), and
``counts_``: the int64 [trials][2] TP / FP array of the train set (this build's addition).

Refused: task='prediction', data that is not 0 / 1, k > 128, a sharded run.  ``W`` is stored and printed; under
task='reconstruction' the scores are whole-matrix, as in the reference's ``evaluate``.
"""
from __future__ import annotations

from itertools import product

import numpy as np

from ..utils import header, ismat, record_many, scores_from_counts, to_dense
from .ContinuousModel import ContinuousModel

METRICS = ["Recall", "Precision", "Accuracy", "F1"]
MAX_K = 128


def threshold_grid(F, n_grid, columnwise=False):
    """The grid of one factor: (n_grid,) floats, or (n_grid, k) with one grid per column."""
    F = np.asarray(F, dtype=np.float64)
    if columnwise:
        return np.stack([np.linspace(F[:, c].min(), F[:, c].max(), n_grid, endpoint=False) for c in range(F.shape[1])], axis=1)
    return np.linspace(F.min(), F.max(), n_grid, endpoint=False)


def best_trial(values):
    """Index of the first trial whose value is strictly greater than every one before it and is not beaten later."""
    best, at = None, 0
    for t, v in enumerate(values):
        if best is None or v > best:
            best, at = v, t
    return at


class SimpleThreshold(ContinuousModel):
    def __init__(self, U, V, W='full', by_metric='F1', columnwise=False, randomize=False, n_grid=None, n_trials=100, normalize_method=None,
                 seed=None):
        if n_grid is None:
            n_grid = 10 if randomize else 40
        self.check_params(U=U, V=V, W=W, by_metric=by_metric, columnwise=columnwise, randomize=randomize, n_grid=n_grid, n_trials=n_trials,
                          normalize_method=normalize_method, solver='grid-search', init_method='custom', seed=seed)

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        if "U" in kwargs:
            self.k = int(self.U.shape[1])
            if self.V.shape[1] != self.k:
                raise ValueError("U and V must have the same number of columns")
            if self.k > MAX_K:
                raise NotImplementedError(f"k={self.k}: this build supports k <= {MAX_K}")
        assert self.solver in ['grid-search']
        assert self.init_method in ['custom']
        assert self.by_metric in METRICS, f"by_metric must be one of {METRICS}"
        assert ismat(self.W) or self.W in ['mask', 'full']
        assert int(self.n_grid) >= 1 and int(self.n_trials) >= 1

    # ---- what is refused, before anything is uploaded ------------------------------------------------------------------------------
    def _refuse(self, X_train, X_val, X_test, kwargs):
        if kwargs.get("task", getattr(self, "task", None)) == "prediction":
            raise NotImplementedError("SimpleThreshold scores whole matrices (task='reconstruction'): its trials are Boolean cover counts, "
                                      "not scores over stored entries")
        for X in (X_train, X_val, X_test):
            if X is not None and not self._values_are_boolean(X):
                raise NotImplementedError("SimpleThreshold takes Boolean (0/1) matrices: a trial is a count of covered ones")
        try:
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        except ImportError:
            world = 1
        if world > 1:
            raise NotImplementedError("SimpleThreshold runs on one GPU: a grid search is one pass over X, there is nothing to shard")
        if self.columnwise and not self.randomize:
            raise NotImplementedError(f"columnwise=True without randomize=True is an exhaustive search over n_grid^(2k) = "
                                      f"{int(self.n_grid)}^{2 * self.k} trials; use randomize=True")

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._refuse(X_train, X_val, X_test, kwargs)
        super().fit(X_train, X_val, X_test, **kwargs)
        self._fit()
        self._engine = None   # (the device copies of the factors and the bits of the extra sets go with it)
        self.X_pd = None   # the Boolean product at the best trial, built on first access
        self.finish(show_logs=self.show_logs, save_model=self.save_model, show_result=self.show_result)

    def init_model(self):
        self._start_timer()
        self._make_name()
        self._init_logs()
        self.U, self.V = np.array(to_dense(self.U), dtype=np.float64), np.array(to_dense(self.V), dtype=np.float64)
        if self.U.shape != (self.m, self.k) or self.V.shape != (self.n, self.k):
            raise ValueError(f"U {self.U.shape} and V {self.V.shape} do not fit X_train {self.m} x {self.n}")
        self.normalize_UV()
        self._engine = self._make_engine()

    def _make_engine(self):
        """The one place the device is touched: a test without a GPU overrides exactly this."""
        from ..engine import BitMatrix
        from ..thresh_grid import ThreshGridEngine
        sets = {"train": BitMatrix(self._X_input, self.device)}
        if sets["train"].max_u8 > 1:
            raise NotImplementedError("SimpleThreshold takes Boolean (0/1) matrices: a trial is a count of covered ones")
        for name, X in (("val", self.X_val), ("test", self.X_test)):
            if X is not None:
                sets[name] = BitMatrix(X, self.device)
        return ThreshGridEngine(sets, self.U, self.V)

    # ---- the search ------------------------------------------------------------------------------------------------------------
    def trials(self):
        """(thr_u, thr_v, pairs, shown): threshold vectors (A, k) and (B, k), the (T, 2) panel pairs of the trials in trial order (None:
        the full grid, u-major), and per trial what the log shows -- (u, v) floats, or (us, vs) tuples when columnwise."""
        n_grid, k = int(self.n_grid), self.k
        gu, gv = threshold_grid(self.U, n_grid, self.columnwise), threshold_grid(self.V, n_grid, self.columnwise)
        if not self.randomize:
            print("[I] grid search with {} trials in total".format(n_grid * n_grid))
            shown = [(float(u), float(v)) for u in gu for v in gv]
            return np.repeat(gu[:, None], k, axis=1), np.repeat(gv[:, None], k, axis=1), None, shown
        n_trials = int(self.n_trials)
        print("[I] randomized grid search with {} trials".format(n_trials))
        if not self.columnwise:
            idx = self.rng.randint(0, n_grid, size=(n_trials, 2))
            shown = [(float(gu[a]), float(gv[b])) for a, b in idx]
            return np.repeat(gu[:, None], k, axis=1), np.repeat(gv[:, None], k, axis=1), idx.astype(np.int32), shown
        idx = self.rng.randint(0, n_grid, size=(n_trials, 2, k))
        cols = np.arange(k)
        thr_u, thr_v = gu[idx[:, 0, :], cols], gv[idx[:, 1, :], cols]
        shown = [(tuple(float(x) for x in thr_u[t]), tuple(float(x) for x in thr_v[t])) for t in range(n_trials)]
        pairs = np.repeat(np.arange(n_trials, dtype=np.int32)[:, None], 2, axis=1)
        return thr_u, thr_v, pairs, shown

    def _fit(self):
        thr_u, thr_v, pairs, shown = self.trials()
        eng = self._engine
        if pairs is None:
            counts = {name: np.asarray(c).reshape(-1, 2) for name, c in eng.grid_counts(thr_u, thr_v).items()}
        else:
            counts = {name: np.asarray(c) for name, c in eng.pair_counts(thr_u, thr_v, pairs).items()}
        names = [name for name in ("train", "val", "test") if name in counts]
        cells = self.m * self.n
        scores = {}
        for name in names:
            sum_x = int(eng.sums[name])
            rows = []
            for tp, fp in counts[name]:
                tp, fp = int(tp), int(fp)
                fn = sum_x - tp
                rows.append(scores_from_counts(tp, fp, fn, cells - tp - fp - fn))
            scores[name] = rows
        by = METRICS.index(self.by_metric)
        best = best_trial([row[by] for row in scores["train"]])
        keys = ["us", "vs"] if self.columnwise else ["u", "v"]
        columns = header(["iter"] + keys, levels=3)
        for name in names:
            columns += list(product([name], [0], METRICS))
        rows = [[t + 1, shown[t][0], shown[t][1]] + [x for name in names for x in scores[name][t]] for t in range(len(shown))]
        record_many(self.logs, "updates", columns, rows)
        self.counts_ = np.asarray(counts["train"], dtype=np.int64)
        self.best_iter = best + 1
        self._best_counts = {}
        for name in names:
            tp, fp = (int(x) for x in counts[name][best])
            fn = int(eng.sums[name]) - tp
            self._best_counts[name] = (tp, fp, fn, cells - tp - fp - fn)
        if self.columnwise:
            self.us, self.vs = shown[best]
        else:
            self.u, self.v = shown[best]
        self.print_msg("best trial {}: {} = {}".format(best + 1, self.by_metric, scores["train"][best][by]))

    # ---- after the fit ---------------------------------------------------------------------------------------------------------
    def _make_X_pd(self):
        from ..device_ops import boolean_product_csr
        if self.columnwise:
            return boolean_product_csr(self.U, self.V, us=np.asarray(self.us), vs=np.asarray(self.vs), device=self.device)
        return boolean_product_csr(self.U, self.V, u=self.u, v=self.v, device=self.device)

    def _score(self, name, metrics):
        """Data set `name` at the best trial, from the counts the search kept."""
        if name not in getattr(self, "_best_counts", {}):
            raise ValueError(f"no {name} data was given to fit()")
        if any(mt in ("RMSE", "MAE") for mt in metrics):
            raise NotImplementedError("SimpleThreshold scores the Boolean metrics only")
        return self._metric_values(metrics, None, self._best_counts[name])
