"""HyperPlus -- a Hyper model's hyperrectangles merged under a false-positive budget.  Drop-in for ``PyBMF/models/HyperPlus.py``
(Xiang et al., Summarizing Transactional Databases with Overlapped Hyperrectangles: the Hyper+ half).

``HyperPlus(model, target_k, samples=500, beta=np.inf, savings='reference')`` imports U, V, T, I, k and the logs of a fitted Hyper
(a ``pybmf_amd`` Hyper, or any object with those six attributes; the model object itself is not kept).  fit() then runs rounds.  A
round samples up to `samples` of the k (k - 1) / 2 pairs of factors, tries each: the pair (m, n) would be replaced by the one rectangle
(T_m | T_n) x (I_m | I_n), which costs false positives; fpb = FP / |X| of that trial must not exceed `beta`.  One of the trials that
fit is merged, and the rounds go on while the budget holds and k >= target_k.

The reference rebuilds the Boolean product of the other k - 2 factors for every trial.  Here a round is one launch and one read
(csrc/hyperplus.hip through ``pybmf_amd/hyperplus.py``): the merged rectangle contains both rectangles it replaces, so the trial's
prediction is the current one OR the rectangle and FP(trial) = FP + new_fp, new_fp = the zero cells of X in T x I that nothing covers
yet -- an AND-popcount pass over |I| column bit rows per pair.  The device returns integers; fpb, the savings and their comparisons are
host fp64 by the reference's expressions.

Kept from the reference, on purpose:
  * savings='reference': cost_savings divides by |T| |I| minus the ones of the trial's prediction on T x I -- a prediction that already
    holds the merged rectangle, so the denominator is 0 and the savings inf for every pair.  best_savings starts at 0 and the test is
    a strict `>`: THE FIRST PAIR IN LIST ORDER THAT FITS THE BUDGET IS MERGED, every later trial of the round changes nothing, and the
    `savings` column of the log is inf in every row.
  * the budget test skips a trial on `fpb > beta`: a trial whose fpb equals beta fits.
  * the stop rule `fpb <= beta and k >= target_k` is tested after a merge: a run ends one below target_k (target_k=3 ends at k = 2)
    unless the budget, or a round in which no trial fits, ends it before.  At k = 1 the pair list is empty and the run ends.
  * the pair list: a = k (k - 1) / 2, np.random.choice(a=a, size=min(samples, a), replace=False) on NumPy's GLOBAL generator (so
    np.random.seed(s) before fit() gives the reference's pairs); the pairs ascend in m, inside one m they keep the order of their
    indices in the sample; index i of row m is n = i - idx_0(m) + m + 1 with idx_0(m) = 0.5 m ((k - 1) + (k - m)).
  * the merged factor goes last, the others keep their order: in T, I, U, V and in every logs['U'] / ['V'] entry (lil copies, one
    per round).
  * `logs` is the imported model's own dict: after a fit the Hyper model's logs hold 'U', 'V' and 'refinements' too, a second
    HyperPlus on the same Hyper appends its rows to the same frame and resets logs['U'] / ['V'] to [].  The Hyper model's U, V, T,
    I, k are not modified.
  * FPR = 1 - TN / (m n - |X|), FPB = FP / |X|, OCR = FP / |X_pd| of the merged prediction, from the integer counts.
Different from the reference:
  * np.Inf does not exist in NumPy 2: the reference raises AttributeError at the first trial that fits the budget.  This build
    uses np.inf and does not raise.
  * savings='new_fp' is this build's own: savings = (|T_m & T_n| + |I_m & I_n|) / new_fp in fp64 (the description length saved per
    false positive added), inf when new_fp = 0; the same strict `>` against the best so far, the same list order, the same budget
    test.  A pair that shares no row and no column saves 0 and is never merged.  Any other value of `savings` is refused.
  * `model.T[i]` and `model.I[i]` ascend (the reference: the iteration order of a set); both are sets.
  * a k of None raises TypeError, T / I lists whose length is not k, and U / V whose shapes do not match X and k, raise ValueError
    (the reference fails somewhere inside the first round).  The one state accepted with fewer sets than k is what Hyper leaves when
    it ran no round: k = 1, no set, one empty column.

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any k whose 2 k bit rows fit
beside the two bit matrices of m_pad x n_pad bits, one GPU.  task='prediction' raises NotImplementedError.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import hstack, issparse, lil_matrix

from .Hyper import Hyper

SAVINGS = ("reference", "new_fp")


class HyperPlus(Hyper):
    title = "HyperPlus"

    def __init__(self, model, target_k, samples=500, beta=np.inf, savings="reference"):
        self.check_params(model=model, target_k=target_k, samples=samples, beta=beta, savings=savings)

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        assert self.beta is not None or self.target_k is not None, "Please specify beta or target_k or both."
        if self.savings not in SAVINGS:
            raise ValueError(f"savings must be one of {SAVINGS}, not {self.savings!r}")
        if 'model' in kwargs:
            model = kwargs.get('model')
            self.import_model(U=model.U, V=model.V, T=model.T, I=model.I, k=model.k, logs=model.logs)
            # the model itself is not kept: finish() pickles every public attribute, and a fitted pybmf_amd model holds device
            # handles (its engine) that do not pickle and device memory that should not outlive it here
            del self.model
            print("[I] k from model :", self.k)

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        if self.k is None:
            raise TypeError(f"{self.title} needs the number of factors of the imported model: its k is None")
        super().fit(X_train, X_val, X_test, **kwargs)

    def init_model(self):
        super().init_model()                  # the factors and the logs exist: neither is initialised
        n_sets = len(self.T)
        if len(self.I) != n_sets or (n_sets != self.k and not (n_sets == 0 and self.k == 1)):
            raise ValueError(f"the imported model has {n_sets} row sets and {len(self.I)} column sets; its k is {self.k}")
        if self.U.shape != (self.m, self.k) or self.V.shape != (self.n, self.k):
            raise ValueError(f"the imported factors have shapes {self.U.shape}, {self.V.shape}; X is {self.m} x {self.n} and k = {self.k}")

    def _engine_class(self):
        from ..hyperplus import HyperPlusEngine
        return HyperPlusEngine

    def _sample_pairs(self):
        """The pair list of a round, as list positions (m, n), m < n."""
        k = self.k
        a = int(k * (k - 1) / 2)
        pairs_idx = np.random.choice(a=a, size=int(min(self.samples, a)), replace=False)
        first = np.array([0.5 * m * ((k - 1) + (k - m)) for m in range(max(k, 1))])          # idx_0(m): the index of pair (m, m + 1)
        m_of = np.searchsorted(first, pairs_idx, side="right") - 1
        by_m = np.argsort(m_of, kind="stable")                                              # ascending m, sample order inside one m
        return [(int(m_of[i]), int(pairs_idx[i] - first[m_of[i]] + m_of[i] + 1)) for i in by_m]

    def _rates(self):
        """(FPR, FPB, OCR) of the prediction against X_train by the reference's expressions, from the integer counts."""
        tp, fp, fn, tn = (np.float64(c) for c in self._counts_of("train"))
        with np.errstate(divide="ignore", invalid="ignore"):
            return 1 - (tn / (tn + fp) if tn + fp > 0 else 0), fp / (tp + fn), fp / (tp + fp)

    def _fit(self):
        from ..bitset import bit_positions
        eng = self._engine
        eng.load_factors(self.T, self.I)
        self._invalidate()
        sum_x = np.float64(eng.sum_x)
        _, fpb, _ = self._rates()
        self.logs['U'], self.logs['V'] = [], []
        self.trials = []          # per round: [(m, n, FP, fpb, savings or None where the budget refused the trial)], and the chosen pair
        is_improving = True
        while is_improving:
            pairs = self._sample_pairs()
            print("[I] Sampled {} pairs. Current FP budget: {:.3f}".format(len(pairs), fpb))
            fp_now = self._counts_of("train")[1]
            new_fp, _, _, n_tc, n_ic = eng.score_pairs([(eng.order[m], eng.order[n]) for m, n in pairs])
            best, best_savings, trials = None, 0, []
            for i, (m, n) in enumerate(pairs):
                with np.errstate(divide="ignore", invalid="ignore"):
                    fpb = np.float64(fp_now + new_fp[i]) / sum_x
                if fpb > self.beta:
                    trials.append((m, n, int(fp_now + new_fp[i]), float(fpb), None))
                    continue
                if self.savings == "reference" or new_fp[i] == 0:
                    savings = np.inf
                else:
                    savings = np.float64(n_tc[i] + n_ic[i]) / np.float64(new_fp[i])
                trials.append((m, n, int(fp_now + new_fp[i]), float(fpb), float(savings)))
                if savings > best_savings:
                    best, best_savings = (m, n), savings
            self.trials.append((trials, best))
            if best is None:
                break
            words_T, words_I = eng.merge(eng.order[best[0]], eng.order[best[1]])
            T = [int(t) for t in bit_positions(words_T) if t < self.m]
            I = [int(j) for j in bit_positions(words_I) if j < self.n]
            others = [i for i in range(self.k) if i not in best]
            self.T, self.I = [self.T[i] for i in others] + [T], [self.I[i] for i in others] + [I]
            u, v = lil_matrix((self.m, 1)), lil_matrix((self.n, 1))
            if T:
                u[T] = 1
            if I:
                v[I] = 1
            self.U = hstack([_lil(self.U)[:, others], u], format='lil')
            self.V = hstack([_lil(self.V)[:, others], v], format='lil')
            self.logs['U'].append(self.U.copy())
            self.logs['V'].append(self.V.copy())
            self.k = self.U.shape[1]
            self._invalidate()
            fpr, fpb, ocr = self._rates()
            self.evaluate(df_name='refinements', head_info={'k': self.k, 'savings': best_savings, 'FPR': fpr, 'FPB': fpb, 'OCR': ocr})
            is_improving = bool(fpb <= self.beta and self.k >= self.target_k)


def _lil(F):
    return F.tolil() if issparse(F) else lil_matrix(np.asarray(F))
