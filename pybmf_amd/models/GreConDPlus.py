"""GreConD+ -- approximate Boolean decomposition that admits overcovering.  Drop-in for ``PyBMF/models/GreConDPlus.py`` (A new
algorithm for Boolean matrix factorization which admits overcovering).

Each factor starts as the concept GreConD would take (the same search, csrc/grecond.hip) and is then EXPANDED greedily, one row or one
column per step, while the weighted coverage score  -w_fp FP + w_fn TP  of the best candidate line improves; a factor that the new one
covers entirely is dropped, extension rows and columns that other factors cover twice are pruned, and X_pd / X_rs are rebuilt from the
factors that survive.  Counts, the expansion steps, the rebuild and the pruning run on the bits in HBM (csrc/grecondplus.hip through
``pybmf_amd/grecondplus.py``); the loop over factors, remove_covered (a subset test on packed words), the log and the stopping rules
are host control flow as in the reference.  Factors, extensions, scores and step sequences are the reference's, bit for bit.

Kept from the reference, on purpose:
  * the expansion scores a candidate row by the ones of X it would cover that are ALREADY covered (x & ~rs) against the zeros, not by
    residual ones; the residual it reads is fixed while a factor expands; equal positive row and column scores stop the expansion.
  * with k given, init_model makes k empty factors and the first remove_covered() drops the k - 1 behind the first: afterwards
    k = U.shape[1], so the `k` column of the log repeats values and "Reach requested factor" counts the log's k, not the factors.
  * remove_overlapped() takes the rows and columns of a factor before its row loop: the column loop still reads the rows just
    removed, with their counts already decremented, and decrements them a second time.
  * early_stop(error=..., k=k): "Error <= tolerance" truncates U and V to [:, :k] while U_exp, V_exp, X_pd and the log keep what was
    there; `shape` in the log is the factor as set, before pruning.
Different from the reference: when no pattern is left (score 0) the reference's own early_stop fails with a TypeError (it calls
_early_stop without `verbose`); here that stop works and leaves the factors found so far (U_exp and V_exp cut to the same columns).
And remove_overlapped() does remove: with a current SciPy the reference raises NotImplementedError at its first removal
(`coverage[i, j_idx] -= 1` on a csr matrix), which no fit of the fixtures reaches; here the lines run as they are written, held to the
reference run on the same counts in a dense container (tests/golden/make_golden_grecondplus.py).

Supported: Boolean X (anything else is refused), task='reconstruction' with or without X_val / X_test, any number of factors, up to
32256 rows (the limit of the concept scan), one GPU.  task='prediction' raises NotImplementedError, as in GreConD.  The pruning builds
the count matrix U @ V.T (m x n int32) only when a row or column passes the subset prefilter, and raises NotImplementedError when it
does not fit in free device memory.  fit(..., steps=N) sets the number of expansion steps per launch (default: a whole expansion),
fit(..., block=N) the candidates per launch of the concept scan; every value gives the same result.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import lil_matrix

from .GreConD import GreConD


def _inside(a, b) -> bool:
    """Packed set a is a subset of packed set b."""
    return not (a & ~b).any()


class GreConDPlus(GreConD):
    title = "GreConD+"

    def __init__(self, k=None, tol=0, w_fp=0.5, w_fn=None):
        if w_fp is None:
            raise ValueError("w_fp must be a finite number")
        self.check_params(k=k, tol=tol, w_fp=w_fp, w_fn=w_fn)

    def check_params(self, **kwargs):
        for name in ("w_fp", "w_fn"):
            w = kwargs.get(name)
            if w is not None and not (isinstance(w, (int, float, np.integer, np.floating)) and np.isfinite(w)):
                raise ValueError(f"{name} must be a finite number" + (" or None" if name == "w_fn" else ""))
        k = kwargs.get("k")
        if k is not None and not (isinstance(k, (int, np.integer)) and k >= 1):
            raise ValueError("k must be a positive integer or None")
        super().check_params(**kwargs)

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        self._steps = kwargs.pop("steps", None)
        if self._steps is not None and not (isinstance(self._steps, (int, np.integer)) and self._steps >= 1):
            raise ValueError("steps must be a positive integer or None")
        for name in ("U", "V", "U_exp", "V_exp"):
            self.__dict__.pop(name, None)
        super().fit(X_train, X_val, X_test, **kwargs)

    def _engine_class(self):
        from ..grecondplus import ExpansionEngine
        return ExpansionEngine

    # the factors live as packed words (f x W, f x nvw) while the fit runs; U, V, U_exp, V_exp are made from them when it ends
    def truncate_factors(self, k):
        self._Ub, self._Vb = self._Ub[:k], self._Vb[:k]

    def _fit(self):
        from ..bitset import unpack_bits
        eng = self._engine
        W, nvw = eng.W, eng.nvw
        w_fp = float(self.w_fp)
        w_fn = 1 - w_fp if self.w_fn is None else float(self.w_fn)      # coverage_score(): w_fn = 1 - w_fp
        k0 = self.k if self.k is not None else 1                       # init_model: k empty factors, or one
        self._Ub, self._Vb = np.zeros((k0, W), dtype=np.uint32), np.zeros((k0, nvw), dtype=np.uint32)
        Ue = Ve = None
        self.n_steps, self.n_covered, self.n_pruned = [], [], []
        k = 0
        is_factorizing = True
        while is_factorizing:
            score, u, v = eng.concept(block=self._block)
            if score == 0:
                is_factorizing = self.early_stop(msg="No pattern found", k=k)
                if Ue is not None:
                    Ue, Ve = Ue[:k], Ve[:k]
                break
            u_exp, v_exp, n_iter = eng.expand(u, v, w_fp, w_fn, steps=self._steps)
            self.n_steps.append(n_iter)
            u, v = u | u_exp, v | v_exp
            # set_factors(k), set_extensions(k)
            Ub, Vb = self._Ub, self._Vb
            if Ub.shape[0] < k + 1:
                Ub = np.vstack([Ub, np.zeros((k + 1 - Ub.shape[0], W), dtype=np.uint32)])
                Vb = np.vstack([Vb, np.zeros((k + 1 - Vb.shape[0], nvw), dtype=np.uint32)])
            if Ue is None:
                Ue, Ve = np.zeros((1, W), dtype=np.uint32), np.zeros((1, nvw), dtype=np.uint32)
            if Ue.shape[0] < k + 1:
                Ue = np.vstack([Ue, np.zeros((k + 1 - Ue.shape[0], W), dtype=np.uint32)])
                Ve = np.vstack([Ve, np.zeros((k + 1 - Ve.shape[0], nvw), dtype=np.uint32)])
            Ub[k], Vb[k], Ue[k], Ve[k] = u, v, u_exp, v_exp
            n_u, n_v = int(unpack_bits(u, self.m).sum()), int(unpack_bits(v, self.n).sum())
            # remove_covered(k): every other factor that lies inside the k-th
            keep = [i for i in range(Ub.shape[0]) if i == k or not (_inside(Ub[i], u) and _inside(Vb[i], v))]
            self.n_covered.append(Ub.shape[0] - len(keep))
            print("[I]     remove_covered() finished with {} patterns removed.".format(Ub.shape[0] - len(keep)))
            if len(keep) != Ub.shape[0]:
                Ub, Vb, Ue, Ve = Ub[keep], Vb[keep], Ue[keep], Ve[keep]
            # remove_overlapped(), then X_pd and X_rs from what is left
            Ub, Vb, Ue, Ve = eng.prune_overlapped(Ub, Vb, Ue, Ve)
            self.n_pruned.append(tuple(eng.pruned))
            self._Ub, self._Vb = Ub, Vb
            eng.rebuild(Ub, Vb)
            self._invalidate()
            self.evaluate(df_name='updates', head_info={'k': k, 'score': score, 'shape': [n_u, n_v]})
            error = self._train_error()
            print("[I] k: {}, score: {}, error: {:.3f}, shape: [{}, {}]".format(k, score, error, n_u, n_v))
            is_factorizing = self.early_stop(error=error, n_factor=k + 1, k=k)
            k = Ub.shape[0]
        self._export(Ue, Ve)

    def _export(self, Ue, Ve):
        """U, V, U_exp, V_exp as the reference leaves them: lil, float, one column per factor."""
        from ..bitset import unpack_bits

        def lil(B, length):
            B = np.zeros((0, 1), dtype=np.uint32) if B is None else B
            out = lil_matrix((length, B.shape[0]))
            for i in range(B.shape[0]):
                rows = np.nonzero(unpack_bits(B[i], length))[0]
                if rows.size:
                    out[rows, i] = 1.0
            return out
        self.U, self.V = lil(self._Ub, self.m), lil(self._Vb, self.n)
        self.U_exp, self.V_exp = lil(Ue, self.m), lil(Ve, self.n)
