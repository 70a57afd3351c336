"""The loop driver of the multiplicative-update models (models/ContinuousModel.mu_loop) on a fake engine, no GPU needed: the pipelined
path (iteration t + 1 enqueued before the scalars of t are read) and the stepwise path take the same decisions and return the same
rows, n_iter, reg and factors, whichever rule stops the loop."""
import numpy as np
import pytest

from pybmf_amd.models.BaseModelTools import BaseModelTools
from pybmf_amd.models.ContinuousModel import mu_loop


class Rule(BaseModelTools):
    def __init__(self, tol, min_diff, max_iter):
        self.tol, self.min_diff, self.max_iter = tol, min_diff, max_iter


class FakeEngine:
    """State = the regularisers of the updates applied so far; the scalars are a function of that state and of the `reg` they are
    decoded with, like the real engines' rows."""

    def __init__(self, pipelined):
        self.pipelined = pipelined
        self.regs = []        # one entry per update applied
        self.calls = []
        self.rows = {}        # iteration -> state its row was taken from (the enqueued rows)
        self.prev = None

    def can_pipeline(self):
        return self.pipelined

    def prepare(self):
        self.calls.append(("prepare",))

    def load_factors(self, U, V):
        self.calls.append(("load_factors",))
        self.regs = list(V)

    def factors(self):
        return np.array([float(len(self.regs))]), np.array(self.regs, dtype=np.float64)

    def _scalars(self, regs, reg):
        c = len(regs)
        rec = 1.0 + 8.0 / (c + 1) + 0.01 * sum(regs)
        rg = reg * 0.5 ** c
        return rec + rg, rec, rg, np.sqrt(rec), rec / 3, (c, 1, 2, 3)

    # stepwise protocol
    def update(self, reg):
        self.calls.append(("update", reg))
        self.regs.append(reg)

    def scalars(self, reg):
        self.calls.append(("scalars", reg))
        return self._scalars(self.regs, reg)

    # pipelined protocol
    def iterate(self, it, reg, update=True):
        self.calls.append(("iterate", it, reg, update))
        assert update == (it > 0)
        if update:
            self.prev = self.factors()
            self.regs.append(reg)
        self.rows[it] = list(self.regs)

    def row(self, it, reg):
        self.calls.append(("row", it, reg))
        assert it in self.rows, f"row {it} was never enqueued"
        assert ("iterate", it + 1) in [c[:2] for c in self.calls], f"row {it} read before iteration {it + 1} was enqueued"
        return self._scalars(self.rows[it], reg)

    def previous_factors(self):
        return self.prev


def run(pipelined, rule, value=0, scored=False):
    eng = FakeEngine(pipelined)
    rows = []

    def on_row(it, reg, scalars):
        rows.append((it, reg) + tuple(scalars))
        return scalars[value]
    n_iter, reg, (U, V) = mu_loop(eng, np.float64(1.0), on_row, rule.early_stop, growth=np.float64(3.0), max_reg=np.float64(20.0),
                                  scored=scored)
    return eng, rows, n_iter, reg, U, V


@pytest.mark.parametrize("stop", ["max_iter", "min_diff", "tol"])
@pytest.mark.parametrize("value", [0, 2])   # the rule on the error (WNMF) or on reg_error (BinaryMFPenalty / PNLPF)
def test_pipelined_and_stepwise_loops_agree(stop, value):
    max_iter = 7
    rule = {"max_iter": Rule(0.0, 0.0, max_iter),
            "min_diff": Rule(0.0, 0.28 if value == 0 else 0.2, max_iter),
            "tol": Rule(3.3 if value == 0 else 0.35, 0.0, max_iter)}[stop]
    eng_p, rows_p, n_p, reg_p, U_p, V_p = run(True, rule, value)
    eng_s, rows_s, n_s, reg_s, U_s, V_s = run(False, rule, value)

    assert rows_p == rows_s and n_p == n_s and reg_p == reg_s
    assert np.array_equal(U_p, U_s) and np.array_equal(V_p, V_s)
    if stop == "max_iter":
        assert n_p == max_iter + 1
    else:
        assert 2 <= n_p < max_iter
    # the regulariser schedule: min(reg * growth, max_reg), and reg ends one growth step past the last update
    sched = [1.0, 3.0, 9.0, 20.0] + [20.0] * 20
    assert [r[1] for r in rows_p] == [1.0] + sched[:n_p]
    assert list(V_p) == sched[:n_p] and reg_p == sched[n_p]

    # stepwise: n_iter updates; pipelined: exactly one more update enqueued than returned, its factors loaded back
    assert [c[0] for c in eng_s.calls].count("update") == n_s and "iterate" not in [c[0] for c in eng_s.calls]
    iters = [c for c in eng_p.calls if c[0] == "iterate"]
    assert [c[1] for c in iters] == list(range(n_p + 2))
    assert sum(c[3] for c in iters) == n_p + 1 == int(U_p[0]) + 1
    assert eng_p.calls[-1] == ("load_factors",) and np.array_equal(eng_p.factors()[1], V_p)
    # the call order: iterate(0, update=False), iterate(1), row(0), then iterate(n + 1) / row(n)
    want = [("iterate", 0, 1.0, False), ("iterate", 1, 1.0, True), ("row", 0, 1.0)]
    for n in range(1, n_p + 1):
        want += [("iterate", n + 1, sched[n], True), ("row", n, sched[n - 1])]
    assert eng_p.calls[:-1] == want
    assert "scalars" not in [c[0] for c in eng_p.calls] and "update" not in [c[0] for c in eng_p.calls]


def test_extra_data_sets_take_the_stepwise_path():
    eng, rows, n_iter, _, _, _ = run(True, Rule(0.0, 0.0, 3), scored=True)
    kinds = [c[0] for c in eng.calls]
    assert "iterate" not in kinds and "row" not in kinds and kinds.count("update") == n_iter == 4
