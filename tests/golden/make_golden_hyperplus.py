#!/usr/bin/env python3
"""Generate g31_hyperplus.{npz,json} by running the *reference* HyperPlus (PyBMF @ 2024_10_08) on a reference Hyper.

Runs only where the reference is mounted (see make_golden.py, whose loader this script uses); nothing of the reference is written
here, only inputs and recorded outputs.

    python tests/golden/make_golden_hyperplus.py          (a quarter of a minute: four Hyper fits come first)

Hyper is fitted exactly as make_golden_hyper.py fits it.  Put in place of what the reference's modules see:
  * Hyper module: `apriori` and `np` (the stand-in miner and the StableNumpy proxy) as in make_golden_hyper.py.
  * HyperPlus module: `np`, a proxy of NumPy that also has `Inf` (NumPy 2 dropped the name; the unpatched module raises
    AttributeError at the first trial that passes beta).  np.random is NumPy's own: the pairs come from the global generator.
  * HyperPlus module: `cost_savings` and `FP`, wrapped to record what they return; a line tracer on _fit reads m, n and fpb at the
    budget test and the pair list and the chosen pair at the end of a round.
Cases (X and the Hyper model of g30's cases):
  a  g30 a, samples 500 (all 10 pairs), beta inf, target_k 1       a merge run down to k = 1
  b  g30 a, samples 3                                                a sample smaller than the pair count; the order inside one m
  c  g30 a, beta between the least first-round fpb and the next     trials refused before one passes; a later round in which none does
  d  g30 a, beta below every first-round fpb                         no merge, no `refinements`, logs['U'] == []
  e  g30 a, target_k 3                                               the run ends at k = 2
  f  g30 a, beta = the float fpb of a first-round trial (the second   that trial is accepted (`>` is strict)
     smallest value; the pair with the smallest is listed later)
  g  g30 b, 33 x 65, samples 20, target_k 70                         a larger k
  h  g30 h, train / val / test, target_k 28, samples 40              the split
  i  g30 f, X of zeros (Hyper leaves k = 1, T = I = [])              no round
  j  a second HyperPlus on the Hyper model of case a, after case a's  the shared, appended log
Recorded per case: X (val / test), the Hyper model's T, I, U, V, k, the arguments and the seed, per round the pair list in order, per
trial (m, n, FP, fpb, savings; savings null where the budget refused the trial) and the chosen pair, every `refinements` row without
the time stamp, logs['U'] / ['V'] per round, the final T, I, U, V, k and TP / FP / FN / TN, and what the Hyper model holds afterwards.

Asserted here: every traced savings is inf; every fpb-vs-beta decision is either an equality (the floats are equal and beta is the
fp64 quotient of that trial's own integers) or more than 1e-9 apart, so no recorded decision hangs on a rounding.
"""
import json
import os
import sys

import numpy as np
from scipy.sparse import csr_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FIT_KW, counts_of, load_reference, quiet  # noqa: E402
from make_golden_grecond import deal, dense_u8, planted  # noqa: E402
from make_golden_hyper import apriori  # noqa: E402
from make_golden_mebf import StableNumpy  # noqa: E402


class InfNumpy:
    """NumPy with the `Inf` of NumPy 1."""
    Inf = np.inf

    def __getattr__(self, name):
        return getattr(np, name)


def sp(A):
    return None if A is None else csr_matrix(A.astype(np.float64))


def fit_hyper(X, min_support, X_val=None, X_test=None):
    from PyBMF.models import Hyper
    mod = sys.modules["PyBMF.models.Hyper"]
    saved = mod.np, mod.apriori
    mod.np, mod.apriori = StableNumpy(True), lambda df, min_support: apriori(df, min_support)[["support", "itemsets"]].copy()
    try:
        with quiet():
            model = Hyper(min_support=min_support)
            model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
    finally:
        mod.np, mod.apriori = saved
    return model


def flat_log(df):
    """The frame without the time stamp: k an int, everything else a float (savings is inf)."""
    cols = [str(c[-1]) if c[0] == "" else "{}/{}".format(c[0], c[-1]) for c in df.columns]
    keep = [i for i, name in enumerate(cols) if name != "time"]
    rows = [[int(r[i]) if cols[i] == "k" else float(r[i]) for i in keep] for r in df.values.tolist()]
    return {"columns": [cols[i] for i in keep], "rows": rows}


def sets_of(model):
    return [sorted(int(t) for t in T) for T in model.T], [sorted(int(j) for j in I) for I in model.I]


def snapshot(model):
    T, I = sets_of(model)
    return dict(T=T, I=I, k=int(model.k), U=dense_u8(csr_matrix(model.U)), V=dense_u8(csr_matrix(model.V)))


def run_plus(PyBMF, hyper, X, seed, X_val=None, X_test=None, **args):
    """One reference HyperPlus on `hyper`; the recorded run as a dict (arrays under U, V, log_U, log_V)."""
    from PyBMF.models import HyperPlus
    mod = sys.modules["PyBMF.models.HyperPlus"]
    with open(mod.__file__) as fh:
        src = fh.read().split("\n")
    budget_line = 1 + next(i for i, line in enumerate(src) if "if fpb > self.beta" in line)
    round_line = 1 + next(i for i, line in enumerate(src) if "if best_m is None" in line)
    sum_x = int(X.sum())
    rounds, trials, fps, decisions = [], [], [], []

    def local_trace(frame, event, arg):
        if event == "line" and frame.f_lineno == budget_line:
            loc = frame.f_locals
            fp, fpb, beta = int(fps[-1]), float(loc["fpb"]), float(loc["self"].beta)
            assert np.float64(fp) / np.float64(sum_x) == fpb
            equal = fpb == beta
            assert abs(fpb - beta) > 1e-9 or (equal and int(round(beta * sum_x)) == fp), (fpb, beta)
            decisions.append(bool(equal))
            trials.append([int(loc["m"]), int(loc["n"]), fp, fpb, None])
        if event == "line" and frame.f_lineno == round_line:
            loc = frame.f_locals
            chosen = None if loc["best_m"] is None else [int(loc["best_m"]), int(loc["best_n"])]
            rounds.append(dict(k=int(loc["self"].k), pairs=[[int(a), int(b)] for a, b in loc["pairs"]], trials=list(trials), chosen=chosen))
            del trials[:]
        return local_trace

    def tracer(frame, event, arg):
        return local_trace if frame.f_code.co_name == "_fit" and frame.f_code.co_filename == mod.__file__ else None

    saved = mod.np, mod.cost_savings, mod.FP
    ref_savings, ref_FP = mod.cost_savings, mod.FP

    def cost_savings(*a):
        s = ref_savings(*a)
        assert s == np.inf, s
        trials[-1][4] = float(s)
        return s

    def FP(gt, pd):
        fps.append(ref_FP(gt=gt, pd=pd))
        return fps[-1]
    mod.np, mod.cost_savings, mod.FP = InfNumpy(), cost_savings, FP
    before = snapshot(hyper)
    try:
        with quiet():
            model = HyperPlus(model=hyper, **args)
            np.random.seed(seed)
            sys.settrace(tracer)
            try:
                model.fit(sp(X), sp(X_val), sp(X_test), **FIT_KW)
            finally:
                sys.settrace(None)
    finally:
        mod.np, mod.cost_savings, mod.FP = saved
    assert model.logs is hyper.logs
    after = snapshot(hyper)
    assert all(np.array_equal(before[key], after[key]) if key in "UV" else before[key] == after[key] for key in before)
    for r in rounds:      # the first listed pair that fits the budget is the one merged
        fits = [t[:2] for t in r["trials"] if t[4] is not None]
        assert r["chosen"] == (fits[0] if fits else None) and [t[:2] for t in r["trials"]] == r["pairs"]
    final = snapshot(model)
    X_pd = csr_matrix(model.X_pd) if getattr(model, "X_pd", None) is not None else csr_matrix(X.shape)
    log = flat_log(model.logs["refinements"]) if "refinements" in model.logs else {"columns": [], "rows": []}
    args = dict(args, beta=(None if args.get("beta", np.inf) == np.inf else float(args["beta"])))      # null: the default, inf
    return dict(args=args, seed=seed, hyper=before, rounds=rounds, ties=int(sum(decisions)), log=log, final=final,
                log_U=[dense_u8(csr_matrix(U)) for U in model.logs["U"]], log_V=[dense_u8(csr_matrix(V)) for V in model.logs["V"]],
                hyper_log_keys=sorted(hyper.logs.keys()), counts=counts_of(PyBMF, sp(X), X_pd))


def first_round_fpbs(hyper, X):
    """fpb of every pair of the Hyper model, dense: [(m, n, FP, fpb)] in (m, n) order."""
    X = X != 0
    T, I = sets_of(hyper)
    P = np.zeros_like(X)
    for t, i in zip(T, I):
        P[np.ix_(t, i)] = True
    out = []
    for a in range(len(T)):
        for b in range(a + 1, len(T)):
            Q = P.copy()
            Q[np.ix_(sorted(set(T[a] + T[b])), sorted(set(I[a] + I[b])))] = True
            fp = int((Q & ~X).sum())
            out.append((a, b, fp, float(np.float64(fp) / np.float64(int(X.sum())))))
    return out


def main():
    PyBMF = load_reference()
    Xa = planted(40, 30, 4, 0.3, 0.0, 2)
    Xb = planted(33, 65, 3, 0.3, 0.03, 9)
    Xz = np.zeros((20, 15), dtype=np.uint8)
    tr, va, te = deal(Xa, 3004)
    Ha, Hb, Hh, Hz = fit_hyper(Xa, 0.3), fit_hyper(Xb, 0.52), fit_hyper(tr, 0.2, va, te), fit_hyper(Xz, 0.5)
    fpbs = sorted({f for _, _, _, f in first_round_fpbs(Ha, Xa)})
    beta_c, beta_d, beta_f = (fpbs[0] + fpbs[1]) / 2, (fpbs[0] / 2 if fpbs[0] > 0 else -1.0), fpbs[1]
    cases = {}
    cases["a"] = run_plus(PyBMF, Ha, Xa, 7, target_k=1, samples=500)
    # case j comes right after case a: it needs the log that case a left in the Hyper model
    cases["j"] = run_plus(PyBMF, Ha, Xa, 17, target_k=4, samples=3)
    rows_a = len(cases["a"]["log"]["rows"])
    assert cases["j"]["log"]["rows"][:rows_a] == cases["a"]["log"]["rows"] and len(cases["j"]["log"]["rows"]) > rows_a
    cases["j"]["rows_before"] = rows_a
    for name, seed, args in (("b", 8, dict(target_k=1, samples=3)), ("c", 9, dict(target_k=1, samples=500, beta=beta_c)),
                             ("d", 10, dict(target_k=1, samples=500, beta=beta_d)), ("e", 11, dict(target_k=3, samples=500)),
                             ("f", 12, dict(target_k=4, samples=500, beta=beta_f))):
        Ha.logs.pop("refinements", None)      # each of these starts from a Hyper model whose log holds no refinements yet
        cases[name] = run_plus(PyBMF, Ha, Xa, seed, **args)
    cases["g"] = run_plus(PyBMF, Hb, Xb, 13, target_k=70, samples=20)
    cases["h"] = run_plus(PyBMF, Hh, tr, 14, X_val=va, X_test=te, target_k=28, samples=40)
    cases["i"] = run_plus(PyBMF, Hz, Xz, 15, target_k=1)
    data = {"a": (Xa,), "b": (Xa,), "c": (Xa,), "d": (Xa,), "e": (Xa,), "f": (Xa,), "g": (Xb,), "h": (tr, va, te), "i": (Xz,), "j": (Xa,)}

    c = cases
    assert c["a"]["final"]["k"] == 1 and len(c["a"]["rounds"]) == c["a"]["hyper"]["k"]
    assert c["b"]["rounds"][0]["k"] * (c["b"]["rounds"][0]["k"] - 1) // 2 > 3 == len(c["b"]["rounds"][0]["pairs"])
    refused = [[t[4] is None for t in r["trials"]] for r in c["c"]["rounds"]]
    assert any(r[0] and not all(r) for r in refused) and all(refused[-1]) and refused[-1] and c["c"]["final"]["k"] > 1
    assert len(c["d"]["rounds"]) == 1 and c["d"]["rounds"][0]["chosen"] is None and not c["d"]["log"]["rows"] and c["d"]["log_U"] == []
    assert c["e"]["final"]["k"] == 2
    first = c["f"]["rounds"][0]
    assert c["f"]["ties"] >= 1 and beta_f > 0 and [t[3] for t in first["trials"] if t[:2] == first["chosen"]] == [beta_f]
    assert c["g"]["hyper"]["k"] > 50 and len(c["g"]["rounds"][0]["pairs"]) == 20
    assert c["i"]["rounds"] == [dict(k=1, pairs=[], trials=[], chosen=None)] and c["i"]["hyper"]["T"] == []

    arrays, meta = {}, {"cases": {}}
    for name, run in cases.items():
        for key, A in zip(("X", "X_val", "X_test"), data[name]):
            arrays[f"{name}_{key}"] = A
        arrays[f"{name}_hyper_U"], arrays[f"{name}_hyper_V"] = run["hyper"].pop("U"), run["hyper"].pop("V")
        arrays[f"{name}_U"], arrays[f"{name}_V"] = run["final"].pop("U"), run["final"].pop("V")
        for r, (U, V) in enumerate(zip(run.pop("log_U"), run.pop("log_V"))):
            arrays[f"{name}_log_U{r}"], arrays[f"{name}_log_V{r}"] = U, V
        meta["cases"][name] = run
        print(name, "args:", run["args"], "k:", run["hyper"]["k"], "->", run["final"]["k"], "rounds:", len(run["rounds"]), "trials:",
              [len(r["trials"]) for r in run["rounds"]], "chosen:", [r["chosen"] for r in run["rounds"]], "ties:", run["ties"], "counts:",
              run["counts"])
    np.savez_compressed(os.path.join(HERE, "g31_hyperplus.npz"), **arrays)
    with open(os.path.join(HERE, "g31_hyperplus.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
