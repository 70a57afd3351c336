"""Hyper, then HyperPlus, on the planted Boolean matrix of examples/hyper.py (40 x 30, 4 rectangles) with 2 % of its cells flipped: Hyper
covers the noisy matrix exactly with many small rectangles, HyperPlus merges pairs of them (beta, the false-positive budget, is left at inf) until
target_k - 1 remain (the reference's stop rule overshoots by one).  Every round scores all its sampled pairs in one launch and one
read.  With savings='reference' the first sampled pair that fits the budget is merged (the reference's savings are always inf);
savings='new_fp' is this build's own ranking: description length saved per false positive added.

    python examples/hyperplus.py             # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import Hyper, HyperPlus

rng = np.random.RandomState(2)
U, V = rng.rand(40, 4) < 0.3, rng.rand(30, 4) < 0.3
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(40, 30) < 0.02)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

hyper = Hyper(min_support=0.3)
hyper.fit(X, **quiet)
print("Hyper: factors:", hyper.k, " ones in X:", int(X.sum()), " ones in X_pd:", hyper.X_pd.nnz)

for savings in ("reference", "new_fp"):
    hyper.logs.pop("refinements", None)          # the log is shared with the Hyper model: a second HyperPlus would append to it
    np.random.seed(7)                            # the pairs come from NumPy's global generator
    plus = HyperPlus(model=hyper, target_k=5, samples=500, savings=savings)
    plus.fit(X, **quiet)
    log = plus.logs["refinements"]
    print(f"\nHyperPlus(target_k=5, savings='{savings}'): {len(log)} rounds, the last ten:")
    print(log.tail(10).to_string())
    print("factors:", plus.k, " ones in X_pd:", plus.X_pd.nnz, " host reads:", plus._engine.reads)
    for T, I in zip(plus.T, plus.I):
        print("  rows", T, "x columns", I)
