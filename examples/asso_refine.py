"""Asso, then its two refiners, on a planted Boolean matrix (300 x 200, 5 rectangles, 4 % flips): AssoIter re-decides one column of U
at a time against the other factors, AssoOpt every row of U over all 2^k subsets of the factors -- both on the GPU.

    python examples/asso_refine.py        # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import Asso, AssoIter, AssoOpt

rng = np.random.RandomState(7)
U, V = rng.rand(300, 5) < 0.2, rng.rand(200, 5) < 0.2
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(300, 200) < 0.04)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)


def errors(model):
    P = np.asarray(model.X_pd.todense()) != 0
    return int((P != (X != 0)).sum())


asso = Asso(tau=0.4, k=6, w_fp=0.5)
asso.fit(X, **quiet)
print("Asso:     wrong cells", errors(asso))

refined = AssoIter(model=asso, w_fp=0.5)
refined.fit(X, **quiet)
print("AssoIter: wrong cells", errors(refined), " cells of U changed:", (refined.U != asso.U).nnz)

best = AssoOpt(model=refined, w_fp=1, w_fn=1)      # with weights 1 / 1 the score of a row is minus its wrong cells, plus a constant
best.fit(X, **quiet)
print("AssoOpt:  wrong cells", errors(best), " cells of U changed:", (best.U != refined.U).nnz)
print(best.logs["refinements"].to_string())
