"""Panda (PaNDa / PaNDa+) on a planted Boolean matrix (300 x 200, 5 rectangles, 1 % flips): every factor is a dense core of the
residual, found by walking the items in order of their correlation with the growing transaction set, then extended by the items and
transactions that do not raise the description length  w_model (|U| + |V|) + w_fp FP + w_fn FN; the scans over the items and the
transactions are bit-set passes on the GPU.

    python examples/panda.py                 # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import Panda

rng = np.random.RandomState(7)
U, V = rng.rand(300, 5) < 0.2, rng.rand(200, 5) < 0.2
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(300, 200) < 0.01)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

panda = Panda(k=4, init_method="correlation")      # k requested factors yield k + 1, as in the reference
panda.fit(X, **quiet)
print(panda.logs["updates"].to_string())
print("factors:", panda.U.shape[1], " ones in X:", int(X.sum()), " ones in X_pd:", panda.X_pd.nnz, " description length:", panda.cost_now)
