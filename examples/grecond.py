"""GreConD on a planted Boolean matrix (300 x 200, 5 rectangles, 1 % flips): greedy concept search, every candidate column of a
sweep scored by bit-set kernels on the GPU; the factors are exact rectangles of ones, so Precision stays 1.

    python examples/grecond.py               # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import GreConD

rng = np.random.RandomState(7)
U, V = rng.rand(300, 5) < 0.2, rng.rand(200, 5) < 0.2
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(300, 200) < 0.01)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

gc = GreConD(k=None, tol=0.01)
gc.fit(X, **quiet)
print(gc.logs["updates"].tail(3).to_string())
print("factors:", gc.U.shape[1], " ones in X:", int(X.sum()), " ones in X_pd:", gc.X_pd.nnz)
