"""Asso on a planted Boolean matrix (300 x 200, 5 rectangles, 2 % flips): candidate basis rows from the column associations, every
candidate of a sweep scored against the current prediction by a fused popcount GEMM on the GPU.

    python examples/asso.py               # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import Asso

rng = np.random.RandomState(7)
U, V = rng.rand(300, 5) < 0.2, rng.rand(200, 5) < 0.2
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(300, 200) < 0.02)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

asso = Asso(tau=0.5, k=5, w_fp=0.5)
asso.fit(X, **quiet)
print(asso.logs["updates"].to_string())
print("factors:", asso.U.shape[1], " ones in X:", int(X.sum()), " ones in X_pd:", asso.X_pd.nnz)
