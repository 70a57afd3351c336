"""Hyper on a planted Boolean matrix (40 x 30, 4 rectangles, noise free): an exact cover by overlapped hyperrectangles.  The candidates
are every column and the frequent itemsets at min_support; each factor is the cheapest (|T| + |I|) / (residual ones of T x I), found
by a lazy greedy whose `iter` column counts the head evaluations of the reference -- here each factor costs the GPU one evaluate
launch over all candidates and two reads.

    python examples/hyper.py                 # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import Hyper

rng = np.random.RandomState(2)
U, V = rng.rand(40, 4) < 0.3, rng.rand(30, 4) < 0.3
X = (U.astype(int) @ V.astype(int).T > 0).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

hyper = Hyper(min_support=0.3)
hyper.fit(X, **quiet)
print(hyper.logs["updates"].to_string())
print("factors:", hyper.k, " ones in X:", int(X.sum()), " ones in X_pd:", hyper.X_pd.nnz, " host reads:", hyper._engine.reads)
for T, I in zip(hyper.T, hyper.I):
    print("  rows", T, "x columns", I)
