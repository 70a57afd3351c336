"""MEBF on a planted Boolean matrix (300 x 200, 5 rectangles, 1 % flips): every factor grows from the median column or row of the
residual, whichever rectangle lowers the weighted error more; scores, the median, the growth and the candidates' confusion counts
are bit-set passes on the GPU.

    python examples/mebf.py                  # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import MEBF

rng = np.random.RandomState(7)
U, V = rng.rand(300, 5) < 0.2, rng.rand(200, 5) < 0.2
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(300, 200) < 0.01)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

mebf = MEBF(k=8, t=0.7)
mebf.fit(X, **quiet)
print(mebf.logs["updates"].tail(3).to_string())
print("factors:", mebf.U.shape[1], " ones in X:", int(X.sum()), " ones in X_pd:", mebf.X_pd.nnz, " cost:", mebf.cost)
