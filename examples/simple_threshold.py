"""The chain of the reference's BinaryMFThreshold tutorial on a generated matrix: NMFSklearn factors, SimpleThreshold's grid search
over the pair of thresholds (all 1600 pairs of a 40 x 40 grid in one pass over X, csrc/thresh_grid.hip), then BinaryMFThreshold's
line search started from the pair the grid found.

    python examples/simple_threshold.py           # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import BinaryMFThreshold, NMFSklearn
from pybmf_amd.models.SimpleThreshold import SimpleThreshold

k = 20
rs = np.random.RandomState(2024)
A, B = rs.rand(300, k) < 0.08, rs.rand(500, k) < 0.08
X = ((A.astype(np.int32) @ B.astype(np.int32).T) > 0) ^ (rs.rand(300, 500) < 0.02)          # planted, 2 % of the cells flipped
X = X.astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

nmf = NMFSklearn(k=k, init_method='nndsvd', max_iter=200, seed=2024)
nmf.fit(X, **quiet)

st = SimpleThreshold(U=nmf.U, V=nmf.V, by_metric='F1', columnwise=False, randomize=False, n_grid=40, seed=2024)
st.fit(X, **quiet)
log = st.logs["updates"]
print(log.iloc[[0, 125, 129, st.best_iter - 1]].to_string())
print("grid search: best of %d trials is iter %d, u = %.6f, v = %.6f, F1 = %.4f" % (len(log), st.best_iter, st.u, st.v, log[("train", 0, "F1")][st.best_iter - 1]))

thr = BinaryMFThreshold(k=k, U=nmf.U, V=nmf.V, W='full', u=st.u, v=st.v, lamda=100, min_diff=1e-3, max_iter=30)
thr.fit(X, **quiet)
print(thr.logs["updates"].to_string())
print("line search from there: u = %.6f, v = %.6f" % (thr.u, thr.v))
