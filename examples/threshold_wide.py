"""The reference's pipeline at a rank above 64: WNMF at k = 72 on a planted Boolean matrix (the two-block engines of pybmf_amd/wide.py),
then BinaryMFThreshold on its factors -- the pair of thresholds that binarises them best, searched on the 128-column objective kernels
(csrc/thresh_wide.hip), eight trial points of a line search per launch.

    python examples/threshold_wide.py           # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import BinaryMFThreshold, WNMF

k = 72
rs = np.random.RandomState(7)
A, B = rs.rand(400, 12) < 0.15, rs.rand(300, 12) < 0.15
X = ((A.astype(np.int32) @ B.astype(np.int32).T) > 0) ^ (rs.rand(400, 300) < 0.03)          # planted, 3 % of the cells flipped
X = X.astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

wnmf = WNMF(k=k, W='full', init_method='normal', max_iter=40, seed=2024)
wnmf.fit(X, **quiet)
print("WNMF at k = %d: U in [%.3f, %.3f], V in [%.3f, %.3f]" % (k, wnmf.U.min(), wnmf.U.max(), wnmf.V.min(), wnmf.V.max()))

thr = BinaryMFThreshold(k=k, U=wnmf.U, V=wnmf.V, W='full', u=0.5, v=0.5, lamda=100, min_diff=1e-3, max_iter=30)
thr.fit(X, **quiet)
print(thr.logs["updates"].to_string())
print("thresholds u = %.4f, v = %.4f; %d trial points per launch" % (thr.u, thr.v, thr._trace["max_pairs"]))
