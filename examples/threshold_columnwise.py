"""The end of the reference's FastStep tutorial (examples/ex05_3_FastStep.ipynb) on a generated matrix whose factor columns have
different scales: SimpleThreshold's randomised per-column search, then BinaryMFThresholdExColumnwise's line search over the 2k
thresholds, started from the tuples ``us``, ``vs`` the search found (csrc/thresh_cols.hip evaluates a whole Armijo chain per call).
A pair of scalar thresholds cannot binarise such factors; one threshold per column can.

    python examples/threshold_columnwise.py           # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models.BinaryMFThresholdExColumnwise import BinaryMFThresholdExColumnwise
from pybmf_amd.models.SimpleThreshold import SimpleThreshold

k = 20
rs = np.random.RandomState(2024)
A, B = rs.rand(300, k) < 0.08, rs.rand(500, k) < 0.08
X = ((A.astype(np.int32) @ B.astype(np.int32).T) > 0) ^ (rs.rand(300, 500) < 0.02)          # planted, 2 % of the cells flipped
X = X.astype(np.uint8)
su, sv = rs.uniform(0.5, 3.0, size=k), rs.uniform(0.5, 3.0, size=k)                          # every column on its own scale
U = (0.7 * A + 0.3 * rs.rand(300, k)) * su
V = (0.7 * B + 0.3 * rs.rand(500, k)) * sv
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

st = SimpleThreshold(U=U, V=V, by_metric='F1', columnwise=True, randomize=True, n_trials=1000, seed=2024)
st.fit(X, **quiet)
f1 = st.logs["updates"][("train", 0, "F1")][st.best_iter - 1]
print("randomised columnwise search: best of %d trials is iter %d, F1 = %.4f" % (len(st.logs["updates"]), st.best_iter, f1))

thr = BinaryMFThresholdExColumnwise(k=k, U=U, V=V, W='full', us=st.us, vs=st.vs, lamda=10, max_iter=100)
thr.fit(X, verbose=False, **quiet)
log = thr.logs["updates"]
print(log.to_string())
print("line search over the %d thresholds, %d iterations: F %.3f -> %.3f, F1 %.4f -> %.4f" % (
    2 * k, thr.n_iter, log[("", "", "F")].iloc[0], log[("", "", "F")].iloc[-1], log[("train", 0, "F1")].iloc[0], log[("train", 0, "F1")].iloc[-1]))
print("us =", np.round(thr.us, 3))
print("vs =", np.round(thr.vs, 3))
