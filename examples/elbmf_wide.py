"""ELBMF at a rank above 64, beside BinaryMFPenalty at the same rank: k = 100 on a planted Boolean matrix.  Both run on the two-block
engines (a factor as two blocks of 64 columns): the penalty model on pybmf_amd/wide.py, the proximal model on pybmf_amd/palm_wide.py --
its step over 128 factor columns and the norms of the 128 x 128 Gram are the kernels of csrc/palm_wide.hip.

    python examples/elbmf_wide.py           # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import ELBMF, BinaryMFPenalty

k = 100
rs = np.random.RandomState(7)
PU, PV = np.kron(np.eye(k), np.ones((3, 1))), np.kron(np.eye(k), np.ones((2, 1)))     # k disjoint 3 x 2 blocks of ones
X = ((PU @ PV.T) > 0) ^ (rs.rand(3 * k, 2 * k) < 0.01)                                 # 1 % of the cells flipped
X = X.astype(np.uint8)
U0, V0 = 0.7 * PU + 0.2 * rs.rand(*PU.shape), 0.7 * PV + 0.2 * rs.rand(*PV.shape)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

pen = BinaryMFPenalty(k=k, U=U0.copy(), V=V0.copy(), W='full', init_method='custom', reg=1.0, reg_growth=1.3, max_iter=20)
pen.fit(X, **quiet)
elb = ELBMF(k=k, U=U0.copy(), V=V0.copy(), W='full', init_method='custom', reg_l1=0.01, reg_l2=0.02, reg_growth=1.05, beta=0.0, max_iter=30)
elb.fit(X, **quiet)

print(elb.logs["updates"].tail(5).to_string())
for name, mdl in (("BinaryMFPenalty", pen), ("ELBMF", elb)):
    tp, fp, fn, tn = mdl._score("train", ["TP", "FP", "FN", "TN"])
    print("%-16s k = %d: TP %d  FP %d  FN %d  TN %d" % (name, k, tp, fp, fn, tn))
print("ELBMF engine:", type(elb._eng).__name__)
