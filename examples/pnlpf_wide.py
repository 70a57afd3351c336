"""PNLPF at a rank above 64, beside BinaryMFPenalty at the same rank and WNMF with the Kullback-Leibler loss: k = 100 on a planted Boolean
matrix.  All three hold a factor as two blocks of 64 columns; the penalty model runs per block (pybmf_amd/wide.py), the two link models
cannot -- the link is applied to the dot product over all 128 columns -- and run on the passes of csrc/link_wide.hip
(pybmf_amd/link_wide.py).

    python examples/pnlpf_wide.py           # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import PNLPF, WNMF, BinaryMFPenalty

k = 100
rs = np.random.RandomState(7)
PU, PV = np.kron(np.eye(k), np.ones((3, 1))), np.kron(np.eye(k), np.ones((2, 1)))     # k disjoint 3 x 2 blocks of ones
X = ((PU @ PV.T) > 0) ^ (rs.rand(3 * k, 2 * k) < 0.01)                                 # 1 % of the cells flipped
X = X.astype(np.uint8)
U0, V0 = 0.7 * PU + 0.2 * rs.rand(*PU.shape), 0.7 * PV + 0.2 * rs.rand(*PV.shape)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

pen = BinaryMFPenalty(k=k, U=U0.copy(), V=V0.copy(), W='full', init_method='custom', reg=1.0, reg_growth=1.3, max_iter=20)
pen.fit(X, **quiet)
pnl = PNLPF(k=k, U=U0.copy(), V=V0.copy(), W='full', init_method='custom', reg=1.0, reg_growth=1.3, link_lamda=10, max_iter=20)
pnl.fit(X, **quiet)
kl = WNMF(k=k, U=U0.copy(), V=V0.copy(), W='full', beta_loss='kullback-leibler', init_method='custom', max_iter=20)
kl.fit(X, **quiet)

print(pnl.logs["updates"].tail(5).to_string())
for name, mdl in (("BinaryMFPenalty", pen), ("PNLPF", pnl)):
    tp, fp, fn, tn = mdl._score("train", ["TP", "FP", "FN", "TN"])
    print("%-16s k = %d: TP %d  FP %d  FN %d  TN %d" % (name, k, tp, fp, fn, tn))
print("WNMF-KL          k = %d: objective %.2f after %d iterations" % (k, float(kl.logs["updates"].values[-1][2]), kl.n_iter))
print("engines:", type(pnl._eng).__name__, "/", type(kl._eng).__name__)
