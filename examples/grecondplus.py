"""GreConD+ on a planted Boolean matrix (300 x 200, 5 rectangles, 3 % flips): each concept of GreConD is expanded row by row and column
by column on the GPU while the weighted coverage score improves, so a factor may cover a few zeros (Precision below 1) and far fewer
factors reach the same error than GreConD needs on noisy data.

    python examples/grecondplus.py           # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.models import GreConD, GreConDPlus

rng = np.random.RandomState(7)
U, V = rng.rand(300, 5) < 0.2, rng.rand(200, 5) < 0.2
X = ((U.astype(int) @ V.astype(int).T > 0) ^ (rng.rand(300, 200) < 0.03)).astype(np.uint8)
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

gp = GreConDPlus(k=8, w_fp=0.3)
gp.fit(X, **quiet)
print(gp.logs["updates"].tail(3).to_string())
print("GreConD+ factors:", gp.U.shape[1], " extension rows / columns:", int(gp.U_exp.sum()), "/", int(gp.V_exp.sum()),
      " expansion steps per factor:", gp.n_steps, " ones in X:", int(X.sum()), " ones in X_pd:", gp.X_pd.nnz)

gc = GreConD(k=8)
gc.fit(X, **quiet)
print("GreConD with 8 factors, last row:")
print(gc.logs["updates"].tail(1).to_string())
