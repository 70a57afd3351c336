"""FastStep on the quick-start problem (1000 x 500 planted Boolean matrix, k = 8): projected Wolfe line search on the logistic
loss, one factor at a time; F, its gradient and the TP / FP counts of (U V^T > tau) are one GPU pass per call.

    python examples/faststep.py              # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybmf_amd.generators import SyntheticMatrixGenerator
from pybmf_amd.models import FastStep

gen = SyntheticMatrixGenerator(m=1000, n=500, k=8, density=[0.2, 0.2])
gen.generate(seed=1000)
gen.add_noise(noise=[0.05, 0.01], seed=2000)
X = gen.X
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

fs = FastStep(k=8, W="full", tau=20, max_round=3, max_iter=10, seed=2024)
fs.fit(X, **quiet)
print(fs.logs["updates"].tail(3).to_string())
print("steps:", len(fs.logs["updates"]), " ones in X_pd:", fs.X_pd.nnz)
