"""The opening of the reference's thresholding notebooks: NMF (scikit-learn's coordinate-descent solver, NNDSVD start) gives real-valued
factors, and BinaryMFThreshold takes them as its 'custom' start and searches the pair of thresholds that binarises them best.

    python examples/nmf_init.py                 # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from pybmf_amd.generators import SyntheticMatrixGenerator
from pybmf_amd.models import BinaryMFThreshold, NMFSklearn

k = 5
X = SyntheticMatrixGenerator(m=300, n=200, k=k, density=(0.2, 0.2)).generate(seed=1000).add_noise(noise=(0.05, 0.01), seed=2000).X
quiet = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)

nmf = NMFSklearn(k=k, init_method='nndsvd', max_iter=1000, seed=2024)
nmf.fit(X, **quiet)
print("NMF: %d iterations, ||X - U V^T||_F = %.3f, U in [%.3f, %.3f], V in [%.3f, %.3f]"
      % (nmf.n_iter_, nmf.model.reconstruction_err_, nmf.U.min(), nmf.U.max(), nmf.V.min(), nmf.V.max()))
print("thresholds 0.5 / 0.5: %d ones in X_pd, %d in X" % (nmf.X_pd.nnz, int(X.sum())))

thr = BinaryMFThreshold(k=k, U=nmf.U, V=nmf.V, W='full', u=0.5, v=0.5, lamda=100, min_diff=1e-3, max_iter=30, init_method='custom', seed=2024)
thr.fit(X, **quiet)
print(thr.logs["updates"].to_string())
