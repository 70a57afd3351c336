"""MessagePassing on a noisy planted matrix (300 x 200, k = 5, 3 % of the cells flipped): fitted on every cell (W='full'), then with 30 %
of the cells hidden (W='mask': the stored pattern of the csr matrix, zeros included) -- matrix completion.  The logged scores of the
second fit set the whole prediction against the stored cells of each set (task='reconstruction'), so their precision is low by
construction; the printed count compares the hidden cells with the clean matrix.

    python examples/message_passing.py       # needs an MI355X (gfx950) and the built library (see README)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
from scipy.sparse import csr_matrix

from pybmf_amd.models import MessagePassing

rs = np.random.RandomState(4)
m, n, k = 300, 200, 5
U, V = rs.rand(m, k) < 0.25, rs.rand(n, k) < 0.25
clean = (U.astype(int) @ V.astype(int).T) > 0
X = clean ^ (rs.rand(m, n) < 0.03)
quiet = dict(show_logs=False, show_result=False, save_model=False)
params = dict(k=k, prior_u=0.4, prior_v=0.4, channel_pos=0.97, channel_neg=0.97, seed=0)


def stored(cells):
    """The cells of `cells` as a csr matrix that stores their values, zeros included."""
    rows, cols = np.nonzero(cells)
    return csr_matrix((X[rows, cols].astype(np.float64), (rows, cols)), shape=X.shape)


full = MessagePassing(W="full", **params)
full.fit(csr_matrix(X.astype(np.float64)), task="reconstruction", **quiet)
print(full.logs["boolean"].to_string())
print("W='full':", full.n_iter, "iterations, converged:", full.converged,
      " cells that differ from the clean matrix:", int((np.asarray(full.X_pd.todense() != 0) ^ clean).sum()), "of", m * n)

shown = rs.rand(m, n) < 0.7
mask = MessagePassing(W="mask", **params)
mask.fit(stored(shown), X_test=stored(~shown), task="reconstruction", **quiet)
print(mask.logs["boolean"].to_string())
pd = np.asarray(mask.X_pd.todense() != 0)
print("W='mask':", mask.n_iter, "iterations, converged:", mask.converged,
      " hidden cells that differ from the clean matrix:", int(((pd ^ clean) & ~shown).sum()), "of", int((~shown).sum()))
