"""MessagePassing -- Boolean factorisation and noisy completion by max-sum message passing (Ravanbakhsh, Poczos, Greiner, *Boolean
Matrix Factorization and Noisy Completion via Message Passing*, ICML 2016, Algorithm 1).  Drop-in for
``PyBMF/models/MessagePassing.py``: its signature, its ``fit`` and its one ``evaluate(df_name='boolean')`` row.

The reference's class imports the algorithm from ``bmf_mp_ravanba``, which is not in its tree, so what is computed is DEFINED HERE
(DESIGN 9.4 has the full statement):

  * the update is Algorithm 1 in its max-sum form with the constants cx = logit(prior_u), cy = logit(prior_v),
    co = log(channel_pos / (1 - channel_neg)) where X = 1 and log((1 - channel_pos) / channel_neg) where X = 0; only this variant
    exists (the wrapper always passes ``min_sum=True``);
  * the start values: init_scale (2 u - 1) on the observed cells, u from a counter-based hash of (seed, side, i, j, f) (zero is a
    symmetric fixed point); ``seed=None`` takes one draw from the model's ``rng``;
  * the damping: hat <- (1 - lr) hat + lr new;
  * the stopping quantity d = the largest change of a marginal in an iteration, tested AFTER the update: the fit stops after the
    iteration in which d < tol, or after max_iter iterations;
  * the tie rule of M_f = max over f' != f of Gamma_f': taken from the two largest values, equal values counted twice;
  * a matrix ``W`` counts as a pattern: its non-zeros are the observed cells, its values are not used.

Every iteration is one streaming pass over the 2 k fp64 messages of every cell on the GPU (csrc/mp.hip through ``pybmf_amd/mp.py``).
``W='full'`` observes every cell, ``W='mask'`` the stored pattern of the csr ``X_train``, explicit zeros included -- matrix completion.
After the fit U = (marginal_U > 0), V = (marginal_V > 0) as 0 / 1 float arrays, X_pd their Boolean product; ``logs['updates']`` has
one row (iter, diff) per iteration; ``marginal_U``, ``marginal_V``, ``n_iter`` and ``converged`` describe the run.

Refused: values other than 0 / 1, k > 64, a sharded run, probabilities outside (0, 1).
"""
from __future__ import annotations

import numpy as np

from .. import _lib as L
from ..utils import ismat
from .ContinuousModel import ContinuousModel


class MessagePassing(ContinuousModel):
    def __init__(self, k, W='mask', prior_u=0.5, prior_v=0.5, channel_pos=0.99, channel_neg=0.99, tol=1e-4, max_iter=500, lr=0.2,
                 seed=None, init_scale=1e-2):
        self.check_params(k=k, W=W, prior_u=prior_u, prior_v=prior_v, channel_pos=channel_pos, channel_neg=channel_neg, tol=tol,
                          max_iter=max_iter, lr=lr, seed=seed, init_scale=init_scale)

    def check_params(self, **kwargs):
        super().check_params(**kwargs)
        if "seed" in kwargs:
            self._start_seed = kwargs["seed"]   # None: one draw from the rng at fit()
        assert (isinstance(self.W, str) and self.W in ['mask', 'full']) or ismat(self.W)
        if not 1 <= int(self.k) <= L.MAX_KP:
            raise NotImplementedError(f"k={self.k}: MessagePassing supports 1 <= k <= {L.MAX_KP}")
        for name in ("prior_u", "prior_v", "channel_pos", "channel_neg"):
            p = getattr(self, name)
            if not 0.0 < p < 1.0:
                raise ValueError(f"{name}={p}: a probability inside (0, 1) is needed (its log odds enter the messages)")
        if not 0.0 < self.lr <= 1.0:
            raise ValueError(f"lr={self.lr}: the damping needs 0 < lr <= 1")
        if int(self.max_iter) < 1:
            raise ValueError(f"max_iter={self.max_iter}: at least one iteration")

    def fit(self, X_train, X_val=None, X_test=None, **kwargs):
        try:
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        except ImportError:
            world = 1
        if world > 1:
            raise NotImplementedError("MessagePassing runs on one GPU: the messages of a cell are not sharded")
        super().fit(X_train, X_val, X_test, **kwargs)
        self._engine = self._make_engine()
        self._log_buffer = {}
        try:
            self._fit()
        finally:
            self._flush_logs()
            self._log_buffer = None
        self.finish(show_logs=self.show_logs, save_model=self.save_model, show_result=self.show_result)

    # ---- start-up ------------------------------------------------------------------------------------------------
    def init_W(self):
        """The observation pattern as a 0 / 1 csr matrix in `_mask_pattern`, None when every cell is observed.  'mask': the stored
        pattern of the csr training matrix, explicit zeros included; a matrix: its non-zeros."""
        self._obs, self._mask_is_pattern, self._mask_pattern = None, False, None
        from scipy.sparse import csr_matrix, issparse
        if isinstance(self.W, str):
            if self.W == 'full':
                return
            if not issparse(self.X_train):
                raise NotImplementedError("W='mask' needs a host matrix (ndarray / scipy sparse) to take the stored pattern from")
            pattern = self.X_train.copy()
        else:
            pattern = csr_matrix(self.W)
            if pattern.shape != (self.m, self.n):
                raise ValueError("W must have the shape of X_train")
            pattern.eliminate_zeros()
        if pattern.nnz == self.m * self.n:
            return   # every cell is observed
        pattern.data = np.ones(pattern.data.shape, dtype=np.uint8)
        self._mask_pattern = pattern

    def _make_engine(self):
        """The one place the engine is made (a test may substitute a NumPy stand-in)."""
        from ..engine import BitMatrix
        from ..mp import MessagePassingEngine
        if not self._boolean:
            raise NotImplementedError("this model's GPU path takes a Boolean (0/1) matrix")
        pattern = None if self._mask_pattern is None else BitMatrix(self._mask_pattern, self._bits.device)
        return MessagePassingEngine(self._bits, self.k, pattern=pattern, prior_u=self.prior_u, prior_v=self.prior_v,
                                    channel_pos=self.channel_pos, channel_neg=self.channel_neg, lr=self.lr, init_scale=self.init_scale)

    # ---- the loop ------------------------------------------------------------------------------------------------
    def _fit(self):
        seed = self._start_seed if getattr(self, "_start_seed", None) is not None else int(self.rng.randint(0, 2 ** 31 - 1))
        eng = self._engine
        eng.start(seed)
        from ..utils import header, record_many
        rows, self.converged = [], False
        while len(rows) < self.max_iter:
            d = eng.step()
            rows.append([len(rows) + 1, d])
            self.print_msg("iter: {}, diff: {:.3e}".format(len(rows), d))
            if d < self.tol:
                self.converged = True
                break
        self.n_iter = len(rows)
        record_many(self.logs, "updates", header(["iter", "diff"], levels=3), rows)
        self.marginal_U, self.marginal_V = eng.marginals()
        U, V = eng.decisions()
        self.U, self.V = U.astype(np.float64), V.astype(np.float64)
        self.X_pd = None   # the Boolean product, built on first access
        self.evaluate(df_name='boolean')

    def _thresholds(self):
        return 0.5, 0.5

    def _make_X_pd(self):
        from ..device_ops import boolean_product_csr
        return boolean_product_csr(self.U, self.V, u=0.5, v=0.5, device=self.device)
