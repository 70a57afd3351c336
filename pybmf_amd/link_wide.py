"""The link models -- PNLPF (sigmoid link on the product) and WNMF with the Kullback-Leibler loss -- at a rank 64 < k <= 128.

The factors are held as two blocks of 64 columns on the base of ``pybmf_amd/blocks.py``, but the two-block trick does not carry
over: the link is applied to the dot product over all 128 columns, so one tile-fused pass forms P over both blocks, sends it through
the link and contracts into both output blocks (csrc/link_wide.hip, ``bmf_link_pass_wide``).  What is per column still runs per
block through the kernels that exist: the slab sums of the denominators (``bmf_reduce_slabs``) or the column sums of the other
factor (``bmf_colsum_fill``), and the fp64 element-wise update (``bmf_mu_epilogue`` with ``den`` set).

``WideLinkMUEngine`` has the stepwise protocol of ``engine.LinkMUEngine`` (load_factors / prepare / update / scalars / factors);
a mask or a weight matrix runs on ``wide.WideMaskedMUEngine(link=...)``.  ``link_engine`` picks by k.  Python-driven, exact-fp32
MFMA, Boolean X, one GPU: a correctness row like the other wide ranks.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .blocks import BK, BlockEngine, check_wide, cover_count_wide, link_sums_wide
from .engine import BitMatrix, _stream


class WideLinkMUEngine(BlockEngine):
    def __init__(self, bits: BitMatrix, k: int, link: int, mode: int, lamda: float = 10.0, thr=(0.5, 0.5), obs_bits: BitMatrix = None):
        """``obs_bits`` (KL only): the observed cells of a W='mask' fit on a pattern that holds every non-zero of X -- the updates are
        those of the all-ones mask, only the objective is summed over the observed cells (see ``engine.LinkMUEngine``)."""
        check_wide(k, what="link engine")
        if link not in (L.LINK_SIGMOID, L.LINK_KL):
            raise ValueError("link must be LINK_SIGMOID or LINK_KL")
        if obs_bits is not None:
            assert link == L.LINK_KL and (obs_bits.m_pad, obs_bits.n_pad, obs_bits.ldx) == (bits.m_pad, bits.n_pad, bits.ldx)
        self.obs_bits = obs_bits
        self.X, self.link, self.mode, self.lamda, self.thr = bits, int(link), int(mode), float(lamda), thr
        mp, np_ = bits.m_pad, bits.n_pad
        self._alloc_blocks(bits.m, bits.n, mp, np_, bits.device, k)
        self.splitsU, self.splitsV = int(lib.bmf_link_splits(self.m, self.n)), int(lib.bmf_link_splits(self.n, self.m))
        self.numU, self.numV = self._blocks((self.splitsU, mp, BK), torch.float32), self._blocks((self.splitsV, np_, BK), torch.float32)
        sig = self.link == L.LINK_SIGMOID
        self.denU_slabs = self._blocks((self.splitsU, mp, BK), torch.float32) if sig else [None, None]
        self.denV_slabs = self._blocks((self.splitsV, np_, BK), torch.float32) if sig else [None, None]
        self.denU, self.denV = self._blocks((mp, BK), torch.float32), self._blocks((np_, BK), torch.float32)
        self.colsum = self._zeros((BK,), torch.float32)
        self.partU, self.partV = self._blocks((mp // 128, 2), torch.float64), self._blocks((np_ // 128, 2), torch.float64)
        self.sums = self._zeros((4,), torch.float64)
        self.sum_x, self.m_total = float(bits.sum_local), bits.m_total
        # bits / ld: X as the pass over this factor's rows reads it; cols, Fo, opad: the other factor
        self._extend_sides(U=dict(num=self.numU, splits=self.splitsU, den=self.denU, den_slabs=self.denU_slabs, part=self.partU, bits=bits.bits,
                                  ld=bits.ldx, cols=self.n, Fo=self.V, opad=np_),
                           V=dict(num=self.numV, splits=self.splitsV, den=self.denV, den_slabs=self.denV_slabs, part=self.partV, bits=bits.bits_t,
                                  ld=bits.ldxt, cols=self.m, Fo=self.U, opad=mp))

    def can_pipeline(self):
        return False

    def _epilogue(self, which, b, mode, reg):
        s = self._side(which)
        self._mu_epilogue(which, b, mode, reg, None if mode == L.MODE_PREPARE else s["num"], s["splits"], s["den"])

    def update_side(self, which, reg):
        """One factor: the pass from the whole old factor (both blocks), the denominators per block, the fp64 update per block."""
        s, st = self._side(which), _stream()
        Fs, Fo, num, den_slabs, den = s["F"], s["Fo"], s["num"], s["den_slabs"], s["den"]
        stride = s["rows_pad"] * BK
        check(lib.bmf_link_pass_wide(ptr(s["bits"]), s["rows_pad"], s["ld"], s["rows"], s["cols"], ptr(Fs[0]), ptr(Fs[1]), ptr(Fo[0]), ptr(Fo[1]), s["opad"],
                                     self.k, self.link, self.lamda, ptr(num[0]), ptr(num[1]), ptr(den_slabs[0]), ptr(den_slabs[1]), stride, s["splits"], st),
              "bmf_link_pass_wide")
        for b in range(2):
            if self.link == L.LINK_SIGMOID:
                check(lib.bmf_reduce_slabs(ptr(den_slabs[b]), stride, s["splits"], stride, ptr(den[b]), None, st), "bmf_reduce_slabs")
            else:  # KL: the denominator is the column-sum vector of the other factor's block, the same for every row
                check(lib.bmf_colsum_fill(ptr(Fo[b]), s["cols"], BK, ptr(self.colsum), ptr(den[b]), s["rows_pad"], st), "bmf_colsum_fill")
        for b in range(2):
            self._epilogue(which, b, self.mode, reg)

    def prepare(self):
        with torch.cuda.device(self.device):
            for which in ("V", "U"):
                for b in range(2):
                    self._epilogue(which, b, L.MODE_PREPARE, 0.0)

    def update(self, reg):
        """V then U (Gauss-Seidel between the factors; both blocks of a factor from the same pass, i.e. from its old value)."""
        with torch.cuda.device(self.device):
            self.update_side("V", reg)
            self.update_side("U", reg)

    def scalars(self, reg):
        """(error, rec_error, reg_error, RMSE, MAE, (TP, FP, FN, TN)) of the current state; one synchronising read."""
        X = self.X
        with torch.cuda.device(self.device):
            self.sums.zero_()
            link_sums_wide(X, self.m, self.n, self.U, self.V, self.k, self.link, self.lamda, None if self.obs_bits is None else self.obs_bits.bits, self.sums)
            self.counts.zero_()
            cover_count_wide(X, self.ubits, self.vcolbits, self.counts)
            out = self._scal
            out[0:3] = self.sums[:3]
            out[3:5] = self.counts.double()   # exact: counts < 2^53
            out[5] = sum(p[:, 0].sum() for p in self.partU)
            out[6] = sum(p[:, 0].sum() for p in self.partV)
            h = out.cpu().numpy()
        cells = float(self.m_total) * float(self.n)
        counts = self._count_tuple(int(h[3]), int(h[4]))
        rmse, mae = float(np.sqrt(h[1] / cells)), float(h[0] / cells)
        if self.link == L.LINK_KL:
            return float(h[2]), float(h[2]), 0.0, rmse, mae, counts
        rec = 0.5 * float(h[1])
        rg = float(reg) * (0.5 * float(h[5]) + 0.5 * float(h[6]))
        return rec + rg, rec, rg, rmse, mae, counts


def check_wide_link(k: int, sharded: bool = False, boolean: bool = True, mfma: str = None):
    """What the link models do not take at a rank above 64, refused with the reason before anything is uploaded."""
    check_wide(k, sharded=sharded, boolean=boolean, mfma=mfma, what="link")


def link_engine(bits, k: int, link: int, mode: int, lamda: float = 10.0, obs=None, obs_bits=None, sharded: bool = False, boolean: bool = True,
                mfma: str = None, with_mae: bool = True, m_total=None):
    """The engine of the link models for rank `k` on Boolean data: at k <= 64 ``engine.LinkMUEngine`` (all-ones mask) or
    ``engine.MaskedMUEngine(link=...)`` (`obs`: a mask / weight matrix as cell lists), exactly as the classes built them before; at
    64 < k <= 128 ``WideLinkMUEngine`` or ``wide.WideMaskedMUEngine(link=...)``.  ``mfma``: None = the engine's default."""
    if k <= L.MAX_KP:
        from .engine import LinkMUEngine, MaskedMUEngine
        if obs is not None:
            return MaskedMUEngine(obs, k, mode, bits=bits, with_mae=with_mae, link=link, lamda=lamda, sharded=sharded, m_total=m_total)
        kw = {} if mfma is None else dict(mfma=mfma)
        return LinkMUEngine(bits, k, link, mode, lamda=lamda, obs_bits=obs_bits, sharded=sharded, **kw)
    check_wide(k, sharded=sharded, boolean=boolean, mfma=mfma, what="link")
    if obs is not None:
        from .wide import WideMaskedMUEngine
        return WideMaskedMUEngine(obs, k, mode, bits=bits, with_mae=with_mae, link=link, lamda=lamda)
    return WideLinkMUEngine(bits, k, link, mode, lamda=lamda, obs_bits=obs_bits)
