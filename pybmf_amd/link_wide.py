"""The link models -- PNLPF (sigmoid link on the product) and WNMF with the Kullback-Leibler loss -- at a rank 64 < k <= 128.

The factors are held as two blocks of 64 columns like everywhere in ``pybmf_amd/wide.py``, but the two-block trick does not carry
over: the link is applied to the dot product over all 128 columns, so one tile-fused pass forms P over both blocks, sends it through
the link and contracts into both output blocks (csrc/link_wide.hip, ``bmf_link_pass_wide``).  What is per column still runs per
block through the kernels that exist: the slab sums of the denominators (``bmf_reduce_slabs``) or the column sums of the other
factor (``bmf_colsum_fill``), and the fp64 element-wise update (``bmf_mu_epilogue`` with ``den`` set).

``WideLinkMUEngine`` has the stepwise protocol of ``engine.LinkMUEngine`` (load_factors / prepare / update / scalars / factors);
a mask or a weight matrix runs on ``wide.WideMaskedMUEngine(link=...)``.  ``link_engine`` picks by k.  Python-driven, exact-fp32
MFMA, Boolean X, one GPU: a correctness row like the other wide ranks.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .engine import BitMatrix, _stream
from .wide import BK, MAX_K_WIDE


class WideLinkMUEngine:
    def __init__(self, bits: BitMatrix, k: int, link: int, mode: int, lamda: float = 10.0, thr=(0.5, 0.5), obs_bits: BitMatrix = None):
        """``obs_bits`` (KL only): the observed cells of a W='mask' fit on a pattern that holds every non-zero of X -- the updates are
        those of the all-ones mask, only the objective is summed over the observed cells (see ``engine.LinkMUEngine``)."""
        if not (BK < k <= MAX_K_WIDE):
            raise NotImplementedError(f"k={k}: the two-block link engine takes {BK} < k <= {MAX_K_WIDE}")
        if link not in (L.LINK_SIGMOID, L.LINK_KL):
            raise ValueError("link must be LINK_SIGMOID or LINK_KL")
        if obs_bits is not None:
            assert link == L.LINK_KL and (obs_bits.m_pad, obs_bits.n_pad, obs_bits.ldx) == (bits.m_pad, bits.n_pad, bits.ldx)
        self.obs_bits = obs_bits
        self.X, self.k, self.link, self.mode, self.lamda, self.thr = bits, int(k), int(link), int(mode), float(lamda), thr
        self.nb, self.kp = 2, BK
        self.kb = [BK, self.k - BK]          # real columns of each block
        dev = self.device = bits.device
        self.m, self.n, self.m_pad, self.n_pad = bits.m, bits.n, bits.m_pad, bits.n_pad
        mp, np_ = self.m_pad, self.n_pad
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        blocks = lambda shape, dt: [z(shape, dt) for _ in range(2)]  # noqa: E731
        self.U64, self.V64 = blocks((mp, BK), torch.float64), blocks((np_, BK), torch.float64)
        self.U, self.V = blocks((mp, BK), torch.float32), blocks((np_, BK), torch.float32)
        self.splitsU, self.splitsV = int(lib.bmf_link_splits(self.m, self.n)), int(lib.bmf_link_splits(self.n, self.m))
        self.numU, self.numV = blocks((self.splitsU, mp, BK), torch.float32), blocks((self.splitsV, np_, BK), torch.float32)
        sig = self.link == L.LINK_SIGMOID
        self.denU_slabs = blocks((self.splitsU, mp, BK), torch.float32) if sig else [None, None]
        self.denV_slabs = blocks((self.splitsV, np_, BK), torch.float32) if sig else [None, None]
        self.denU, self.denV = blocks((mp, BK), torch.float32), blocks((np_, BK), torch.float32)
        self.colsum = z((BK,), torch.float32)
        self.partU, self.partV = blocks((mp // 128, 2), torch.float64), blocks((np_ // 128, 2), torch.float64)
        self.ubits, self.vbits = blocks((mp,), torch.int64), blocks((np_,), torch.int64)
        self.ucolbits, self.vcolbits = blocks((BK, mp // 32), torch.int32), blocks((BK, np_ // 32), torch.int32)
        self.sums = z((4,), torch.float64)
        self.counts = z((2,), torch.int64)
        self._scal = z((8,), torch.float64)
        self.sum_x, self.m_total = float(bits.sum_local), bits.m_total

    def load_factors(self, U0, V0):
        assert U0.shape == (self.m, self.k) and V0.shape == (self.n, self.k), (U0.shape, V0.shape)
        for F64, F, F0, rows in ((self.U64, self.U, U0, self.m), (self.V64, self.V, V0, self.n)):
            for b in range(2):
                F64[b].zero_()
                F64[b][:rows, : self.kb[b]] = torch.from_numpy(np.ascontiguousarray(F0[:, BK * b: BK * b + self.kb[b]], dtype=np.float64)).to(self.device)
                F[b].copy_(F64[b])

    def factors(self):
        U = torch.cat([self.U64[b][: self.m, : self.kb[b]] for b in range(2)], dim=1).cpu().numpy()
        V = torch.cat([self.V64[b][: self.n, : self.kb[b]] for b in range(2)], dim=1).cpu().numpy()
        return U, V

    def can_pipeline(self):
        return False

    def _epilogue(self, which, b, mode, reg):
        if which == "V":
            F64, F, rows_pad, rows, num, splits, den = self.V64, self.V, self.n_pad, self.n, self.numV, self.splitsV, self.denV
            rb, cb, part, thr = self.vbits, self.vcolbits, self.partV, self.thr[1]
        else:
            F64, F, rows_pad, rows, num, splits, den = self.U64, self.U, self.m_pad, self.m, self.numU, self.splitsU, self.denU
            rb, cb, part, thr = self.ubits, self.ucolbits, self.partU, self.thr[0]
        a = L.EpilogueArgs()
        a.F64, a.F, a.rows_pad, a.rows, a.k, a.kp = F64[b].data_ptr(), F[b].data_ptr(), rows_pad, rows, self.kb[b], BK
        a.num, a.slab_stride, a.splits = (0 if mode == L.MODE_PREPARE else num[b].data_ptr()), rows_pad * BK, splits
        a.G, a.den, a.reg, a.mode, a.thr, a.terms = 0, den[b].data_ptr(), float(reg), mode, float(thr), 0
        a.panel, a.ldp, a.rowbits, a.colbits, a.ldcb = 0, rows_pad, rb[b].data_ptr(), cb[b].data_ptr(), rows_pad // 32
        a.partials, a.stop, a.blockmax = part[b].data_ptr(), 0, 0
        check(lib.bmf_mu_epilogue(C.byref(a), _stream()), "bmf_mu_epilogue")

    def _side(self, which, reg):
        """One factor: the pass from the whole old factor (both blocks), the denominators per block, the fp64 update per block."""
        X, st = self.X, _stream()
        if which == "V":
            bits, rows_pad, ldx, rows, cols, Fs, Fo, opad = X.bits_t, self.n_pad, X.ldxt, self.n, self.m, self.V, self.U, self.m_pad
            num, den_slabs, den, splits = self.numV, self.denV_slabs, self.denV, self.splitsV
        else:
            bits, rows_pad, ldx, rows, cols, Fs, Fo, opad = X.bits, self.m_pad, X.ldx, self.m, self.n, self.U, self.V, self.n_pad
            num, den_slabs, den, splits = self.numU, self.denU_slabs, self.denU, self.splitsU
        stride = rows_pad * BK
        check(lib.bmf_link_pass_wide(ptr(bits), rows_pad, ldx, rows, cols, ptr(Fs[0]), ptr(Fs[1]), ptr(Fo[0]), ptr(Fo[1]), opad, self.k, self.link,
                                     self.lamda, ptr(num[0]), ptr(num[1]), ptr(den_slabs[0]), ptr(den_slabs[1]), stride, splits, st), "bmf_link_pass_wide")
        for b in range(2):
            if self.link == L.LINK_SIGMOID:
                check(lib.bmf_reduce_slabs(ptr(den_slabs[b]), stride, splits, stride, ptr(den[b]), None, st), "bmf_reduce_slabs")
            else:  # KL: the denominator is the column-sum vector of the other factor's block, the same for every row
                check(lib.bmf_colsum_fill(ptr(Fo[b]), cols, BK, ptr(self.colsum), ptr(den[b]), rows_pad, st), "bmf_colsum_fill")
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
            self._side("V", reg)
            self._side("U", reg)

    def scalars(self, reg):
        """(error, rec_error, reg_error, RMSE, MAE, (TP, FP, FN, TN)) of the current state; one synchronising read."""
        X = self.X
        with torch.cuda.device(self.device):
            st = _stream()
            self.sums.zero_()
            ob = ptr(self.obs_bits.bits) if self.obs_bits is not None else None
            check(lib.bmf_link_sums_wide(ptr(X.bits), self.m_pad, X.ldx, self.m, self.n, ptr(self.U[0]), ptr(self.U[1]), ptr(self.V[0]), ptr(self.V[1]),
                                         self.n_pad, self.k, self.link, self.lamda, ob, ptr(self.sums), st), "bmf_link_sums_wide")
            self.counts.zero_()
            check(lib.bmf_cover_count_wide(ptr(X.bits), X.m_pad, X.ldx, X.n_pad // 32, ptr(self.ubits[0]), ptr(self.ubits[1]), ptr(self.vcolbits[0]),
                                           ptr(self.vcolbits[1]), X.n_pad // 32, ptr(self.counts), st), "bmf_cover_count_wide")
            out = self._scal
            out[0:3] = self.sums[:3]
            out[3:5] = self.counts.double()   # exact: counts < 2^53
            out[5] = sum(p[:, 0].sum() for p in self.partU)
            out[6] = sum(p[:, 0].sum() for p in self.partV)
            h = out.cpu().numpy()
        cells = float(self.m_total) * float(self.n)
        tp, fp = int(h[3]), int(h[4])
        fn = int(self.sum_x) - tp
        counts = (tp, fp, fn, self.m_total * self.n - tp - fp - fn)
        rmse, mae = float(np.sqrt(h[1] / cells)), float(h[0] / cells)
        if self.link == L.LINK_KL:
            return float(h[2]), float(h[2]), 0.0, rmse, mae, counts
        rec = 0.5 * float(h[1])
        rg = float(reg) * (0.5 * float(h[5]) + 0.5 * float(h[6]))
        return rec + rg, rec, rg, rmse, mae, counts


def check_wide_link(k: int, sharded: bool = False, boolean: bool = True, mfma: str = None):
    """What the link models do not take at a rank above 64, refused with the reason before anything is uploaded."""
    if k > MAX_K_WIDE:
        raise NotImplementedError(f"k={k}: this build supports k <= {MAX_K_WIDE}")
    if sharded:
        raise NotImplementedError(f"k={k}: a rank above {L.MAX_KP} runs on one GPU (row sharding needs k <= {L.MAX_KP})")
    if not boolean:
        raise NotImplementedError(f"k={k}: the link models at a rank above {L.MAX_KP} take Boolean (0/1) data; real-valued data needs k <= {L.MAX_KP}")
    if mfma == "bf16":
        raise NotImplementedError(f"k={k}: the link passes at a rank above {L.MAX_KP} run on the exact-fp32 MFMA only (mfma='bf16' needs k <= {L.MAX_KP})")


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
    check_wide_link(k, sharded=sharded, boolean=boolean, mfma=mfma)
    if obs is not None:
        from .wide import WideMaskedMUEngine
        return WideMaskedMUEngine(obs, k, mode, bits=bits, with_mae=with_mae, link=link, lamda=lamda)
    return WideLinkMUEngine(bits, k, link, mode, lamda=lamda, obs_bits=obs_bits)
