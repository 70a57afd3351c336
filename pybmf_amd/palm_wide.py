"""The proximal (PALM / iPALM) models ELBMF and PRIMP at a rank 64 < k <= 128: ``palm.PalmEngine`` with every factor as two blocks
of 64 columns (the layout and the shared launches of ``blocks.py``; the reference has no rank limit).

Per block through the kernels of the k <= 64 path: the digit planes, the bits GEMMs X V_b and X^T U_b (twice per block: the 24-bit
planes of the factor, then the planes of their remainder -- see ``refresh``), ``bmf_dot_slabs``.  What
couples the blocks: the four 64 x 64 blocks of a Gram (``bmf_gram_cross``), assembled into one 128 x 128 fp64 matrix for its norms
(``bmf_sym_norms_wide``: the step size never visits the host) and for <U^T U, V^T V>; the step itself over all 128 columns
(``bmf_palm_epilogue_wide``); the cover count over 128 factors (``bmf_cover_count_wide``).  With a mask / weight matrix the gradient
is den - num of ``bmf_masked_pass_wide`` at the extrapolated point and the step is element-wise: ``bmf_palm_epilogue`` per block with
``den`` set and the wide norms.

Stepped from Python with one synchronising read per iteration (``can_pipeline()`` is False): a correctness row like the rest of the
rank 65-128 paths, not a tuned one.  Boolean X, one GPU, int8 operands.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .blocks import BK, BlockEngine, check_wide, cover_count_wide, masked_pass_wide, split_into
from .engine import BitMatrix, _stream

WN = 2 * BK   # side of the assembled Gram


class WidePalmEngine(BlockEngine):
    def __init__(self, X: BitMatrix, k: int, variant: int, beta: float = 0.0, thr=(0.5, 0.5), obs=None):
        check_wide(k, what="palm engine")
        self.X, self.variant, self.beta, self.thr = X, int(variant), float(beta), thr
        self.norm_kind = L.NORM_SPECTRAL if variant == L.PALM_ELBMF else L.NORM_FROBENIUS
        mp, np_ = X.m_pad, X.n_pad
        self._alloc_blocks(X.m, X.n, mp, np_, X.device, k)
        # X V_b and X^T U_b: the slabs of the GEMM on the digit planes of the factor, then as many again for the planes of what the
        # 24-bit planes left over (refresh); every consumer sums over all 2 * splits slabs
        self._alloc_derived(X, slab_sets=2)
        z = self._zeros
        self.Up64, self.Vp64 = self._blocks((mp, BK), torch.float64), self._blocks((np_, BK), torch.float64)
        self._rest64, self._rest32 = {"U": z((mp, BK), torch.float64), "V": z((np_, BK), torch.float64)}, {"U": z((mp, BK), torch.float32), "V": z((np_, BK), torch.float32)}
        self._rpanel, self._rscale = {"U": z((3, BK, mp), torch.int8), "V": z((3, BK, np_), torch.int8)}, z((2 * BK,), torch.float32)
        self._g64 = z((BK, BK), torch.float64)
        self.GU64, self.GV64 = z((WN, WN), torch.float64), z((WN, WN), torch.float64)    # the assembled 128 x 128 Grams
        self.normsU, self.normsV = z((2,), torch.float64), z((2,), torch.float64)
        # gap partials of both blocks side by side, and the <U, X V> partials of both blocks: bmf_palm_scalars sums each as one array
        self._partU, self._partV = z((2, mp // 128), torch.float64), z((2, np_ // 128), torch.float64)
        self.dot_blocks = 512
        self.dotpart = z((2, self.dot_blocks), torch.float64)
        self.sum_x = float(X.sum_local)
        self._extend_sides(U=dict(P64=self.Up64, G64=self.GU64, norms=self.normsU, norms_o=self.normsV, part=self._partU),
                           V=dict(P64=self.Vp64, G64=self.GV64, norms=self.normsV, norms_o=self.normsU, part=self._partV))
        self.obs = obs
        if obs is not None:
            assert (obs.m, obs.n) == (X.m, X.n)
            self.numU, self.denU, self.numV, self.denV = (self._blocks((r, BK), torch.float32) for r in (mp, mp, np_, np_))
            self.FeU, self.FeV = self._blocks((mp, BK), torch.float32), self._blocks((np_, BK), torch.float32)
            self._grad_ready = {"U": False, "V": False}

    def can_pipeline(self):
        return False

    # ---- factors ------------------------------------------------------------------------------------------------------------
    def load_factors(self, U0, V0, U_prev=None, V_prev=None):
        """Initial factors; ``U_prev / V_prev``: the iterate before them (inertial term), default = the same (ELBMF.py:111)."""
        super().load_factors(U0, V0)
        for P64, F0, Fp in ((self.Up64, U0, U_prev), (self.Vp64, V0, V_prev)):
            Fp = np.asarray(F0 if Fp is None else Fp, dtype=np.float64)
            assert Fp.shape == np.shape(F0), (np.shape(F0), Fp.shape)
            split_into(P64, Fp)
        with torch.cuda.device(self.device):
            self.refresh("U")
            self.refresh("V")

    # ---- everything derived from a factor ---------------------------------------------------------------------------------------
    def refresh(self, which):
        """After factor `which` changed: the digit planes of both blocks, the four blocks of its Gram (fp32) and the assembled
        128 x 128 fp64 Gram, its two norms, and the big contraction that uses it (X V_b for V, X^T U_b for U)."""
        s = self._side(which)
        with torch.cuda.device(self.device):
            st = _stream()
            self._planes(s, st)
            for a in range(2):
                for b in range(a, 2):
                    self._gram_pair(s, a, b, s["G64"][BK * a: BK * a + BK, BK * b: BK * b + BK], s["G64"][BK * b: BK * b + BK, BK * a: BK * a + BK], st,
                                    stage=self._g64)
            check(lib.bmf_sym_norms_wide(ptr(s["G64"]), ptr(s["norms"]), st), "bmf_sym_norms_wide")
            slabs, splits = s["xf"], s["xf_splits"]
            r64, r32, rpanel = self._rest64[which], self._rest32[which], self._rpanel[which]
            for b in range(2):
                self._bits_gemm(s, s["panel"][b], s["scale"][b], slabs[b], st)
                # The planes hold rint(F 2^e) per column, 24 bits below the column's maximum: an entry of 2e-3 in a column that reaches 1 is
                # off by up to 6e-8, and X F inherits it.  The reference's prox has no dead zone at 0 -- an exact-zero entry goes to 0 or
                # to kai by the sign of an argument that is a difference of such sums, of size 1e-8 on near-Boolean factors -- so at this
                # rank the contraction is completed: what the planes left over, F - q / 2^e (exact in fp64), goes through the same
                # builder and the same GEMM with its own column scales, into the second half of the slabs (48 bits in all).
                sc = s["scale"][b][:BK].double()
                torch.mul(s["F64"][b], sc, out=r64)
                r64.round_().clamp_(-8355711.0, 8355711.0).div_(sc)
                torch.sub(s["F64"][b], r64, out=r64)
                r32.copy_(r64)
                self._panel(r64, r32, s["rows_pad"], rpanel, self._rscale, st)
                self._bits_gemm(s, rpanel, self._rscale, slabs[b][splits:], st)

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def masked_grad(self, which):
        """(W o X) G and (W o (Fe G^T)) G per block of factor `which` over the observed cells, Fe = its extrapolated point, G = the
        CURRENT other factor (ELBMF.py:188-190); see PalmEngine.masked_grad."""
        assert self.obs is not None
        s = self._side(which)
        ls, rows = (self.obs.csr, self.X.m) if which == "U" else (self.obs.csc, self.X.n)
        Fe, num, den, other = (self.FeU, self.numU, self.denU, self.V) if which == "U" else (self.FeV, self.numV, self.denV, self.U)
        with torch.cuda.device(self.device):
            st = _stream()
            for b in range(2):
                check(lib.bmf_palm_extrapolate(ptr(s["F64"][b]), ptr(s["P64"][b]), self.beta, s["rows_pad"] * BK, ptr(Fe[b]), st), "bmf_palm_extrapolate")
            masked_pass_wide(ls, rows, Fe, other, num, den, None)
        self._grad_ready[which] = True

    def step(self, which, l1: float, l2: float, gap_l1: float = 0.0, gap_l2: float = 0.0, advance_prev: bool = True):
        """One proximal step of factor `which` from the CURRENT contraction / Gram of the other factor."""
        s = self._side(which)
        if self.obs is not None:
            if not self._grad_ready[which]:
                self.masked_grad(which)
            num, den = (self.numU, self.denU) if which == "U" else (self.numV, self.denV)
            with torch.cuda.device(self.device):
                for b in range(2):   # element-wise per block: the masked pass has done the coupling
                    a = L.PalmArgs()
                    a.F64, a.Fprev64, a.F = s["F64"][b].data_ptr(), s["P64"][b].data_ptr(), s["F"][b].data_ptr()
                    a.rows_pad, a.rows, a.k, a.kp = s["rows_pad"], s["rows"], self.kb[b], BK
                    a.splits, a.num, a.den, a.slab_stride = 1, num[b].data_ptr(), den[b].data_ptr(), s["rows_pad"] * BK
                    a.G, a.norms, a.norm_kind, a.variant = None, s["norms_o"].data_ptr(), self.norm_kind, self.variant
                    a.beta, a.l1, a.l2, a.gap_l1, a.gap_l2 = self.beta, float(l1), float(l2), float(gap_l1), float(gap_l2)
                    a.advance_prev, a.thr = int(advance_prev), float(s["thr"])
                    a.rowbits, a.colbits, a.ldcb = s["rb"][b].data_ptr(), s["cb"][b].data_ptr(), s["rows_pad"] // 32
                    a.partials, a.blockmax, a.stop = s["part"][b].data_ptr(), None, None
                    check(lib.bmf_palm_epilogue(C.byref(a), _stream()), "bmf_palm_epilogue")
            self._grad_ready[which] = False
            return
        a = L.PalmWideArgs()
        a.struct_bytes = C.sizeof(L.PalmWideArgs)
        a.rows, a.k, a.splits, a.rows_pad, a.slab_stride = s["rows"], self.k, 2 * s["splits"], s["rows_pad"], s["rows_pad"] * BK
        for b in range(2):
            a.F64[b], a.Fprev64[b], a.F[b], a.num[b] = s["F64"][b].data_ptr(), s["P64"][b].data_ptr(), s["F"][b].data_ptr(), s["num"][b].data_ptr()
            a.rowbits[b], a.colbits[b], a.partials[b] = s["rb"][b].data_ptr(), s["cb"][b].data_ptr(), s["part"][b].data_ptr()
            for c in range(2):
                a.G[b][c] = s["Go"][b][c].data_ptr()
        a.norms, a.norm_kind, a.variant = s["norms_o"].data_ptr(), self.norm_kind, self.variant
        a.beta, a.l1, a.l2, a.gap_l1, a.gap_l2 = self.beta, float(l1), float(l2), float(gap_l1), float(gap_l2)
        a.advance_prev, a.thr, a.ldcb = int(advance_prev), float(s["thr"]), s["rows_pad"] // 32
        with torch.cuda.device(self.device):
            check(lib.bmf_palm_epilogue_wide(C.byref(a), _stream()), "bmf_palm_epilogue_wide")

    # ---- the scalars of an iteration ----------------------------------------------------------------------------------------------
    def scalars(self, with_counts=True):
        """(||X - U V^T||_F^2, U gap, V gap, (TP, FP, FN, TN) or None) of the current state; one synchronising read.  Needs
        Mslab = X V and both Grams of the current factors (i.e. both sides refreshed)."""
        X = self.X
        with torch.cuda.device(self.device):
            st = _stream()
            n = X.m_pad * BK
            for b in range(2):
                check(lib.bmf_dot_slabs(ptr(self.U64[b]), ptr(self.Mslab[b]), n, 2 * self.splits_xv, n, ptr(self.dotpart[b]), self.dot_blocks, st), "bmf_dot_slabs")
            if with_counts:   # (the counters are zero: the previous call reset them)
                cover_count_wide(X, self.ubits, self.vcolbits, self.counts)
            # <U^T U, V^T V> over the four block pairs = the entry-wise product of the two assembled Grams, in fp64
            check(lib.bmf_palm_scalars(ptr(self.dotpart), 2 * self.dot_blocks, ptr(self.GU64), ptr(self.GV64), WN * WN, ptr(self._partU),
                                       self._partU.numel(), ptr(self._partV), self._partV.numel(), ptr(self.counts) if with_counts else None,
                                       ptr(self._scal), st), "bmf_palm_scalars")
            h = self._scal.cpu().numpy()
        err = self.sum_x - 2.0 * float(h[0]) + float(h[1])
        counts = self._count_tuple(int(h[4]), int(h[5])) if with_counts else None
        return err, float(h[2]), float(h[3]), counts


def palm_engine(X: BitMatrix, k: int, variant: int, beta: float = 0.0, obs=None, sharded: bool = False):
    """The engine of the proximal models for rank `k`: ``PalmEngine`` at k <= 64, ``WidePalmEngine`` at 64 < k <= 128."""
    from .palm import PalmEngine
    if k <= L.MAX_KP:
        return PalmEngine(X, k, variant, beta=beta, obs=obs)
    check_wide(k, sharded=sharded, what="palm")
    return WidePalmEngine(X, k, variant, beta=beta, obs=obs)
