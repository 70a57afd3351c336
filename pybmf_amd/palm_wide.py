"""The proximal (PALM / iPALM) models ELBMF and PRIMP at a rank 64 < k <= 128: ``palm.PalmEngine`` with every factor as two blocks
of 64 columns (the layout of ``wide.py``; the reference has no rank limit).

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
from .engine import BitMatrix, _stream, xf_slots_i8
from .wide import BK, MAX_K_WIDE

WN = 2 * BK   # side of the assembled Gram


class WidePalmEngine:
    def __init__(self, X: BitMatrix, k: int, variant: int, beta: float = 0.0, thr=(0.5, 0.5), obs=None):
        if k > MAX_K_WIDE:
            raise NotImplementedError(f"k={k}: this build supports k <= {MAX_K_WIDE}")
        if not (BK < k):
            raise NotImplementedError(f"k={k}: the two-block engine takes {BK} < k <= {MAX_K_WIDE}")
        self.X, self.k, self.variant, self.beta, self.thr = X, int(k), int(variant), float(beta), thr
        self.norm_kind = L.NORM_SPECTRAL if variant == L.PALM_ELBMF else L.NORM_FROBENIUS
        self.nb, self.kp = 2, BK   # (kp: columns of a block -- what the scorers are told; they recognise the block lists)
        self.kb = [BK, self.k - BK]
        dev = self.device = X.device
        mp, np_ = X.m_pad, X.n_pad
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        blocks = lambda rows, dt: [z((rows, BK), dt) for _ in range(2)]  # noqa: E731
        self.U64, self.V64, self.Up64, self.Vp64 = (blocks(r, torch.float64) for r in (mp, np_, mp, np_))
        self.U, self.V = blocks(mp, torch.float32), blocks(np_, torch.float32)
        self.Upanel, self.Vpanel = [z((3, BK, mp), torch.int8) for _ in range(2)], [z((3, BK, np_), torch.int8) for _ in range(2)]
        self.scaleU, self.scaleV = [z((2 * BK,), torch.float32) for _ in range(2)], [z((2 * BK,), torch.float32) for _ in range(2)]
        self._ws = z((max(mp, np_) // 128 * BK,), torch.float32)
        with torch.cuda.device(dev):
            self.splits_xv, self.splits_xtu = xf_slots_i8(mp, np_, BK), xf_slots_i8(np_, mp, BK)
            self._tiled = X.tiled()
        # X V_b and X^T U_b: the slabs of the GEMM on the digit planes of the factor, then as many again for the planes of what the
        # 24-bit planes left over (refresh); every consumer sums over all 2 * splits slabs
        self.Mslab = [z((2 * self.splits_xv, mp, BK), torch.float32) for _ in range(2)]
        self.Nslab = [z((2 * self.splits_xtu, np_, BK), torch.float32) for _ in range(2)]
        self._rest64, self._rest32 = {"U": z((mp, BK), torch.float64), "V": z((np_, BK), torch.float64)}, {"U": z((mp, BK), torch.float32), "V": z((np_, BK), torch.float32)}
        self._rpanel, self._rscale = {"U": z((3, BK, mp), torch.int8), "V": z((3, BK, np_), torch.int8)}, z((2 * BK,), torch.float32)
        self.gram_blocks = int(min(256, max(1, max(mp, np_) // 256)))
        self._gslabs = z((self.gram_blocks, BK, BK), torch.float32)
        self._g64 = z((BK, BK), torch.float64)
        self.GU, self.GV = ([[z((BK, BK), torch.float32) for _ in range(2)] for _ in range(2)] for _ in range(2))
        self.GU64, self.GV64 = z((WN, WN), torch.float64), z((WN, WN), torch.float64)    # the assembled 128 x 128 Grams
        self.normsU, self.normsV = z((2,), torch.float64), z((2,), torch.float64)
        # gap partials of both blocks side by side, and the <U, X V> partials of both blocks: bmf_palm_scalars sums each as one array
        self._partU, self._partV = z((2, mp // 128), torch.float64), z((2, np_ // 128), torch.float64)
        self.dot_blocks = 512
        self.dotpart = z((2, self.dot_blocks), torch.float64)
        self.ubits, self.vbits = [z((mp,), torch.int64) for _ in range(2)], [z((np_,), torch.int64) for _ in range(2)]
        self.ucolbits = [z((BK, mp // 32), torch.int32) for _ in range(2)]
        self.vcolbits = [z((BK, np_ // 32), torch.int32) for _ in range(2)]
        self.counts = z((2,), torch.int64)
        self._scal = z((8,), torch.float64)
        self.sum_x = float(X.sum_local)
        self.obs = obs
        if obs is not None:
            assert (obs.m, obs.n) == (X.m, X.n)
            self.numU, self.denU, self.numV, self.denV = (blocks(r, torch.float32) for r in (mp, mp, np_, np_))
            self.FeU, self.FeV = blocks(mp, torch.float32), blocks(np_, torch.float32)
            self._grad_ready = {"U": False, "V": False}

    def can_pipeline(self):
        return False

    def _side(self, which):
        X = self.X
        if which == "U":
            return dict(F64=self.U64, P64=self.Up64, F=self.U, rows_pad=X.m_pad, rows=X.m, panel=self.Upanel, scale=self.scaleU,
                        G=self.GU, G64=self.GU64, norms=self.normsU, part=self._partU, rb=self.ubits, cb=self.ucolbits, thr=self.thr[0],
                        num=self.Mslab, splits=self.splits_xv, Go=self.GV, norms_o=self.normsV)
        return dict(F64=self.V64, P64=self.Vp64, F=self.V, rows_pad=X.n_pad, rows=X.n, panel=self.Vpanel, scale=self.scaleV,
                    G=self.GV, G64=self.GV64, norms=self.normsV, part=self._partV, rb=self.vbits, cb=self.vcolbits, thr=self.thr[1],
                    num=self.Nslab, splits=self.splits_xtu, Go=self.GU, norms_o=self.normsU)

    # ---- factors ------------------------------------------------------------------------------------------------------------
    def load_factors(self, U0, V0, U_prev=None, V_prev=None):
        """Initial factors; ``U_prev / V_prev``: the iterate before them (inertial term), default = the same (ELBMF.py:111)."""
        X = self.X
        for F64, P64, F, F0, Fp, rows in ((self.U64, self.Up64, self.U, U0, U_prev, X.m), (self.V64, self.Vp64, self.V, V0, V_prev, X.n)):
            F0 = np.asarray(F0, dtype=np.float64)
            Fp = F0 if Fp is None else np.asarray(Fp, dtype=np.float64)
            assert F0.shape == Fp.shape == (rows, self.k), (F0.shape, Fp.shape)
            for b in range(2):
                cols = slice(BK * b, BK * b + self.kb[b])
                F64[b].zero_()
                P64[b].zero_()
                F64[b][:rows, : self.kb[b]] = torch.from_numpy(np.ascontiguousarray(F0[:, cols])).to(self.device)
                P64[b][:rows, : self.kb[b]] = torch.from_numpy(np.ascontiguousarray(Fp[:, cols])).to(self.device)
                F[b].copy_(F64[b])
        with torch.cuda.device(self.device):
            self.refresh("U")
            self.refresh("V")

    def _gather(self, F64):
        rows = self.X.m if F64 is self.U64 or F64 is self.Up64 else self.X.n
        return torch.cat([F64[b][:rows, : self.kb[b]] for b in range(2)], dim=1).cpu().numpy()

    def factors(self):
        return self._gather(self.U64), self._gather(self.V64)

    # ---- everything derived from a factor ---------------------------------------------------------------------------------------
    def refresh(self, which):
        """After factor `which` changed: the digit planes of both blocks, the four blocks of its Gram (fp32) and the assembled
        128 x 128 fp64 Gram, its two norms, and the big contraction that uses it (X V_b for V, X^T U_b for U)."""
        s, X = self._side(which), self.X
        kk = BK * BK
        with torch.cuda.device(self.device):
            st = _stream()
            for b in range(2):
                check(lib.bmf_make_panel_i8(ptr(s["F64"][b]), ptr(s["F"][b]), s["rows_pad"], BK, BK, 3, ptr(s["panel"][b]), s["rows_pad"], ptr(self._ws),
                                            ptr(s["scale"][b]), st), "bmf_make_panel_i8")
            for a in range(2):
                for b in range(a, 2):
                    check(lib.bmf_gram_cross(ptr(s["F"][a]), ptr(s["F"][b]), s["rows_pad"], ptr(self._gslabs), self.gram_blocks, st), "bmf_gram_cross")
                    check(lib.bmf_reduce_slabs(ptr(self._gslabs), kk, self.gram_blocks, kk, ptr(s["G"][a][b]), ptr(self._g64), st), "bmf_reduce_slabs")
                    s["G64"][BK * a: BK * a + BK, BK * b: BK * b + BK].copy_(self._g64)
                    if a != b:   # G[b][a] = G[a][b]^T
                        s["G"][b][a].copy_(s["G"][a][b].t())
                        s["G64"][BK * b: BK * b + BK, BK * a: BK * a + BK].copy_(self._g64.t())
            check(lib.bmf_sym_norms_wide(ptr(s["G64"]), ptr(s["norms"]), st), "bmf_sym_norms_wide")
            if which == "V":
                gemm = lambda panel, scale, out: check(lib.bmf_xf_bits_i8(ptr(self._tiled[0]), X.m_pad, X.ldx, X.n_pad // 32, ptr(panel), X.n_pad, 3,   # noqa: E731
                                                                          ptr(scale[BK:]), BK, ptr(out), X.m_pad * BK, self.splits_xv, 1, st), "bmf_xf_bits_i8")
                slabs, splits = self.Mslab, self.splits_xv
            else:
                gemm = lambda panel, scale, out: check(lib.bmf_xf_bits_i8(ptr(self._tiled[1]), X.n_pad, X.ldxt, X.m_pad // 32, ptr(panel), X.m_pad, 3,   # noqa: E731
                                                                          ptr(scale[BK:]), BK, ptr(out), X.n_pad * BK, self.splits_xtu, 1, st), "bmf_xf_bits_i8")
                slabs, splits = self.Nslab, self.splits_xtu
            r64, r32, rpanel = self._rest64[which], self._rest32[which], self._rpanel[which]
            for b in range(2):
                gemm(s["panel"][b], s["scale"][b], slabs[b])
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
                check(lib.bmf_make_panel_i8(ptr(r64), ptr(r32), s["rows_pad"], BK, BK, 3, ptr(rpanel), s["rows_pad"], ptr(self._ws), ptr(self._rscale), st),
                      "bmf_make_panel_i8")
                gemm(rpanel, self._rscale, slabs[b][splits:])

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
            if ls.get("part_wide") is None:
                ls["part_wide"] = [torch.zeros((max(ls["nseg"], 1), 2, BK), dtype=torch.float32, device=self.device) for _ in range(2)]
            p0, p1 = ls["part_wide"]
            check(lib.bmf_masked_pass_wide(ptr(ls["ptr"]), ptr(ls["idx"]), ptr(ls["val"]), ptr(ls["wgt"]), rows, ptr(ls["seg_row"]), ptr(ls["seg_beg"]),
                                           ls["nseg"], ptr(ls["row_seg_ptr"]), ptr(Fe[0]), ptr(Fe[1]), ptr(other[0]), ptr(other[1]), ptr(p0), ptr(p1),
                                           ptr(num[0]), ptr(num[1]), ptr(den[0]), ptr(den[1]), None, st), "bmf_masked_pass_wide")
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
                check(lib.bmf_cover_count_wide(ptr(X.bits), X.m_pad, X.ldx, X.n_pad // 32, ptr(self.ubits[0]), ptr(self.ubits[1]), ptr(self.vcolbits[0]),
                                               ptr(self.vcolbits[1]), X.n_pad // 32, ptr(self.counts), st), "bmf_cover_count_wide")
            # <U^T U, V^T V> over the four block pairs = the entry-wise product of the two assembled Grams, in fp64
            check(lib.bmf_palm_scalars(ptr(self.dotpart), 2 * self.dot_blocks, ptr(self.GU64), ptr(self.GV64), WN * WN, ptr(self._partU),
                                       self._partU.numel(), ptr(self._partV), self._partV.numel(), ptr(self.counts) if with_counts else None,
                                       ptr(self._scal), st), "bmf_palm_scalars")
            h = self._scal.cpu().numpy()
        err = self.sum_x - 2.0 * float(h[0]) + float(h[1])
        counts = None
        if with_counts:
            tp, fp = int(h[4]), int(h[5])
            fn = int(self.sum_x) - tp
            counts = (tp, fp, fn, X.m * X.n - tp - fp - fn)
        return err, float(h[2]), float(h[3]), counts


def palm_engine(X: BitMatrix, k: int, variant: int, beta: float = 0.0, obs=None, sharded: bool = False):
    """The engine of the proximal models for rank `k`: ``PalmEngine`` at k <= 64, ``WidePalmEngine`` at 64 < k <= 128."""
    from .palm import PalmEngine
    if k <= L.MAX_KP:
        return PalmEngine(X, k, variant, beta=beta, obs=obs)
    if k > MAX_K_WIDE:
        raise NotImplementedError(f"k={k}: this build supports k <= {MAX_K_WIDE}")
    if sharded:
        raise NotImplementedError(f"k={k}: a rank above {L.MAX_KP} runs on one GPU")
    return WidePalmEngine(X, k, variant, beta=beta, obs=obs)
