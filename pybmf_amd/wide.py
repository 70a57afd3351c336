"""Multiplicative updates for a rank 64 < k <= 128 (the reference has no rank limit: PyBMF/models/BinaryMFPenalty.py:32).

Every kernel of the k <= 64 path is written for one 64-bit word of factor bits per row.  A wider factor is held here as two BLOCKS
of 64 columns, F = [F_0 | F_1] (the layout, its state and the shared launches: ``pybmf_amd/blocks.py``); what is per column runs per
block through the kernels that exist -- the bits GEMMs X V_b and X^T U_b on the int8 digit planes, the plane builder, the fp64
element-wise update (``bmf_mu_epilogue`` with a precomputed denominator) -- and what couples the blocks is in csrc/wide.hip: the
re-associated denominator den_b = sum_b' F_b' G[b'][b] (``bmf_fg_f32``), the cross blocks of the Gram matrices (``bmf_gram_cross``),
the cover count over all 128 factors (``bmf_cover_count_wide``) and the residual sums with the full product (``bmf_resid_sums_wide``).

Python-driven, the interface of ``engine.MaskedMUEngine`` (prepare / update / scalars, and the pipelined iterate / row): a
correctness row -- no BASELINE configuration has k > 64 -- not a tuned path.  Boolean X, one GPU.  ``WideMUEngine``: the all-ones
mask (re-associated dense path); ``WideMaskedMUEngine``: W = 'mask' / a weight matrix (contractions over the observed cells,
``bmf_masked_pass_wide``; with ``link=`` the link models under a mask, ``bmf_masked_link_pass_wide``).  The link models under the
all-ones mask are in ``pybmf_amd/link_wide.py``.  X_val / X_test are scored by ``engine.ObservedScorer`` / ``WholeScorer``, which take
the block lists.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .blocks import (BK, MAX_K_WIDE, BlockEngine, check_wide, cover_count_wide, join, link_sums_wide, masked_pass_wide,  # noqa: F401
                     resid_sums_wide, resid_workspace)
from .engine import BitMatrix, HostRows, _stream


class WideMUEngine(BlockEngine):
    def __init__(self, X: BitMatrix, k: int, mode: int = L.MODE_PENALTY, with_mae: bool = True, thr=(0.5, 0.5)):
        check_wide(k, what="mu engine")
        if mode not in (L.MODE_PENALTY, L.MODE_WNMF):
            raise ValueError("mode must be MODE_PENALTY or MODE_WNMF")
        self.X, self.mode, self.with_mae, self.thr = X, int(mode), bool(with_mae), thr
        self._alloc_blocks(X.m, X.n, X.m_pad, X.n_pad, X.device, k)
        self._alloc_derived(X)
        mp, np_ = X.m_pad, X.n_pad
        self.denU, self.denV = self._blocks((mp, BK), torch.float32), self._blocks((np_, BK), torch.float32)
        self.partU, self.partV = self._blocks((mp // 128, 2), torch.float64), self._blocks((np_ // 128, 2), torch.float64)
        self.GU64, self.GV64 = ([self._blocks((BK, BK), torch.float64) for _ in range(self.nb)] for _ in range(2))
        self.sums = self._zeros((2,), torch.float64)
        self._mae_ws = resid_workspace(X) if self.with_mae else None
        self.sum_x = float(X.sum_local)
        self._extend_sides(U=dict(den=self.denU, part=self.partU, G64=self.GU64), V=dict(den=self.denV, part=self.partV, G64=self.GV64))

    # ---- the pieces ---------------------------------------------------------------------------------------------------------
    def _denominators(self, which):
        """den_b = sum_a F_a G[a][b] with G the Gram matrix of the OTHER factor, for both blocks, from the factor as it stands (all of it
        before any block is updated: the reference updates every column from the old factor, BinaryMFPenalty.py:139-148)."""
        s = self._side(which)
        st = _stream()
        for b in range(self.nb):
            for a in range(self.nb):
                check(lib.bmf_fg_f32(ptr(s["F"][a]), s["rows_pad"], ptr(s["Go"][a][b]), BK, ptr(s["den"][b]), int(a > 0), st), "bmf_fg_f32")

    def _epilogue(self, which, b, mode, reg, with_num=True):
        s = self._side(which)
        self._mu_epilogue(which, b, mode, reg, s["num"] if with_num else None, s["splits"], s["den"])

    def _refresh(self, which):
        """Everything derived from a factor after it changed: digit planes of both blocks, the four blocks of its Gram matrix, and the
        big contraction that uses it (X V_b for V, X^T U_b for U)."""
        s, st = self._side(which), _stream()
        self._planes(s, st)
        for a in range(self.nb):
            for b in range(a, self.nb):
                self._gram_pair(s, a, b, s["G64"][a][b], s["G64"][b][a], st)
        for b in range(self.nb):
            self._bits_gemm(s, s["panel"][b], s["scale"][b], s["xf"][b], st)

    # ---- the loop body ------------------------------------------------------------------------------------------------------
    def prepare(self):
        """Iteration-0 bookkeeping (BinaryMFPenalty.py:68-75): shadows, bits and regulariser sums of the initial factors, <U0, X V0>,
        both Gram matrices and X^T U0 for the first V update."""
        with torch.cuda.device(self.device):
            for b in range(self.nb):
                self._epilogue("V", b, L.MODE_PREPARE, 0.0, with_num=False)
            self._refresh("V")
            for b in range(self.nb):
                self._epilogue("U", b, L.MODE_PREPARE, 0.0)
            self._refresh("U")

    def update(self, reg):
        """V then U (Gauss-Seidel between the factors, every column of a factor from its old value), regulariser `reg`."""
        with torch.cuda.device(self.device):
            for which in ("V", "U"):
                self._denominators(which)
                for b in range(self.nb):
                    self._epilogue(which, b, self.mode, reg)
                self._refresh(which)

    # ---- the loop without a host round trip per iteration (round 5): iteration t + 1 is enqueued before the scalars of t are read ----
    def can_pipeline(self):
        return True

    def iterate(self, it: int, reg: float, update: bool = True):
        """Enqueue iteration `it`: keep the current iterate, update (unless update = False: log row 0), gather the scalars into a pinned
        host row with an asynchronous copy + event.  ``row(it, reg)`` waits for that row only (the protocol of MaskedMUEngine /
        LinkMUEngine, driven by ContinuousModel.mu_loop)."""
        with torch.cuda.device(self.device):
            if getattr(self, "_ring", None) is None:
                self._ring = HostRows()
                self._Up = [torch.empty_like(t) for t in self.U64]
                self._Vp = [torch.empty_like(t) for t in self.V64]
            if update:
                for b in range(self.nb):
                    self._Up[b].copy_(self.U64[b], non_blocking=True)
                    self._Vp[b].copy_(self.V64[b], non_blocking=True)
                self.update(reg)
            self._gather_scalars()
            self._ring.slot(it).copy_(self._scal, non_blocking=True)
            self._ring.mark(it)

    def row(self, it: int, reg: float):
        return self._decode(self._ring.wait(it), reg)

    def previous_factors(self):
        """The iterate before the last enqueued update."""
        return join(self._Up, self.m, self.k), join(self._Vp, self.n, self.k)

    def scalars(self, reg):
        """(error, rec_error, reg_error, RMSE, MAE, (TP, FP, FN, TN)) of the current state; one synchronising read.  rec_error in
        the trace form 1/2 (sum X - 2 <U, X V> + <U^T U, V^T V>) like the k <= 64 loop (api.hip::finalize_body)."""
        with torch.cuda.device(self.device):
            self._gather_scalars()
            h = self._scal.cpu().numpy()
        return self._decode(h, reg)

    def _gather_scalars(self):
        """The eight scalars of the current state into self._scal (device), nothing read back."""
        out = self._scal
        out.zero_()
        out[0] = sum(p[:, 1].sum() for p in self.partU)                      # <U, X V>
        out[1] = sum((self.GU64[a][b] * self.GV64[a][b]).sum() for a in range(self.nb) for b in range(self.nb))
        out[2] = sum(p[:, 0].sum() for p in self.partU)
        out[3] = sum(p[:, 0].sum() for p in self.partV)
        self.counts.zero_()
        cover_count_wide(self.X, self.ubits, self.vcolbits, self.counts)
        out[4:6] = self.counts.double()
        if self.with_mae:
            self._resid_sums()
            out[6] = self.sums[0]

    def _resid_sums(self):
        if self._mae_ws is None:
            self._mae_ws = resid_workspace(self.X)
        self.sums.zero_()
        resid_sums_wide(self.X, self._tiled[1], self.U, self.V, self._mae_ws, self.sums)

    def _decode(self, h, reg):
        cells = float(self.m) * float(self.n)
        rec = 0.5 * (self.sum_x - 2.0 * float(h[0]) + float(h[1]))
        rg = float(reg) * (0.5 * float(h[2]) + 0.5 * float(h[3])) if self.mode == L.MODE_PENALTY else 0.0
        rmse = float(np.sqrt(max(2.0 * rec, 0.0) / cells))
        mae = float(h[6]) / cells if self.with_mae else float("nan")
        return rec + rg, rec, rg, rmse, mae, self._count_tuple(int(h[4]), int(h[5]))

    def residual_sums(self):
        """(sum |X - U V^T|, sum (X - U V^T)^2) of the current factors by the direct pass (bmf_resid_sums_wide)."""
        with torch.cuda.device(self.device):
            self._resid_sums()
            s = self.sums.cpu().numpy()
        return float(s[0]), float(s[1])


class WideMaskedMUEngine(BlockEngine):
    """The masked updates (W = 'mask' or a weight matrix: PyBMF/models/BinaryMFPenalty.py:139-142,154-157, WNMF.py:98-106) for a
    rank 64 < k <= 128: ``engine.MaskedMUEngine`` with every factor as two 64-column blocks.  The pass over the observed cells takes
    the dot product over both blocks and leaves numerators / denominators per block (``bmf_masked_pass_wide``); the fp64 element-wise
    update runs per block (the denominators already carry the coupling).  Whole-matrix scores of a Boolean X (task =
    'reconstruction') from ``bmf_resid_sums_wide`` and ``bmf_cover_count_wide``.  Stepped from Python, one read-back per iteration;
    one GPU.  ``link`` = L.LINK_SIGMOID (PNLPF) or L.LINK_KL (WNMF, Kullback-Leibler loss): the dot product over both blocks goes through
    the link inside the pass (``bmf_masked_link_pass_wide``) and the whole-matrix scores are taken against the link prediction
    (``bmf_link_sums_wide``); under KL the denominator is the column-sum vector of each block of the other factor, as
    ``engine.MaskedMUEngine`` makes it."""

    def __init__(self, obs, k: int, mode: int, bits: BitMatrix = None, with_mae: bool = True, thr=(0.5, 0.5), link: int = 0, lamda: float = 10.0):
        check_wide(k, what="mu engine")
        if mode not in (L.MODE_PENALTY, L.MODE_WNMF):
            raise ValueError("mode must be MODE_PENALTY or MODE_WNMF")
        if link not in (0, L.LINK_SIGMOID, L.LINK_KL) or (link and bits is None):
            raise NotImplementedError("the two-block masked engine takes link = 0, LINK_SIGMOID or LINK_KL; a link needs the Boolean (0/1) X")
        from .engine import round_up
        self.obs, self.mode, self.bits, self.with_mae, self.thr = obs, int(mode), bits, bool(with_mae), thr
        self.link, self.lamda = int(link), float(lamda)
        mp, np_ = round_up(max(obs.m, 1), L.ROW_PAD), round_up(obs.n, L.ROW_PAD)
        self._alloc_blocks(obs.m, obs.n, mp, np_, obs.device, k)
        if bits is not None:
            assert (bits.m_pad, bits.n_pad) == (mp, np_)
        self.sum_x = float(bits.sum_local) if bits is not None else None
        self.numU, self.denU = self._blocks((mp, BK), torch.float32), self._blocks((mp, BK), torch.float32)
        self.numV, self.denV = self._blocks((np_, BK), torch.float32), self._blocks((np_, BK), torch.float32)
        self.partU, self.partV = self._blocks((mp // 128, 2), torch.float64), self._blocks((np_ // 128, 2), torch.float64)
        self.sums, self.sums2 = self._zeros((4,), torch.float64), self._zeros((4,), torch.float64)
        self._mae_ws = None
        self._tiled_t = None
        self._extend_sides(U=dict(num=self.numU, den=self.denU, part=self.partU), V=dict(num=self.numV, den=self.denV, part=self.partV))

    def can_pipeline(self):
        return False

    def _pass(self, ls, rows, Fself, Fother, num, den, sums):
        if sums is not None:
            sums.zero_()
        masked_pass_wide(ls, rows, Fself, Fother, num, den, sums, self.link, self.lamda)
        if self.link == L.LINK_KL:   # denominator O F_other: the column sums of the other factor (fp64 master), the same for every row
            F64 = self.V64 if Fother is self.V else self.U64
            for b in range(2):
                den[b].copy_(F64[b].sum(0).float().unsqueeze(0).expand_as(den[b]))

    def _epilogue(self, which, b, mode, reg):
        s = self._side(which)
        self._mu_epilogue(which, b, mode, reg, None if mode == L.MODE_PREPARE else s["num"], 1, s["den"])

    def prepare(self):
        """Shadows, bits and regulariser partials of the initial factors; numerators of the first V update + rec_error."""
        with torch.cuda.device(self.device):
            for which in ("V", "U"):
                for b in range(2):
                    self._epilogue(which, b, L.MODE_PREPARE, 0.0)
            self._pass(self.obs.csc, self.n, self.V, self.U, self.numV, self.denV, self.sums)

    def update(self, reg):
        """V then U (Gauss-Seidel between the factors; both blocks of a factor from the same pass, i.e. from its old value), then the
        pass that prepares the next V update and measures rec_error of the new state."""
        with torch.cuda.device(self.device):
            for b in range(2):
                self._epilogue("V", b, self.mode, reg)
            self._pass(self.obs.csr, self.m, self.U, self.V, self.numU, self.denU, None)
            for b in range(2):
                self._epilogue("U", b, self.mode, reg)
            self._pass(self.obs.csc, self.n, self.V, self.U, self.numV, self.denV, self.sums)

    def scalars(self, reg):
        """(error, rec_error, reg_error, RMSE, MAE, (TP, FP, FN, TN) or None): rec_error over the observed cells (0.5 sum W o (X - U V^T)^2),
        RMSE / MAE / counts over the whole matrix (task='reconstruction') when the Boolean matrix was given."""
        cells = float(self.m) * float(self.n)
        with torch.cuda.device(self.device):
            out = self._scal
            out.zero_()
            out[0] = self.sums[0]
            out[1] = sum(p[:, 0].sum() for p in self.partU)
            out[2] = sum(p[:, 0].sum() for p in self.partV)
            if self.bits is not None:
                B = self.bits
                if self._mae_ws is None:
                    self._mae_ws = resid_workspace(B)
                    self._tiled_t = B.tiled()[1]
                self.sums2.zero_()
                if self.link:   # whole-matrix RMSE / MAE against the link prediction (PNLPF.get_prediction, PNLPF.py:50-58)
                    link_sums_wide(B, self.m, self.n, self.U, self.V, self.k, self.link, self.lamda, None, self.sums2)
                else:
                    resid_sums_wide(B, self._tiled_t, self.U, self.V, self._mae_ws, self.sums2)
                self.counts.zero_()
                cover_count_wide(B, self.ubits, self.vcolbits, self.counts)
                out[3:5] = self.sums2[:2]
                out[5:7] = self.counts.double()
            h = out.cpu().numpy()
        rec = 0.5 * float(h[0])
        rg = float(reg) * (0.5 * float(h[1]) + 0.5 * float(h[2])) if self.mode == L.MODE_PENALTY else 0.0
        rmse = mae = float("nan")
        counts = None
        if self.bits is not None:
            rmse, mae = float(np.sqrt(h[4] / cells)), float(h[3] / cells)
            counts = self._count_tuple(int(h[5]), int(h[6]))
        return rec + rg, rec, rg, rmse, mae, counts
