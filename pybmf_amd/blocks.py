"""What the rank 64 < k <= 128 engines share: a factor held as two BLOCKS of 64 columns, F = [F_0 | F_1], zero padded.

``BlockEngine`` is the base of ``wide.WideMUEngine`` / ``WideMaskedMUEngine``, ``link_wide.WideLinkMUEngine`` and
``palm_wide.WidePalmEngine``: the block state and its ``_side`` records, split / join of a host factor, the argument block of
``bmf_mu_epilogue``, and the chain of what is derived from a factor (digit planes, Gram block pairs, bits GEMMs).  The entry points
of the C library that take both blocks at once are wrapped once each, below the class, for the engines, the scorers of
``engine.py`` and the models.  ``check_wide`` words every refusal of a rank above 64.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .engine import _stream, xf_slots_i8

MAX_K_WIDE = 128
BK = 64   # columns of a block

_ONE_GPU = f"a rank above {L.MAX_KP} runs on one GPU"
_REAL = f"real-valued data needs k <= {L.MAX_KP}"
# what: (sharded, data that is not 0 / 1, mfma='bf16'), as each family words it
_REFUSALS = {
    "mu": (f"{_ONE_GPU}, on Boolean (0/1) data", f"{_ONE_GPU}, on Boolean (0/1) data", None),
    "link": (f"{_ONE_GPU} (row sharding needs k <= {L.MAX_KP})", f"the link models at a rank above {L.MAX_KP} take Boolean (0/1) data; {_REAL}",
             f"the link passes at a rank above {L.MAX_KP} run on the exact-fp32 MFMA only (mfma='bf16' needs k <= {L.MAX_KP})"),
    "palm": (_ONE_GPU, None, None),
    "threshold": (f"{_ONE_GPU} (a sharded run needs k <= {L.MAX_KP})", f"BinaryMFThreshold at a rank above {L.MAX_KP} takes Boolean (0/1) data; {_REAL}", None),
}
_ENGINES = {"mu engine": "the two-block engine", "link engine": "the two-block link engine", "palm engine": "the two-block engine"}


def check_wide(k: int, *, sharded: bool = False, boolean: bool = True, mfma: str = None, what: str = "mu"):
    """What a rank above 64 does not take, refused with the reason before anything is uploaded.  ``what``: the family whose wording
    is used ('mu', 'link', 'palm', 'threshold'); '<family> engine' is a two-block constructor, which takes no k <= 64 either."""
    if k > MAX_K_WIDE and what not in ("mu engine", "link engine"):   # (these two constructors word both ends of the range in one text)
        raise NotImplementedError(f"k={k}: this build supports k <= {MAX_K_WIDE}")
    if what in _ENGINES and not (BK < k <= MAX_K_WIDE):
        raise NotImplementedError(f"k={k}: {_ENGINES[what]} takes {BK} < k <= {MAX_K_WIDE}")
    if k <= BK:
        return
    texts = _REFUSALS[what.split()[0]]
    for refused, text in zip((sharded, not boolean, mfma == "bf16"), texts):
        if refused and text:   # (None: a family that has no such switch)
            raise NotImplementedError(f"k={k}: {text}")


# ---- a host factor <-> its two blocks ---------------------------------------------------------------------------------------------
def split_into(blocks, F):
    """The (rows, k) array `F` into the two (rows_pad, 64) tensors `blocks` (in their dtype): block b takes columns 64 b ..., every
    other row and column is zero."""
    rows, k = F.shape
    for b, t in enumerate(blocks):
        kb = min(BK, k - BK * b)
        t.zero_()
        t[:rows, :kb] = torch.from_numpy(np.ascontiguousarray(F[:, BK * b: BK * b + kb], dtype=np.float64 if t.dtype == torch.float64 else np.float32)).to(t.device)


def join(blocks, rows: int, k: int):
    """The (rows, k) host array of two blocks."""
    return torch.cat([t[:rows, : min(BK, k - BK * b)] for b, t in enumerate(blocks)], dim=1).cpu().numpy()


class BlockEngine:
    nb, kp = 2, BK   # (kp: columns of a block -- what the scorers are told; they recognise the block lists)

    def _zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def _blocks(self, shape, dtype):
        return [self._zeros(shape, dtype) for _ in range(self.nb)]

    def _alloc_blocks(self, m, n, m_pad, n_pad, device, k):
        """The state every engine keeps per block: fp64 masters and fp32 shadows of both factors, their thresholded bits by row and
        by column, the cover counters and the scalar row; and the ``_side`` record of each factor (``self.thr`` is set before)."""
        self.m, self.n, self.m_pad, self.n_pad, self.device, self.k = m, n, m_pad, n_pad, device, int(k)
        self.m_total = m
        self.kb = [BK, self.k - BK]          # real columns of each block
        self.U64, self.V64 = self._blocks((m_pad, BK), torch.float64), self._blocks((n_pad, BK), torch.float64)
        self.U, self.V = self._blocks((m_pad, BK), torch.float32), self._blocks((n_pad, BK), torch.float32)
        self.ubits, self.vbits = self._blocks((m_pad,), torch.int64), self._blocks((n_pad,), torch.int64)
        self.ucolbits, self.vcolbits = self._blocks((BK, m_pad // 32), torch.int32), self._blocks((BK, n_pad // 32), torch.int32)
        self.counts = self._zeros((2,), torch.int64)
        self._scal = self._zeros((8,), torch.float64)
        self._sides = {"U": dict(F64=self.U64, F=self.U, rows_pad=m_pad, rows=m, rb=self.ubits, cb=self.ucolbits, thr=self.thr[0]),
                       "V": dict(F64=self.V64, F=self.V, rows_pad=n_pad, rows=n, rb=self.vbits, cb=self.vcolbits, thr=self.thr[1])}

    def _side(self, which):
        """One factor's tensors by role (lists are per block); built once, extended by the engine with what it adds."""
        return self._sides[which]

    def _extend_sides(self, U, V):
        self._sides["U"].update(U)
        self._sides["V"].update(V)

    def _alloc_derived(self, X, slab_sets=1):
        """What the dense engines derive from a factor, per block: int8 digit planes and their scales, the slabs of the bits GEMM
        with it (``slab_sets`` times the stream-K slots), the fp32 blocks of its Gram matrix."""
        mp, np_, f32 = X.m_pad, X.n_pad, torch.float32
        self.Upanel, self.Vpanel = self._blocks((3, BK, mp), torch.int8), self._blocks((3, BK, np_), torch.int8)
        self.scaleU, self.scaleV = self._blocks((2 * BK,), f32), self._blocks((2 * BK,), f32)
        self._ws = self._zeros((max(mp, np_) // 128 * BK,), f32)
        with torch.cuda.device(self.device):
            self.splits_xv, self.splits_xtu = xf_slots_i8(mp, np_, BK), xf_slots_i8(np_, mp, BK)
            self._tiled = X.tiled()
        self.Mslab, self.Nslab = self._blocks((slab_sets * self.splits_xv, mp, BK), f32), self._blocks((slab_sets * self.splits_xtu, np_, BK), f32)
        self.gram_blocks = int(min(256, max(1, max(mp, np_) // 256)))
        self._gslabs = self._zeros((self.gram_blocks, BK, BK), f32)
        self.GU, self.GV = ([self._blocks((BK, BK), f32) for _ in range(self.nb)] for _ in range(2))
        # num: the contraction the update of this factor reads (X V for U); xf*: the GEMM with this factor (X^T U_b -> Nslab for U)
        self._extend_sides(U=dict(panel=self.Upanel, scale=self.scaleU, G=self.GU, Go=self.GV, num=self.Mslab, splits=self.splits_xv,
                                  xf=self.Nslab, xf_bits=self._tiled[1], xf_rows=np_, xf_ld=X.ldxt, xf_splits=self.splits_xtu),
                           V=dict(panel=self.Vpanel, scale=self.scaleV, G=self.GV, Go=self.GU, num=self.Nslab, splits=self.splits_xtu,
                                  xf=self.Mslab, xf_bits=self._tiled[0], xf_rows=mp, xf_ld=X.ldx, xf_splits=self.splits_xv))

    # ---- factors ------------------------------------------------------------------------------------------------------------
    def load_factors(self, U0, V0):
        U0, V0 = np.asarray(U0), np.asarray(V0)
        assert U0.shape == (self.m, self.k) and V0.shape == (self.n, self.k), (U0.shape, V0.shape)
        for s, F0 in ((self._side("U"), U0), (self._side("V"), V0)):
            split_into(s["F64"], F0)
            for b in range(self.nb):
                s["F"][b].copy_(s["F64"][b])

    def factors(self):
        return join(self.U64, self.m, self.k), join(self.V64, self.n, self.k)

    def _count_tuple(self, tp, fp):
        """(TP, FP, FN, TN) from the two counted ones and sum X."""
        fn = int(self.sum_x) - tp
        return tp, fp, fn, self.m_total * self.n - tp - fp - fn

    # ---- the fp64 element-wise update of one block ------------------------------------------------------------------------------
    def _epilogue_args(self, which, b, mode, reg, num, splits, den):
        """The argument block of ``bmf_mu_epilogue`` for block `b` of factor `which`: numerator slabs ``num[b]`` (`splits` of them;
        None: no numerator), denominator ``den[b]`` already carrying what couples the blocks."""
        s = self._side(which)
        a = L.EpilogueArgs()
        a.F64, a.F, a.rows_pad, a.rows, a.k, a.kp = s["F64"][b].data_ptr(), s["F"][b].data_ptr(), s["rows_pad"], s["rows"], self.kb[b], BK
        a.num, a.slab_stride, a.splits = (0 if num is None else num[b].data_ptr()), s["rows_pad"] * BK, splits
        a.G, a.den, a.reg, a.mode, a.thr, a.terms = 0, den[b].data_ptr(), float(reg), mode, float(s["thr"]), 0
        a.panel, a.ldp, a.rowbits, a.colbits, a.ldcb = 0, s["rows_pad"], s["rb"][b].data_ptr(), s["cb"][b].data_ptr(), s["rows_pad"] // 32
        a.partials, a.stop = s["part"][b].data_ptr(), 0
        return a

    def _mu_epilogue(self, which, b, mode, reg, num, splits, den):
        a = self._epilogue_args(which, b, mode, reg, num, splits, den)
        check(lib.bmf_mu_epilogue(C.byref(a), _stream()), "bmf_mu_epilogue")

    # ---- everything derived from a factor (after ``_alloc_derived``) --------------------------------------------------------------
    def _panel(self, F64, F, rows_pad, panel, scale, st):
        check(lib.bmf_make_panel_i8(ptr(F64), ptr(F), rows_pad, BK, BK, 3, ptr(panel), rows_pad, ptr(self._ws), ptr(scale), st), "bmf_make_panel_i8")

    def _planes(self, s, st):
        """The digit planes of both blocks of the factor of record `s`."""
        for b in range(self.nb):
            self._panel(s["F64"][b], s["F"][b], s["rows_pad"], s["panel"][b], s["scale"][b], st)

    def _gram_pair(self, s, a, b, g64, g64_t, st, stage=None):
        """F_a^T F_b in fp32 into s["G"][a][b] and in fp64 into `g64`; for a != b their transposes into s["G"][b][a] and `g64_t`.
        ``stage``: a contiguous 64 x 64 fp64 buffer the sum lands in first, when `g64` is a view into a larger matrix."""
        kk = BK * BK
        dst = g64 if stage is None else stage
        check(lib.bmf_gram_cross(ptr(s["F"][a]), ptr(s["F"][b]), s["rows_pad"], ptr(self._gslabs), self.gram_blocks, st), "bmf_gram_cross")
        check(lib.bmf_reduce_slabs(ptr(self._gslabs), kk, self.gram_blocks, kk, ptr(s["G"][a][b]), ptr(dst), st), "bmf_reduce_slabs")
        if stage is not None:
            g64.copy_(stage)
        if a != b:   # G[b][a] = G[a][b]^T
            s["G"][b][a].copy_(s["G"][a][b].t())
            g64_t.copy_(dst.t())

    def _bits_gemm(self, s, panel, scale, out, st):
        """X F_b (record of V) or X^T F_b (record of U) from one block's digit planes and scales into the slabs at `out`."""
        check(lib.bmf_xf_bits_i8(ptr(s["xf_bits"]), s["xf_rows"], s["xf_ld"], s["rows_pad"] // 32, ptr(panel), s["rows_pad"], 3, ptr(scale[BK:]), BK,
                                 ptr(out), s["xf_rows"] * BK, s["xf_splits"], 1, st), "bmf_xf_bits_i8")


# ---- the entry points that take both blocks of a factor, one call site each -----------------------------------------------------------
def cover_count_wide(B, ubits, vcolbits, counts):
    """TP / FP of the Boolean product over all 128 factors against the bits of `B`, added to `counts`."""
    check(lib.bmf_cover_count_wide(ptr(B.bits), B.m_pad, B.ldx, B.n_pad // 32, ptr(ubits[0]), ptr(ubits[1]), ptr(vcolbits[0]), ptr(vcolbits[1]),
                                   B.n_pad // 32, ptr(counts), _stream()), "bmf_cover_count_wide")


def resid_workspace(B):
    return torch.zeros(((B.m_pad + B.n_pad) * 2 * BK,), dtype=torch.int16, device=B.device)


def resid_sums_wide(B, bits_t, U, V, ws, sums, tiled=1):
    """sum |X - U V^T| and sum (X - U V^T)^2 with the product over both blocks, added to `sums`; `bits_t`: the bits of X^T, in the
    tiled layout (``B.tiled()[1]``) or, with tiled = 0, as ``B.bits_t``; `ws` from ``resid_workspace``."""
    check(lib.bmf_resid_sums_wide(ptr(bits_t), B.ldxt, B.m_pad, B.n_pad, ptr(U[0]), ptr(U[1]), ptr(V[0]), ptr(V[1]), ptr(ws), ptr(sums), tiled,
                                  _stream()), "bmf_resid_sums_wide")


def link_sums_wide(B, m, n, U, V, k, link, lamda, obs_bits, sums):
    """The objective sums of a link model against the link prediction over both blocks, added to `sums`; `obs_bits`: the bits of the
    observed cells the objective is restricted to, or None."""
    check(lib.bmf_link_sums_wide(ptr(B.bits), B.m_pad, B.ldx, m, n, ptr(U[0]), ptr(U[1]), ptr(V[0]), ptr(V[1]), B.n_pad, k, int(link), float(lamda),
                                 ptr(obs_bits), ptr(sums), _stream()), "bmf_link_sums_wide")


def masked_pass_wide(ls, rows, Fself, Fother, num, den, sums, link=0, lamda=0.0):
    """The pass over the observed cells `ls` (one orientation of a ``SparseObs``) with the dot product over both blocks: numerators
    and denominators per block, the objective sums added to `sums` (or None); with `link` the product goes through the link.  The
    per-segment partials stay with `ls`, made on first use."""
    if ls.get("part_wide") is None:
        ls["part_wide"] = [torch.zeros((max(ls["nseg"], 1), 2, BK), dtype=torch.float32, device=Fself[0].device) for _ in range(2)]
    p0, p1 = ls["part_wide"]
    args = (ptr(ls["ptr"]), ptr(ls["idx"]), ptr(ls["val"]), ptr(ls["wgt"]), rows, ptr(ls["seg_row"]), ptr(ls["seg_beg"]), ls["nseg"],
            ptr(ls["row_seg_ptr"]), ptr(Fself[0]), ptr(Fself[1]), ptr(Fother[0]), ptr(Fother[1]), ptr(p0), ptr(p1), ptr(num[0]), ptr(num[1]),
            ptr(den[0]), ptr(den[1]), ptr(sums))
    if link:
        check(lib.bmf_masked_link_pass_wide(*args, int(link), float(lamda), _stream()), "bmf_masked_link_pass_wide")
    else:
        check(lib.bmf_masked_pass_wide(*args, _stream()), "bmf_masked_pass_wide")
