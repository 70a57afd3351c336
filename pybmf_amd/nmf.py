"""Device state and step driver of coordinate-descent NMF (scikit-learn's Frobenius 'cd' solver: the model ``NMFSklearn``).

One iteration of the solver is, per factor, the k x k Gram of the other factor, the contraction of X with it and a sweep over the
rows of the factor that moves (``bmf_nmf_cd_sweep``, csrc/nmf_cd.hip); the Gram and the contraction are the kernels of the
multiplicative-update path.  ``bmf_nmf_cd_iterate`` enqueues a whole iteration and leaves the two violations in pinned host memory;
the stopping rule looks at them on the host, one read per iteration.

``bits_product`` is the other use of the bits GEMM here: X T or X^T T for a thin real matrix T of any sign (the products of the
randomised SVD behind the NNDSVD initialisers), in blocks of 32 or 64 columns, T quantised to three int8 digit planes like a factor.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr
from .engine import BitMatrix, HostRows, _stream, xf_slots_i8


def bits_product(X: BitMatrix, T, transposed: bool = False) -> np.ndarray:
    """X @ T (T: n x c), or X^T @ T (T: m x c) when ``transposed``, as fp64 on the host.  The bits of X are exact; T enters as 24-bit
    integers per column (relative to the column's largest entry), the sums are exact and leave the device as fp32 slabs."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    red, red_pad, rows, rows_pad = (X.m, X.m_pad, X.n, X.n_pad) if transposed else (X.n, X.n_pad, X.m, X.m_pad)
    if T.ndim != 2 or T.shape[0] != red:
        raise ValueError(f"bits_product: T has shape {T.shape}, expected {red} rows")
    dev = X.device
    out = np.empty((rows, T.shape[1]), dtype=np.float64)
    with torch.cuda.device(dev):
        tiled = X.tiled()[1 if transposed else 0]
        st = _stream()
        c0 = 0
        while c0 < T.shape[1]:
            cw = min(64, T.shape[1] - c0)
            kb = 32 if cw <= 32 else 64
            F64 = torch.zeros((red_pad, kb), dtype=torch.float64, device=dev)
            F64[:red, :cw] = torch.from_numpy(T[:, c0:c0 + cw]).to(dev)
            F = F64.to(torch.float32)
            panel = torch.zeros((3, kb, red_pad), dtype=torch.int8, device=dev)
            scale = torch.zeros((2 * kb,), dtype=torch.float32, device=dev)
            ws = torch.zeros((red_pad // 128 * kb,), dtype=torch.float32, device=dev)
            splits = xf_slots_i8(rows_pad, red_pad, kb)
            slabs = torch.zeros((splits, rows_pad, kb), dtype=torch.float32, device=dev)
            res = torch.zeros((rows_pad, kb), dtype=torch.float64, device=dev)
            check(lib.bmf_make_panel_i8(ptr(F64), ptr(F), red_pad, kb, kb, 3, ptr(panel), red_pad, ptr(ws), ptr(scale), st), "bmf_make_panel_i8")
            check(lib.bmf_xf_bits_i8(ptr(tiled), rows_pad, red_pad // 32, red_pad // 32, ptr(panel), red_pad, 3, ptr(scale[kb:]), kb, ptr(slabs),
                                     rows_pad * kb, splits, 1, st), "bmf_xf_bits_i8")
            check(lib.bmf_reduce_slabs(ptr(slabs), rows_pad * kb, splits, rows_pad * kb, None, ptr(res), st), "bmf_reduce_slabs")
            out[:, c0:c0 + cw] = res[:rows, :cw].cpu().numpy()
            c0 += cw
    return out


class NMFEngine:
    def __init__(self, X: BitMatrix, k: int):
        if not (1 <= k <= L.MAX_KP):
            raise NotImplementedError(f"k={k}: this build supports 1 <= k <= {L.MAX_KP}")
        self.X, self.k = X, int(k)
        self.kp = kp = 32 if k <= 32 else 64
        dev = self.device = X.device
        mp, np_ = X.m_pad, X.n_pad
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.U64, self.V64 = z((mp, kp), torch.float64), z((np_, kp), torch.float64)
        self.U, self.V = z((mp, kp), torch.float32), z((np_, kp), torch.float32)
        self.Upanel, self.Vpanel = z((3, kp, mp), torch.int8), z((3, kp, np_), torch.int8)
        self.scaleU, self.scaleV = z((2 * kp,), torch.float32), z((2 * kp,), torch.float32)
        self.wsU, self.wsV = z((mp // 128 * kp,), torch.float32), z((np_ // 128 * kp,), torch.float32)
        with torch.cuda.device(dev):
            self.splits_xv, self.splits_xtu = xf_slots_i8(mp, np_, kp), xf_slots_i8(np_, mp, kp)
            self._tiled = X.tiled()
            self._ring = HostRows()   # the violations are written by the device straight into pinned host memory
        self.Mslab, self.Nslab = z((self.splits_xv, mp, kp), torch.float32), z((self.splits_xtu, np_, kp), torch.float32)
        self.gram_blocks = int(min(256, max(1, max(mp, np_) // 256)))
        self.gram_slabs = z((self.gram_blocks, kp, kp), torch.float32)
        self.GU, self.GV = z((kp, kp), torch.float32), z((kp, kp), torch.float32)
        self.GU64, self.GV64 = z((kp * kp,), torch.float64), z((kp * kp,), torch.float64)
        self.partU, self.partV = z((mp // 128,), torch.float64), z((np_ // 128,), torch.float64)
        self.dot_blocks = 1024
        self.dotpart = z((self.dot_blocks,), torch.float64)
        self.sum_x = float(X.sum_local)
        st = self._st = L.NmfState()
        st.struct_bytes = C.sizeof(L.NmfState)
        st.m, st.n, st.k, st.kp = X.m, X.n, self.k, kp
        st.splits_xv, st.splits_xtu, st.gram_blocks, st.log_rows = self.splits_xv, self.splits_xtu, self.gram_blocks, HostRows.LOG_ROWS
        st.m_pad, st.n_pad = mp, np_
        st.Xtiled, st.XTtiled = self._tiled[0].data_ptr(), self._tiled[1].data_ptr()
        for name in ("U64", "V64", "U", "V", "Upanel", "Vpanel", "scaleU", "scaleV", "wsU", "wsV", "Mslab", "Nslab", "gram_slabs", "GU", "GV",
                     "GU64", "GV64", "partU", "partV"):
            setattr(st, name, getattr(self, name).data_ptr())
        st.log = self._ring.host.data_ptr()
        self._last = -1

    def load_factors(self, U0, V0):
        """Initial factors (V is n x k); the digit planes of V are what the first half-iteration contracts X with."""
        X = self.X
        for F64, F, F0, rows in ((self.U64, self.U, U0, X.m), (self.V64, self.V, V0, X.n)):
            F0 = np.ascontiguousarray(F0, dtype=np.float64)
            if F0.shape != (rows, self.k):
                raise ValueError(f"factor of shape {F0.shape}, expected {(rows, self.k)}")
            F64.zero_()
            F64[:rows, : self.k] = torch.from_numpy(F0).to(self.device)
            F.copy_(F64)
        self._panel_v()

    def _panel_v(self):
        X, kp = self.X, self.kp
        with torch.cuda.device(self.device):
            check(lib.bmf_make_panel_i8(ptr(self.V64), ptr(self.V), X.n_pad, kp, kp, 3, ptr(self.Vpanel), X.n_pad, ptr(self.wsV), ptr(self.scaleV),
                                        _stream()), "bmf_make_panel_i8")

    def product(self, T, transposed: bool = False) -> np.ndarray:
        """X @ T, or X^T @ T when ``transposed`` (the products of the NNDSVD initialisers)."""
        return bits_product(self.X, T, transposed)

    def iterate(self, it: int):
        """Enqueue iteration `it` (0-based): the sweep of U, then the sweep of V with the new U; ``row(it)`` waits for its violations."""
        with torch.cuda.device(self.device):
            check(lib.bmf_nmf_cd_iterate(C.byref(self._st), int(it), _stream()), "bmf_nmf_cd_iterate")
            self._ring.mark(it)
        self._last = it

    def row(self, it: int):
        """(violation of the U sweep, violation of the V sweep) of iteration `it`."""
        if not self._ring.has(it):
            raise RuntimeError(f"row {it} is not available (last iteration enqueued: {self._last})")
        h = self._ring.wait(it)
        return float(h[0]), float(h[1])

    def factors(self):
        X = self.X
        return self.U64[: X.m, : self.k].cpu().numpy(), self.V64[: X.n, : self.k].cpu().numpy()

    def rec_error(self) -> float:
        """||X - U V^T||_F^2 = ||X||^2 - 2 <U, X V> + <U^T U, V^T V> of the current factors, from fp64 scalars."""
        X, kp, kk = self.X, self.kp, self.kp * self.kp
        with torch.cuda.device(self.device):
            st = _stream()
            for F, rows_pad, G, G64 in ((self.U, X.m_pad, self.GU, self.GU64), (self.V, X.n_pad, self.GV, self.GV64)):
                check(lib.bmf_gram_partial(ptr(F), rows_pad, kp, kp, ptr(self.gram_slabs), self.gram_blocks, st), "bmf_gram_partial")
                check(lib.bmf_reduce_slabs(ptr(self.gram_slabs), kk, self.gram_blocks, kk, ptr(G), ptr(G64), st), "bmf_reduce_slabs")
            check(lib.bmf_xf_bits_i8(ptr(self._tiled[0]), X.m_pad, X.n_pad // 32, X.n_pad // 32, ptr(self.Vpanel), X.n_pad, 3, ptr(self.scaleV[kp:]), kp,
                                     ptr(self.Mslab), X.m_pad * kp, self.splits_xv, 1, st), "bmf_xf_bits_i8")
            n = X.m_pad * kp
            check(lib.bmf_dot_slabs(ptr(self.U64), ptr(self.Mslab), n, self.splits_xv, n, ptr(self.dotpart), self.dot_blocks, st), "bmf_dot_slabs")
            cross = float(self.dotpart.cpu().numpy().sum())
            gram = float(np.dot(self.GU64.cpu().numpy(), self.GV64.cpu().numpy()))
        return self.sum_x - 2.0 * cross + gram
