"""Device state of a FastStep fit (``PyBMF/models/FastStep.py``): the fp64 master factors, B_k = U V^T - U[:, k] V[:, k]^T - tau of
the factor being searched, the bits of X (and of the mask), and the scratch of the evaluation pass (csrc/faststep.hip).

    eng.set_factor(k)                                  rebuild B_k from the masters
    F, du, dv, tp, fp = eng.evaluate(u, v, want_grad, want_counts)
    eng.commit(k, u, v)                                write the accepted column into the masters

The (m + n)-vector of a candidate crosses the bus once per evaluation (pinned staging buffer, at most 1 MB), the results come back in
one copy.  Every launch goes to the stream that was current when the engine was made; an evaluation ends with a synchronisation of it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .engine import BitMatrix


class FastStepEngine:
    def __init__(self, bits: BitMatrix, k: int, tau: float, U, V, mask: BitMatrix = None):
        if k > L.MAX_KP:
            raise NotImplementedError(f"k={k}: FastStep supports k <= {L.MAX_KP}")
        self.bits, self.mask = bits, mask
        if mask is not None and (mask.m_pad, mask.n_pad, mask.ldx, mask.device) != (bits.m_pad, bits.n_pad, bits.ldx, bits.device):
            raise ValueError("the mask must have the shape and the device of X")
        self.m, self.n, self.k, self.tau = bits.m, bits.n, int(k), float(tau)
        self.kp = 32 if k <= 32 else 64
        self.sum_x = int(bits.sum_local)
        self.device = dev = bits.device
        m_pad, n_pad = bits.m_pad, bits.n_pad
        n_work = int(lib.bmf_faststep_eval_work(m_pad, n_pad, self.m, self.n))
        if n_work < 0:
            check(n_work, "bmf_faststep_eval_work")
        with torch.cuda.device(dev):
            # B_k is 8 bytes per padded cell (16 GB at 100 000 x 20 000): refuse before the allocator does
            need = (m_pad * n_pad + n_work) * 8
            free_b, _ = torch.cuda.mem_get_info(dev)
            if need > free_b:
                raise NotImplementedError(f"FastStep on {self.m} x {self.n}: the fp64 base matrix of the factor being searched takes "
                                          f"{need / 2 ** 30:.1f} GiB, {free_b / 2 ** 30:.1f} GiB of device memory are free")
            self.B = torch.empty((m_pad, n_pad), dtype=torch.float64, device=dev)
            self.work = torch.empty(n_work, dtype=torch.float64, device=dev)
            self.Ud = torch.zeros((m_pad, self.kp), dtype=torch.float64, device=dev)
            self.Vd = torch.zeros((n_pad, self.kp), dtype=torch.float64, device=dev)
            self.Ud[: self.m, : self.k] = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float64)).to(dev)
            self.Vd[: self.n, : self.k] = torch.from_numpy(np.ascontiguousarray(V, dtype=np.float64)).to(dev)
            # candidate: [u (m) | v (n)];  result: [F, TP, FP (int64 bit patterns), unused | du (m) | dv (n)]
            self._x_host = torch.zeros(self.m + self.n, dtype=torch.float64).pin_memory()
            self._x_dev = torch.zeros(self.m + self.n, dtype=torch.float64, device=dev)
            self._res_dev = torch.zeros(4 + self.m + self.n, dtype=torch.float64, device=dev)
            self._res_host = torch.zeros(4 + self.m + self.n, dtype=torch.float64).pin_memory()
            self._stream_obj = torch.cuda.current_stream()
        self._x_np, self._res_np = self._x_host.numpy(), self._res_host.numpy()
        self._res_i64 = self._res_np.view(np.int64)
        self._stream = C.c_void_p(self._stream_obj.cuda_stream)
        self._factor = None

    def set_factor(self, k: int):
        """B_k = U V^T - tau without latent column k, from the masters as they stand."""
        assert 0 <= k < self.k
        B = self.bits
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream_obj):
            check(lib.bmf_faststep_base(ptr(self.Ud), ptr(self.Vd), B.m_pad, B.n_pad, self.m, self.n, self.k, self.kp, int(k), self.tau,
                                        ptr(self.B), self._stream), "bmf_faststep_base")
        self._factor = int(k)

    def evaluate(self, u, v, want_grad=True, want_counts=False):
        """(F, du, dv, tp, fp) at the candidate column (u, v) of the factor chosen by set_factor(); du / dv are None without
        want_grad, tp / fp without want_counts."""
        if self._factor is None:
            raise RuntimeError("set_factor(k) first")
        m, n, B = self.m, self.n, self.bits
        self._x_np[:m] = u
        self._x_np[m:] = v
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream_obj):
            self._x_dev.copy_(self._x_host, non_blocking=True)
            base, res = self._x_dev.data_ptr(), self._res_dev.data_ptr()
            check(lib.bmf_faststep_eval(ptr(self.B), ptr(B.bits), None if self.mask is None else ptr(self.mask.bits), B.m_pad, B.n_pad,
                                        B.ldx, m, n, C.c_void_p(base), C.c_void_p(base + 8 * m), int(want_grad), int(want_counts),
                                        ptr(self.work), C.c_void_p(res), C.c_void_p(res + 32) if want_grad else None,
                                        C.c_void_p(res + 32 + 8 * m) if want_grad else None, C.c_void_p(res + 8) if want_counts else None,
                                        self._stream), "bmf_faststep_eval")
            n_back = 4 + m + n if want_grad else 4
            self._res_host[:n_back].copy_(self._res_dev[:n_back], non_blocking=True)
            self._stream_obj.synchronize()
        F = float(self._res_np[0])
        du = self._res_np[4:4 + m].copy() if want_grad else None
        dv = self._res_np[4 + m:4 + m + n].copy() if want_grad else None
        tp, fp = (int(self._res_i64[1]), int(self._res_i64[2])) if want_counts else (None, None)
        return F, du, dv, tp, fp

    def commit(self, k: int, u, v):
        """Column k of the masters := (u, v).  B_k does not hold column k, so it stays valid."""
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream_obj):
            self.Ud[: self.m, k] = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(self.device)
            self.Vd[: self.n, k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(self.device)

    def prediction(self):
        """(U V^T > tau) of the masters as a scipy csr matrix: the fp64 product on the device, thresholded there.  Overwrites B_k."""
        from scipy.sparse import csr_matrix
        B = self.bits
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream_obj):
            check(lib.bmf_faststep_base(ptr(self.Ud), ptr(self.Vd), B.m_pad, B.n_pad, self.m, self.n, self.k, self.kp, -1, self.tau,
                                        ptr(self.B), self._stream), "bmf_faststep_base")
            self._factor = None
            pd = (self.B[: self.m, : self.n] > 0).cpu().numpy()
        return csr_matrix(pd.astype(int))

    def factors(self):
        return self.Ud[: self.m, : self.k].cpu().numpy(), self.Vd[: self.n, : self.k].cpu().numpy()
