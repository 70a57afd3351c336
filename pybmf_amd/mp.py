"""Device state of a MessagePassing fit (``pybmf_amd/models/MessagePassing.py``; csrc/mp.hip): the 2 k fp64 hat messages of every cell
as k planes of m x ldn doubles per side (ldn = n rounded up to 64), the marginals Xi [m][k] and Ups [k][ldn], the bits of X (and of the
observation pattern) and the partial-sum workspace.

    eng.start(seed)            the counter-based fill on the pattern, then the sums: nothing of size m n k crosses the bus
    d = eng.step()             one Jacobi iteration of every observed cell; d = the largest change of a marginal
    Xi, Ups = eng.marginals()  (m, k) and (n, k) fp64
    U, V = eng.decisions()     (Xi > 0), (Ups > 0) as bool arrays, from the bits the device formed
    Ph, Ps = eng.messages()    the hats as (m, n, k) arrays (tests)

Every launch goes to the stream that was current when the engine was made; step() ends with one 8-byte read of d through pinned
memory and a synchronisation of that stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib, ptr
from .engine import BitMatrix, round_up


def channel_constants(prior_u, prior_v, channel_pos, channel_neg):
    """(cx, cy, co1, co0): the log odds of the priors and of the channel where X = 1 / X = 0."""
    return (float(np.log(prior_u / (1 - prior_u))), float(np.log(prior_v / (1 - prior_v))),
            float(np.log(channel_pos / (1 - channel_neg))), float(np.log((1 - channel_pos) / channel_neg)))


class MessagePassingEngine:
    def __init__(self, bits: BitMatrix, k: int, pattern: BitMatrix = None, prior_u=0.5, prior_v=0.5, channel_pos=0.99, channel_neg=0.99,
                 lr=0.2, init_scale=1e-2):
        if not 1 <= k <= L.MAX_KP:
            raise NotImplementedError(f"k={k}: MessagePassing supports 1 <= k <= {L.MAX_KP}")
        if pattern is not None and (pattern.m, pattern.n, pattern.ldx, pattern.device) != (bits.m, bits.n, bits.ldx, bits.device):
            raise ValueError("the pattern must have the shape and the device of X")
        self.bits, self.pattern = bits, pattern
        self.m, self.n, self.k = bits.m, bits.n, int(k)
        self.ldn = round_up(self.n, 64)
        self.lr, self.init_scale = float(lr), float(init_scale)
        self.cx, self.cy, self.co1, self.co0 = channel_constants(prior_u, prior_v, channel_pos, channel_neg)
        self.device = dev = bits.device
        n_work = int(lib.bmf_mp_work(self.m, self.n, self.k))
        if n_work < 0:
            check(n_work, "bmf_mp_work")
        m, n, k, ldn = self.m, self.n, self.k, self.ldn
        with torch.cuda.device(dev):
            # 16 k bytes per padded cell (5.2 GB at 10 000 x 2 000, k = 16): refuse before the allocator does
            need = 2 * m * ldn * k * 8 + n_work * 8
            free_b, _ = torch.cuda.mem_get_info(dev)
            if need > free_b:
                raise NotImplementedError(f"MessagePassing on {m} x {n}, k = {k}: the fp64 messages and their partial sums take {need} "
                                          f"bytes ({need / 2 ** 30:.2f} GiB), {free_b} bytes ({free_b / 2 ** 30:.2f} GiB) of device "
                                          "memory are free")
            self.Phi = torch.zeros((k, m, ldn), dtype=torch.float64, device=dev)
            self.Psi = torch.zeros((k, m, ldn), dtype=torch.float64, device=dev)
            self.work = torch.empty(n_work, dtype=torch.float64, device=dev)
            self.Xi = torch.zeros((m, k), dtype=torch.float64, device=dev)
            self.Ups = torch.zeros((k, ldn), dtype=torch.float64, device=dev)
            self.ubits = torch.zeros(m, dtype=torch.int64, device=dev)
            self.vbits = torch.zeros(n, dtype=torch.int64, device=dev)
            self._d_dev = torch.zeros(1, dtype=torch.float64, device=dev)
            self._d_host = torch.zeros(1, dtype=torch.float64).pin_memory()
            self._stream_obj = torch.cuda.current_stream()
        self._d_np = self._d_host.numpy()
        self._stream = C.c_void_p(self._stream_obj.cuda_stream)
        self._started = False

    def _on_stream(self):
        return torch.cuda.stream(self._stream_obj)

    def _wbits(self):
        return None if self.pattern is None else ptr(self.pattern.bits)

    def start(self, seed: int):
        """The hats := init_scale (2 u - 1) on the pattern (u from splitmix64 of the cell's counter), the marginals := their sums."""
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_mp_start(self._wbits(), self.bits.ldx, self.m, self.n, self.k, self.ldn, int(seed) & (2 ** 64 - 1), self.init_scale,
                                   ptr(self.Phi), ptr(self.Psi), self._stream), "bmf_mp_start")
            check(lib.bmf_mp_reduce(ptr(self.Phi), ptr(self.Psi), self.m, self.n, self.k, self.ldn, self.cx, self.cy, ptr(self.work),
                                    ptr(self.Xi), ptr(self.Ups), ptr(self._d_dev), ptr(self.ubits), ptr(self.vbits), self._stream),
                  "bmf_mp_reduce")
        self._started = True

    def step(self) -> float:
        """One iteration; returns d = max(max |Xi_new - Xi|, max |Ups_new - Ups|)."""
        if not self._started:
            raise RuntimeError("start(seed) first")
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_mp_step(ptr(self.bits.bits), self._wbits(), self.bits.ldx, self.m, self.n, self.k, self.ldn, self.co1, self.co0,
                                  self.lr, self.cx, self.cy, ptr(self.Phi), ptr(self.Psi), ptr(self.work), ptr(self.Xi), ptr(self.Ups),
                                  ptr(self._d_dev), ptr(self.ubits), ptr(self.vbits), self._stream), "bmf_mp_step")
            self._d_host.copy_(self._d_dev, non_blocking=True)
            self._stream_obj.synchronize()
        return float(self._d_np[0])

    def marginals(self):
        with torch.cuda.device(self.device), self._on_stream():
            return self.Xi.cpu().numpy(), np.ascontiguousarray(self.Ups[:, : self.n].cpu().numpy().T)

    def decisions(self):
        with torch.cuda.device(self.device), self._on_stream():
            ub, vb = self.ubits.cpu().numpy().view(np.uint64), self.vbits.cpu().numpy().view(np.uint64)
        f = np.arange(self.k, dtype=np.uint64)
        return ((ub[:, None] >> f) & np.uint64(1)).astype(bool), ((vb[:, None] >> f) & np.uint64(1)).astype(bool)

    def messages(self):
        with torch.cuda.device(self.device), self._on_stream():
            return (np.ascontiguousarray(self.Phi[:, :, : self.n].cpu().numpy().transpose(1, 2, 0)),
                    np.ascontiguousarray(self.Psi[:, :, : self.n].cpu().numpy().transpose(1, 2, 0)))
