"""What the host engines of the Boolean models share (grecond / grecondplus / asso / asso_refine / mebf / panda .py): the packed-word
helpers and ``BitSetEngine``, the part of an engine that does not depend on the algorithm -- the ground truths, the stream, the
confusion counts of the prediction bits (csrc/bits_common.hip), the factors as arrays and the prediction as csr.

Packed words are little-endian uint32: bit i of a set is bit i % 32 of word i // 32, zero padded.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import check, lib, ptr
from .engine import BitMatrix

POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def pack_bits(flags, words: int) -> np.ndarray:
    """A 0 / 1 vector as `words` little-endian uint32 words (bit i of word i // 32), zero padded."""
    flags = np.asarray(flags).astype(bool).ravel()
    out = np.zeros(words * 32, dtype=np.uint8)
    out[: flags.size] = flags
    return np.packbits(out, bitorder="little").view(np.uint32).copy()


def unpack_bits(words, length: int) -> np.ndarray:
    """The first `length` bits of packed uint32 words as a bool vector."""
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:length].astype(bool)


def popcount(words) -> int:
    return int(POP8[np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)].sum())


def bit_positions(words) -> np.ndarray:
    """The set bits of packed uint32 words, ascending."""
    return np.nonzero(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little"))[0].astype(np.int32)


class BitSetEngine:
    """A subclass names itself (`title`, for the refusals), keeps its applied factors as packed (u, v) in `_factors` and says with
    `_pd_bits()` where its prediction bits are."""
    title = None

    def __init__(self, bits: BitMatrix, extra: dict = None):
        """bits: the training matrix.  extra: {name: BitMatrix} of further ground truths of the same shape (val / test)."""
        self.bits, self.m, self.n = bits, bits.m, bits.n
        self.device = dev = bits.device
        self.sum_x = int(bits.sum_local)
        self.truth = {"train": bits}
        for name, B in (extra or {}).items():
            if (B.m, B.n, B.device) != (bits.m, bits.n, bits.device):
                raise ValueError(f"the {name} matrix must have the shape and the device of X")
            self.truth[name] = B
        with torch.cuda.device(dev):
            self._conf_work = torch.zeros(2 * max(self.m, self.n), dtype=torch.int32, device=dev)
            self._conf = torch.zeros(2, dtype=torch.int64, device=dev)
            self._stream_obj = torch.cuda.current_stream()
        self._stream = C.c_void_p(self._stream_obj.cuda_stream)

    def _on_stream(self):
        return torch.cuda.stream(self._stream_obj)

    @staticmethod
    def _p(tensor, word=0):
        return C.c_void_p(tensor.data_ptr() + 4 * word)

    def _require_free(self, need: int, what: str, hint: str = ""):
        """Refuse when `need` more bytes of device memory are not free.  what: the subject and its verb; hint: what is not built."""
        free_b, _ = torch.cuda.mem_get_info(self.device)
        if need > free_b:
            raise NotImplementedError(f"{self.title} on {self.m} x {self.n}: {what} {need} more bytes ({need / 2 ** 30:.2f} GiB), "
                                      f"{free_b} bytes ({free_b / 2 ** 30:.2f} GiB) of device memory are free{hint}")

    # ---- prediction ---------------------------------------------------------------------------------------------------
    def _pd_bits(self, for_counts: bool):
        """(the prediction's bit tensor, True when it is the transposed one).  An engine that keeps both orientations may hand
        counts() one and prediction() the other."""
        raise NotImplementedError

    def counts(self, name="train"):
        """(TP, FP, FN, TN) of the prediction bits against data set `name`."""
        G = self.truth[name]
        pd, transposed = self._pd_bits(True)
        gt, rows, ld = (G.bits_t, self.n, self.bits.ldxt) if transposed else (G.bits, self.m, self.bits.ldx)
        with torch.cuda.device(self.device), self._on_stream():
            check(lib.bmf_bits_confusion(ptr(pd), ptr(gt), rows, ld, ptr(self._conf_work), ptr(self._conf), self._stream),
                  "bmf_bits_confusion")
            tp, n_pd = (int(x) for x in self._conf.cpu().numpy())
        fp, fn = n_pd - tp, int(G.sum_local) - tp
        return tp, fp, fn, self.m * self.n - tp - fp - fn

    def factor_arrays(self):
        """(U, V) of the applied factors as uint8 arrays of shape (m, f) and (n, f)."""
        fs = self._factors
        U, V = np.zeros((self.m, len(fs)), dtype=np.uint8), np.zeros((self.n, len(fs)), dtype=np.uint8)
        for i, (u, v) in enumerate(fs):
            U[:, i], V[:, i] = unpack_bits(u, self.m), unpack_bits(v, self.n)
        return U, V

    def prediction(self):
        """X_pd as a scipy csr matrix, from the device bits."""
        from scipy.sparse import csr_matrix
        pd, transposed = self._pd_bits(False)
        rows, cols = (self.n, self.m) if transposed else (self.m, self.n)
        dense = np.unpackbits(pd[:rows].cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :cols]
        return csr_matrix((dense.T if transposed else dense).astype(int))
