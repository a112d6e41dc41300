"""Python face of the coherent antenna combiner (include/sonde_abi.h, DESIGN SPEC 3.14): thin, no compute -- every call goes through
the C ABI of libsonde_mi355.so.

    SondeCombiner       the K antennas' complex64 rows of each sonde (row a * n_sondes + i = sonde i on antenna a, as K tuners with
                        the same VFO list write them) -> one row per sonde, y = sum_a conj(w_a) x_a, the weights per block of about
                        21 ms from the block's own M = sum x x^H
    weights()           the weights rule (sonde_combine_weights): pure host
    share()             |w_a|^2 of one antenna (sonde_combine_share)

The antennas share one sample clock and start together; DiversityReceiver(combine="coherent") (diversity.py) is the receiver built on it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._handle import Handle, chk, complex_rows, complex_stride, current_stream
from ._lib import COMBINE_DTYPE, INPUT_IQ, SondeError


def defaults(rate: int) -> int:
    """the block length the combiner picks for rows at `rate` (sonde_combine_defaults)"""
    b = C.c_uint32()
    chk(_lib.load().sonde_combine_defaults(int(rate), C.byref(b)))
    return b.value


def weights(m, w_prev=None, antennas: int | None = None) -> np.ndarray:
    """the weights of one block (sonde_combine_weights): m = the 16 doubles of M (COMBINE_DTYPE "m"), w_prev = the previous block's
    weights as K complex numbers (None: after a restart; then `antennas` says K).  Returns K complex128."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (16,):
        raise SondeError("m must hold the 16 doubles of M")
    if w_prev is None:
        if antennas is None:
            raise SondeError("antennas is needed where there are no previous weights")
        K, prev = int(antennas), None
    else:
        wp = np.ascontiguousarray(w_prev, dtype=np.complex128)
        K, prev = len(wp), wp.ctypes.data_as(C.c_void_p)
    w = np.zeros(max(K, 1), dtype=np.complex128)
    chk(_lib.load().sonde_combine_weights(K, m.ctypes.data_as(C.c_void_p), prev, w.ctypes.data_as(C.c_void_p)))
    return w[:K]


def share(w, a: int) -> float:
    """antenna a's share |w_a|^2 of the complex weights w (sonde_combine_share)"""
    w = np.ascontiguousarray(w, dtype=np.complex128)
    if not 0 <= int(a) < len(w):
        raise SondeError("no such antenna")
    return float(_lib.load().sonde_combine_share(w.ctypes.data_as(C.c_void_p), int(a)))


class SondeCombiner(Handle):
    """The combiner of `antennas` (2..4) rows per sonde at `rate`.  process() takes a float32 device view [antennas * n_sondes, n, 2]
    (rows any stride apart, contiguous inside a row), n a positive multiple of `block` and <= max_samples, and returns [n_sondes, n, 2]
    or writes it into `out` (a float32 view [n_sondes, >= n, 2] that does not overlap the rows: a SondeBatch input buffer will do).
    readout() synchronises and returns the last submit's blocks (COMBINE_DTYPE: sonde, block, m, w, wf), sonde by sonde."""
    DESTROY = "sonde_combine_destroy"

    def __init__(self, n_sondes: int, antennas: int, rate: int, max_samples: int, block: int = 0, device: int = 0, *, input_kind: int = INPUT_IQ):
        self._create("sonde_combine_create", int(n_sondes), int(antennas), int(rate), int(max_samples), int(block), int(input_kind), int(device))
        h = self.h
        self.n_sondes, self.antennas, self.rate, self.max_samples, self.device = int(n_sondes), int(antennas), int(rate), int(max_samples), int(device)
        self.block = int(self.L.sonde_combine_block(h))
        self._last = 0

    def process(self, rows, out=None, stream: int | None = None):
        import torch
        n, stride = complex_rows(rows, self.antennas * self.n_sondes, self.device, "combiner", "antennas * n_sondes",
                                 f"{self.antennas} x {self.n_sondes}", "phase")
        if out is None:
            out = torch.empty((self.n_sondes, n, 2), dtype=torch.float32, device=rows.device)
        ostride = complex_stride(out)
        if ostride is None or out.shape[0] != self.n_sondes or out.shape[1] < n or out.device != rows.device:
            raise SondeError("out must be a float32 device view [n_sondes, >= n, 2], contiguous inside a row")
        if stream is None:
            stream = current_stream(rows.device)
        self._keep = (rows, out)
        chk(self.L.sonde_combine_process(self.h, C.c_void_p(rows.data_ptr()), n, stride, C.c_void_p(out.data_ptr()), ostride, C.c_void_p(stream)))
        self._last = n // self.block
        return out[:, :n]

    def restart(self, i: int):
        """sonde i's next block starts a stream of its own: block index 0, no previous weights (after a retune or a slot reuse)"""
        chk(self.L.sonde_combine_restart(self.h, int(i)))

    def readout(self) -> np.ndarray:
        out = np.zeros(self.n_sondes * self._last, dtype=COMBINE_DTYPE)
        n = chk(self.L.sonde_combine_readout(self.h, out.ctypes.data_as(C.c_void_p), len(out)))
        return out[:n]
