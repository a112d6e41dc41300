"""Python face of the sonde type detector (include/sonde_abi.h, DESIGN SPEC 3.8): thin, no compute -- every call goes through the
C ABI of libsonde_mi355.so.

For channels of unknown type: detect, then build the SondeBatch from the detected types, e.g.

    det = SondeDetector(C, n)
    det.submit(rows)
    kind = det.results()["type"]          # -1: nothing decided yet
    SondeBatch(C, n, types=np.where(kind < 0, 0, kind))
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._handle import Handle, channel_rows, chk
from ._lib import DETECTION_DTYPE, INPUT_IQ, SondeError

NTYPES = 7


def templates(sonde_type: int) -> np.ndarray:
    """the type's sync template as +-1 int8 at its stream rate (24 kS/s GFSK, 6 kS/s AFSK)"""
    L = _lib.load()
    n = chk(L.sonde_detect_templates(int(sonde_type), None, 0))
    out = np.zeros(n, np.int8)
    chk(L.sonde_detect_templates(int(sonde_type), out.ctypes.data_as(C.c_void_p), n))
    return out


def thresholds() -> np.ndarray:
    """theta_k of the decision, float32 [7]"""
    out = np.zeros(NTYPES, np.float32)
    chk(_lib.load().sonde_detect_thresholds(out.ctypes.data_as(C.c_void_p)))
    return out


class SondeDetector(Handle):
    """Sonde type of many 48 kS/s channels, one HIP workgroup per channel.  submit() takes the rows SondeBatch.submit takes:
    a device tensor [C, n, 2] (float32 IQ, int16 for INPUT_IQ16, int8 for INPUT_IQ8) or [C, n] float32 (INPUT_REAL), n % 2048 == 0,
    strided between channels only.  type_mask: None or C bitmasks (bit k: type k may be decided)."""
    DESTROY = "sonde_detect_destroy"

    def __init__(self, n_channels: int, max_samples: int, *, input_kind: int = INPUT_IQ, type_mask=None, device: int = 0):
        self.n_channels = int(n_channels)
        self.max_samples = int(max_samples)
        self.input_kind = input_kind
        self.device = int(device)
        self._mask = None
        mp = None
        if type_mask is not None:
            self._mask = np.ascontiguousarray(type_mask, dtype=np.uint8)
            if self._mask.shape != (self.n_channels,):
                raise SondeError("type_mask must hold one bitmask per channel")
            mp = self._mask.ctypes.data_as(C.c_void_p)
        self._create("sonde_detect_create", self.n_channels, self.max_samples, input_kind, mp, self.device)

    def submit(self, samples, stream: int | None = None):
        n, stride = channel_rows(samples, self.input_kind, self.n_channels, self.device, "detector")
        self._keep = samples
        chk(self.L.sonde_detect_submit(self.h, C.c_void_p(samples.data_ptr()), n, stride, C.c_void_p(stream or 0)))

    def results(self) -> dict:
        """numpy arrays type [C] (int32, -1 = none), best [C, 7] (float64), pos [C, 7] (uint64, input samples), inverted [C, 7] (bool)"""
        out = np.zeros(self.n_channels, DETECTION_DTYPE)
        chk(self.L.sonde_detect_results(self.h, out.ctypes.data_as(C.c_void_p), self.n_channels))
        inv = ((out["inverted"][:, None] >> np.arange(NTYPES, dtype=np.uint32)) & 1).astype(bool)
        return {"type": out["type"].copy(), "best": out["best"].copy(), "pos": out["pos"].copy(), "inverted": inv}

    def reset(self):
        chk(self.L.sonde_detect_reset(self.h))

    def restart_channels(self, channels):
        """the listed channels back to their state after create, ordered on the last submit's stream, no synchronisation
        (sonde_detect_restart_channels)"""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        chk(self.L.sonde_detect_restart_channels(self.h, ch.ctypes.data_as(C.c_void_p), len(ch)))

    def test_shift_age(self, channels, samples):
        """Test introspection, not for hosts (sonde_detect_test_shift_age): the listed channels become the same streams, begun
        samples[i] input samples (a multiple of 30720) earlier; ordered like restart_channels."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        sm = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, dtype=np.uint64), ch.shape))
        chk(self.L.sonde_detect_test_shift_age(self.h, ch.ctypes.data_as(C.c_void_p), len(ch), sm.ctypes.data_as(C.c_void_p)))

    def read(self, channel: int):
        """the last submit's quantised streams of one channel: D [n/2], A_imet [n/8], A_c50 [n/8] (int32)"""
        D = np.zeros(self.max_samples // 2, np.int32)
        ai = np.zeros(self.max_samples // 8, np.int32)
        ac = np.zeros(self.max_samples // 8, np.int32)
        n = chk(self.L.sonde_detect_read(self.h, int(channel), D.ctypes.data_as(C.c_void_p), ai.ctypes.data_as(C.c_void_p),
                                         ac.ctypes.data_as(C.c_void_p)))
        return D[:n // 2], ai[:n // 8], ac[:n // 8]
