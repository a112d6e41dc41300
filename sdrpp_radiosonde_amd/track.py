"""Python face of the carrier meter and the tracking step (include/sonde_abi.h, DESIGN SPEC 3.11): thin, no compute -- every call
goes through the C ABI of libsonde_mi355.so.

    SondeTracker        per row of complex samples (the tuner's rows) and per look of about 0.1 s: A = sum x[m] conj(x[m - lag]) and
                        P = sum |x[m]|^2 on the GPU; err_hz / level_db / quality of a look on the host
    step()              the loop's rule (sonde_track_step): one look -> the VFO's next offset

WidebandReceiver(track=True) (tuner.py) is the loop built from the two and SondeTuner.retune(continuous=True)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import INPUT_IQ, LOOK_DTYPE, TRACK_DEADBAND_HZ, TRACK_MAX_STEP_HZ
from ._handle import Handle, chk, complex_rows, current_stream


def defaults(rate: int) -> tuple[int, int]:
    """(look_samples, lag) the meter picks for rows at `rate` (sonde_track_defaults)"""
    a, b = C.c_uint32(), C.c_uint32()
    chk(_lib.load().sonde_track_defaults(int(rate), C.byref(a), C.byref(b)))
    return a.value, b.value


def err_hz(rate: int, lag: int, a_re: float, a_im: float) -> float:
    return float(_lib.load().sonde_track_err_hz(int(rate), int(lag), float(a_re), float(a_im)))


def level_db(p: float, look_samples: int) -> float:
    return float(_lib.load().sonde_track_level_db(float(p), int(look_samples)))


def quality(a_re: float, a_im: float, p: float) -> float:
    return float(_lib.load().sonde_track_quality(float(a_re), float(a_im), float(p)))


def _params(params):
    if params is None:
        return None
    p = _lib.SondeTrackParams()
    p.struct_size = C.sizeof(p)
    p.deadband_hz = int(params.get("deadband_hz", 0))
    p.max_step_hz = int(params.get("max_step_hz", 0))
    return C.byref(p)


def step(offset_hz: int, bandwidth_hz: int, rate_in: int, rate: int, lag: int, a_re: float, a_im: float, params: dict | None = None) -> int:
    """the VFO's next offset from one look (sonde_track_step); params: {"deadband_hz": .., "max_step_hz": ..} (0 / absent = default)"""
    look = _lib.SondeTrackLook()
    look.a_re, look.a_im = float(a_re), float(a_im)
    new = C.c_int32()
    chk(_lib.load().sonde_track_step(int(offset_hz), int(bandwidth_hz), int(rate_in), int(rate), int(lag), C.byref(look), _params(params),
                                     C.byref(new)))
    return new.value


class SondeTracker(Handle):
    """The carrier meter over n_rows complex64 rows at `rate`.  submit() takes a float32 device view [n_rows, n, 2] (rows any stride
    apart, contiguous inside a row), n a positive multiple of 256 and <= max_samples; results() synchronises and returns the looks
    finished since the last call (LOOK_DTYPE: row, look, a_re, a_im, p) and how many older ones each row dropped."""
    DESTROY = "sonde_track_destroy"

    def __init__(self, n_rows: int, rate: int, max_samples: int, *, look_samples: int = 0, lag: int = 0, input_kind: int = INPUT_IQ,
                 device: int = 0):
        self._create("sonde_track_create", int(n_rows), int(rate), int(max_samples), int(look_samples), int(lag), int(input_kind), int(device))
        h = self.h
        self.n_rows, self.rate, self.max_samples, self.device = int(n_rows), int(rate), int(max_samples), int(device)
        self.look_samples = int(self.L.sonde_track_look_samples(h))
        self.lag = int(self.L.sonde_track_lag(h))
        self.ring = int(self.L.sonde_track_ring(h))

    def submit(self, rows, stream: int | None = None):
        n, stride = complex_rows(rows, self.n_rows, self.device, "meter", "n_rows", self.n_rows, "carrier")
        if stream is None:
            stream = current_stream(rows.device)
        self._keep = rows
        chk(self.L.sonde_track_submit(self.h, C.c_void_p(rows.data_ptr()), n, stride, C.c_void_p(stream)))

    def restart(self, row: int):
        """drop the row's unfinished look and lag history: its next look starts at the next submit's first sample"""
        chk(self.L.sonde_track_restart(self.h, int(row)))

    def results(self):
        out = np.zeros(self.n_rows * self.ring, dtype=LOOK_DTYPE)
        dropped = np.zeros(self.n_rows, dtype=np.uint64)
        n = chk(self.L.sonde_track_results(self.h, out.ctypes.data_as(C.c_void_p), len(out), dropped.ctypes.data_as(C.c_void_p)))
        return out[:n], dropped

    def err_hz(self, looks) -> np.ndarray:
        return np.array([err_hz(self.rate, self.lag, k["a_re"], k["a_im"]) for k in looks])

    def level_db(self, looks) -> np.ndarray:
        return np.array([level_db(k["p"], self.look_samples) for k in looks])

    def quality(self, looks) -> np.ndarray:
        return np.array([quality(k["a_re"], k["a_im"], k["p"]) for k in looks])
