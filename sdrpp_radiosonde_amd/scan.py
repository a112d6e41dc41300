"""Python face of the band scanner (include/sonde_abi.h, DESIGN SPEC 3.10): thin, no compute -- every call goes through the C ABI of
libsonde_mi355.so.

    SondeScanner    Welch's averaged power spectrum of one wideband stream on the GPU; candidates() lists where the carriers are
    search          the candidate search alone, over any spectrum (pure host, no GPU)
    survey          wideband block -> scanner -> one detection VFO per candidate -> type detector: [(offset_hz, type, cn0, bandwidth)]

The result of survey() with type >= 0 is the `sondes` argument of tuner.WidebandReceiver: from a raw wideband stream to decoded
frames with no outside knowledge of where the sondes are or what they are."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._chain import IQ48_MAX_BW as DETECT_BW          # survey(): the bandwidth of every detection VFO
from ._handle import Handle, chk, current_stream, wideband_block
from ._lib import CANDIDATE_DTYPE, INPUT_IQ, SondeError, SondeScanParams

DETECT_RATE = 48000        # survey(): the rate of the detection rows
MAX_CANDIDATES = 4096


def _params(smooth_hz: int = 0, min_sep_hz: int = 0, centroid_hz: int = 0, threshold: float = 0.0) -> SondeScanParams:
    """0 = the default of SPEC 3.10, each"""
    return SondeScanParams(C.sizeof(SondeScanParams), int(smooth_hz), int(min_sep_hz), int(centroid_hz), float(threshold))


def auto_fft_size(rate_in: int) -> int:
    """the fft_size a scanner created with fft_size=0 takes (sonde_scan_auto_fft_size)"""
    return chk(_lib.load().sonde_scan_auto_fft_size(int(rate_in)))


def window(n: int) -> np.ndarray:
    """the float32 periodic Hann window of n points (sonde_scan_window)"""
    w = np.zeros(int(n), np.float32)
    chk(_lib.load().sonde_scan_window(int(n), w.ctypes.data_as(C.c_void_p), w.size))
    return w


def search(P, rate_in: int, **params) -> np.ndarray:
    """candidates of the spectrum P (float32 [N], ascending frequency) as a structured array (offset_hz, bandwidth_hz, cn0_dbhz,
    excess_db, bin), in ascending bin order (sonde_scan_search: pure host)"""
    P = np.ascontiguousarray(P, dtype=np.float32)
    if P.ndim != 1:
        raise SondeError("the spectrum must be one-dimensional")
    L = _lib.load()
    p = _params(**params)
    out = np.zeros(MAX_CANDIDATES, CANDIDATE_DTYPE)
    n = chk(L.sonde_scan_search(P.ctypes.data_as(C.c_void_p), P.size, int(rate_in), C.byref(p), out.ctypes.data_as(C.c_void_p), out.size))
    return out[:min(n, out.size)].copy()


class SondeScanner(Handle):
    """The averaged power spectrum of one wideband complex stream.  submit() takes a device block [n_in, 2] (float32; int16 for
    INPUT_IQ16, int8 for INPUT_IQ8) of any length 1 .. max_in: the unfinished segment is carried, and the spectrum does not depend
    on how the stream is cut into submits.  All submits of one scanner go on one stream."""
    DESTROY = "sonde_scan_destroy"

    def __init__(self, rate_in: int, max_in: int, *, fft_size: int = 0, input_kind: int = INPUT_IQ, device: int = 0):
        self._create("sonde_scan_create", int(rate_in), int(fft_size), int(max_in), int(input_kind), int(device))
        self.rate_in, self.max_in, self.input_kind, self.device = int(rate_in), int(max_in), int(input_kind), int(device)
        self.fft_size = chk(self.L.sonde_scan_fft_size(self.h))

    def submit(self, block, stream: int | None = None):
        n_in = wideband_block(block, self.input_kind, self.device, "scanner")
        if stream is None:
            stream = current_stream(block.device)
        self._keep = block
        chk(self.L.sonde_scan_submit(self.h, C.c_void_p(block.data_ptr()), n_in, C.c_void_p(stream)))

    def reset(self):
        chk(self.L.sonde_scan_reset(self.h))

    @property
    def segments(self) -> int:
        return chk(self.L.sonde_scan_segments(self.h))

    def spectrum(self):
        """(freqs_hz float64 [N], P float32 [N]) in ascending frequency; raises before the first whole segment"""
        n = self.fft_size
        P = np.zeros(n, np.float32)
        chk(self.L.sonde_scan_spectrum(self.h, P.ctypes.data_as(C.c_void_p), n))
        return (np.arange(n, dtype=np.float64) - n // 2) * (self.rate_in / n), P

    def candidates(self, **params) -> np.ndarray:
        p = _params(**params)
        out = np.zeros(MAX_CANDIDATES, CANDIDATE_DTYPE)
        n = chk(self.L.sonde_scan_candidates(self.h, C.byref(p), out.ctypes.data_as(C.c_void_p), out.size))
        return out[:min(n, out.size)].copy()


def survey(block, rate_in: int, *, input_kind: int = INPUT_IQ, device: int = 0, **params):
    """Where the sondes of a wideband block are and what they are: [(offset_hz, type, cn0_dbhz, bandwidth_hz), ...] in ascending
    offset.  The block is scanned, every candidate gets one 40 kHz detection VFO at 48 kHz in one SondeTuner, and SondeDetector
    decides the rows' types.  type -1: nothing decided (kept, so that the caller can look again later), or the VFO would not lie
    inside the band (not tuned).  Detection runs on the largest part of the block that leaves whole detector tiles at 48 kHz."""
    from .detect import SondeDetector
    from ._chain import plan
    from .tuner import SondeTuner
    n = int(block.shape[0])
    sc = SondeScanner(rate_in, n, input_kind=input_kind, device=device)
    try:
        sc.submit(block)
        cand = sc.candidates(**params)
    finally:
        sc.close()
    types = np.full(len(cand), -1, np.int64)
    fit = [i for i, c in enumerate(cand) if 2 * abs(int(c["offset_hz"])) + DETECT_BW <= int(rate_in)]
    if fit:
        granule = plan(rate_in, ()).granule          # of the iq48 chain with no AFSK sonde: whole detector tiles at DETECT_RATE
        n_use = n // granule * granule
        if not n_use:
            raise SondeError(f"survey() needs at least {granule} samples to detect the candidates' types")
        tu = SondeTuner(rate_in, DETECT_RATE, [(int(cand[i]["offset_hz"]), DETECT_BW) for i in fit], n_use, input_kind=input_kind, device=device)
        det = None
        try:
            rows = tu.process(block[:n_use])
            det = SondeDetector(len(fit), rows.shape[1], device=device)
            det.submit(rows)
            types[fit] = det.results()["type"]
        finally:
            tu.close()
            if det is not None:
                det.close()
    return [(int(c["offset_hz"]), int(t), float(c["cn0_dbhz"]), int(c["bandwidth_hz"])) for c, t in zip(cand, types)]
