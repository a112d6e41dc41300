"""The receive chain under WidebandReceiver, DiversityReceiver and LiveReceiver (private): wideband stream -> tuner(s) -> 48 kHz
rows -> SondeBatch.  What the three share is here, once: the block arithmetic (plan), the VFO bandwidth of the iq48 chain, the
batch and its input rows, the block check and the tracking loop of SPEC 3.11.  Nothing here computes on the samples."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._handle import chk
from ._lib import C50, IMET4, INPUT_IQ, TILE, SondeError
from .batch import VFO_RATE, SondeBatch

AFSK_TILE = 16384          # a batch with an AFSK sonde (iMet-4, SRS-C50) takes rows in multiples of this
IQ48_MAX_BW = 40000        # the iq48 chain's VFO bandwidth cap (M10 / M20: 50 kHz does not fit a 48 kHz row); every probe and detection VFO


def iq48_bandwidth(t: int) -> int:
    """the bandwidth of a sonde type's VFO in the iq48 chain"""
    return min(VFO_RATE[t], IQ48_MAX_BW)


def ratio(rate_in: int, rate_out: int) -> tuple[int, int]:
    """(up, down) = rate_out / rate_in in lowest terms (sonde_tuner_ratio; raises for rates the tuner refuses)"""
    up, down = C.c_int(), C.c_int()
    chk(_lib.load().sonde_tuner_ratio(int(rate_in), int(rate_out), C.byref(up), C.byref(down)))
    return up.value, down.value


def vfo_down(rate: int) -> int:
    down = C.c_int()
    chk(_lib.load().sonde_vfo_ratio(int(rate), None, C.byref(down)))
    return down.value


def multiple_for(a: int, b: int, c: int) -> int:
    """the smallest n > 0 with n * a / b a multiple of c (a / b in lowest terms or not)"""
    g = math.gcd(a, b)
    a, b = a // g, b // g
    return c * b // math.gcd(a, c * b)


def lcm(*v: int) -> int:
    out = 1
    for x in v:
        out = out * x // math.gcd(out, x)
    return out


def out48(rate_in: int, n: int) -> int:
    """the 48 kHz samples of n input samples (n a multiple of the granule: exact)"""
    return n * 48000 // rate_in


@dataclass(frozen=True)
class Plan:
    tile: int          # the batch's row unit at 48 kHz
    granule: int       # the smallest block that leaves whole tiles (and whole steps of every stage) at 48 kHz
    max_in: int        # the largest block, a multiple of the granule
    n48: int           # its samples at 48 kHz
    groups: dict       # tuner rate -> indices into `types`: {48000: all} for iq48, one group per distinct VFO_RATE for reference


def plan(rate_in: int, types, max_in: int | None = None, chain: str = "iq48", track: bool = False) -> Plan:
    """The block arithmetic of a receiver for these sonde types (max_in None / 0: one granule).  chain="reference" adds every VFO
    rate's tuner and resampler steps to the granule, and with track=True whole 256-sample meter blocks at every VFO rate."""
    types = list(types)
    fs = int(rate_in)
    tile = AFSK_TILE if any(t in (IMET4, C50) for t in types) else TILE
    if chain == "iq48":
        groups = {48000: list(range(len(types)))}
        parts = [ratio(fs, 48000)[1], multiple_for(48000, fs, tile)]
    else:
        groups = {}
        for i, t in enumerate(types):
            groups.setdefault(VFO_RATE[t], []).append(i)
        parts = [multiple_for(48000, fs, tile)]
        for b in groups:
            parts += [ratio(fs, b)[1], multiple_for(b, fs, vfo_down(b))]
            if track:
                parts.append(multiple_for(b, fs, 256))
    granule = lcm(*parts)
    max_in = int(max_in or granule)
    if max_in % granule:
        raise SondeError(f"max_in must be a multiple of the granule ({granule})")
    return Plan(tile, granule, max_in, out48(fs, max_in), groups)


def check_block(n: int, granule: int, max_in: int, noun: str = "block"):
    if n == 0 or n % granule or n > max_in:
        raise SondeError(f"the {noun} must hold a positive multiple of the granule ({granule}) samples, at most max_in ({max_in})")


def batch(n_channels: int, n48: int, types, device: int, rescue, input_kind: int = INPUT_IQ, flags: int = 0) -> SondeBatch:
    """the decoders of a chain; rescue: the receiver's five rescue keywords in _lib.rescue_flags' order; flags: further create flags"""
    return SondeBatch(n_channels, n48, types=np.asarray(types, dtype=np.uint8), input_kind=input_kind, device=device,
                      flags=_lib.rescue_flags(*rescue) | int(flags))


def rows(n_rows: int, n48: int, device: int, input_kind: int = INPUT_IQ):
    """the buffer the tuners write and the batch reads: n_rows float32 rows of n48 samples, the library's row stride apart"""
    import torch
    stride = int(_lib.load().sonde_row_stride(n48, input_kind))
    return torch.empty((n_rows, stride, 2) if input_kind == INPUT_IQ else (n_rows, stride), dtype=torch.float32, device=f"cuda:{device}")


def track_looks(tracker, tuner, rate_in: int, params: dict, skip=None):
    """The loop of SPEC 3.11 over one meter and the tuner whose rows it sees: the newest look of every row that `skip` does not
    leave out -> (row, the VFO's next offset by track.step, err_hz, level_db).  The caller retunes and logs before the next look
    is stepped."""
    from . import track as tk
    looks, _ = tracker.results()
    newest = {}
    for lk in looks:
        newest[int(lk["row"])] = lk           # rows come oldest look first
    for k, lk in newest.items():
        if skip is not None and skip(k):
            continue
        new = tk.step(tuner.offsets[k], tuner.bandwidths[k], rate_in, tracker.rate, tracker.lag, lk["a_re"], lk["a_im"], params)
        yield k, new, tk.err_hz(tracker.rate, tracker.lag, lk["a_re"], lk["a_im"]), tk.level_db(lk["p"], tracker.look_samples)
