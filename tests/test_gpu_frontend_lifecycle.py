"""Create, destroy and create again for the six front-end objects (VFO, channelizer, tuner, scanner, tracker, detector):
(a) a device that does not exist is refused with the entry point's name in the text and the handle left null;
(b) an object created on memory that an object with dirty carried state has just given back starts from the same state as the
    first one: the same submits give the same outputs, bit for bit;
(c) the channelizer's failures name their entry point in sonde_last_error();
(d) the eight Python wrappers close alike: twice is harmless, the handle is gone, a closed object refuses its calls."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeChannelizer, SondeError, SondeVfo
from sdrpp_radiosonde_amd.combine import SondeCombiner
from sdrpp_radiosonde_amd.detect import SondeDetector
from sdrpp_radiosonde_amd.scan import SondeScanner
from sdrpp_radiosonde_amd.track import SondeTracker
from sdrpp_radiosonde_amd.tuner import SondeTuner

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ---------------------------------------------------------------- (a)
_VFO1 = (_lib.SondeTunerVfo * 1)(_lib.SondeTunerVfo(0, 10_000))
CREATES = {
    "sonde_vfo_create": lambda L, dev, h: L.sonde_vfo_create(2, 20_000, 1000, dev, h),
    "sonde_chan_create": lambda L, dev, h: L.sonde_chan_create(None, 1, dev, h),
    "sonde_tuner_create": lambda L, dev, h: L.sonde_tuner_create(1_000_000, 48_000, 1, _VFO1, 8000, _lib.INPUT_IQ, dev, h),
    "sonde_scan_create": lambda L, dev, h: L.sonde_scan_create(1_000_000, 1024, 1536, _lib.INPUT_IQ, dev, h),
    "sonde_track_create": lambda L, dev, h: L.sonde_track_create(2, 48_000, 2048, 0, 0, _lib.INPUT_IQ, dev, h),
    "sonde_detect_create": lambda L, dev, h: L.sonde_detect_create(2, 2048, _lib.INPUT_IQ, None, dev, h),
}


@pytest.mark.parametrize("name", list(CREATES))
def test_a_device_that_does_not_exist_is_refused(name):
    L = _lib.load()
    h = C.c_void_p()
    assert CREATES[name](L, torch.cuda.device_count(), C.byref(h)) != 0
    text = _lib.last_error()
    assert name in text and "no such HIP device" in text, text
    assert h.value is None


# ---------------------------------------------------------------- (b)
def _noise_and_tone(shape_n, seed, f=0.0137, amp=1.0):
    """[..., n, 2] float32: fixed-seed noise plus a tone: every carried buffer is left dirty"""
    rng = np.random.default_rng(seed)
    n = shape_n[-1]
    ph = 2 * np.pi * f * np.arange(n)
    x = 0.3 * rng.standard_normal(shape_n + (2,)) + amp * np.stack([np.cos(ph), np.sin(ph)], axis=-1)
    return torch.from_numpy(x.astype(np.float32)).to(DEV)


def _vfo():
    x = _noise_and_tone((3, 2, 1000), 1)
    v = SondeVfo(2, 20_000, 1000)
    out = [v.process(x[k]).cpu().numpy() for k in range(3)]
    v.close()
    return out


def _channelizer():
    c = SondeChannelizer(blocks_per_submit=1)
    x = _noise_and_tone((2, c.samples_per_submit), 2, f=0.0123)
    out = []
    for k in range(2):
        c.submit(x[k])
        out.append(c.read()[0])
    out.append(c.frames())
    c.close()
    return out


def _tuner():
    x = _noise_and_tone((3, 8000), 3, f=0.0101)
    t = SondeTuner(1_000_000, 48_000, [(10_000, 10_000)], 8000)
    out = [t.process(x[k]).cpu().numpy() for k in range(3)]
    t.close()
    return out


def _scanner():
    x = _noise_and_tone((3, 1536), 4)
    s = SondeScanner(1_000_000, 1536, fft_size=1024)
    for k in range(3):
        s.submit(x[k])
    out = [s.spectrum()[1], np.array([s.segments])]
    s.close()
    return out


def _tracker():
    x = _noise_and_tone((3, 2, 2048), 5)
    t = SondeTracker(2, 48_000, 2048)
    for k in range(3):
        t.submit(x[k])
    looks, dropped = t.results()
    assert len(looks) == 2                      # 24 blocks of 256: one look of 19 blocks per row
    t.close()
    return [looks, dropped]


def _detector():
    x = _noise_and_tone((3, 2, 2048), 6)
    d = SondeDetector(2, 2048)
    out = []
    for k in range(3):
        d.submit(x[k])
        out += list(d.read(0)) + list(d.read(1))
    r = d.results()
    d.close()
    return out + [r["type"], r["best"], r["pos"], r["inverted"]]


@pytest.mark.parametrize("run", [_vfo, _channelizer, _tuner, _scanner, _tracker, _detector], ids=lambda f: f.__name__[1:])
def test_fresh_state_on_reused_memory(run):
    a = run()
    b = run()
    assert len(a) == len(b) and any(np.asarray(v).view(np.uint8).any() for v in a)
    for va, vb in zip(a, b):
        assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes()


# ---------------------------------------------------------------- (c)
def test_channelizer_failures_name_their_entry_point():
    L = _lib.load()
    assert L.sonde_vfo_ratio(1, None, None) != 0 and "sonde_vfo_ratio" in _lib.last_error()       # what a silent failure would leave behind
    h = C.c_void_p()
    assert L.sonde_chan_create(None, 9, 0, C.byref(h)) != 0 and h.value is None
    assert "sonde_chan_create" in _lib.last_error() and "blocks_per_submit" in _lib.last_error()
    c = SondeChannelizer(blocks_per_submit=1)
    x = torch.zeros((c.samples_per_submit, 2), device=DEV)
    assert L.sonde_vfo_ratio(1, None, None) != 0
    assert L.sonde_chan_submit(c.h, C.c_void_p(x.data_ptr()), c.samples_per_submit - 500, None) != 0
    assert "sonde_chan_submit" in _lib.last_error() and "n_samples" in _lib.last_error()
    c.close()


# ---------------------------------------------------------------- (d)
# the smallest objects their create entries accept (CREATES above) and one call each that needs the handle; what a closed object
# answers was read off the wrappers as they were before they shared a base: the library refuses a null handle, SondeError every time
WRAPPERS = {
    "batch": (lambda: SondeBatch(2, 2048), lambda o: o.sync()),
    "channelizer": (lambda: SondeChannelizer(blocks_per_submit=1), lambda o: o.read()),
    "vfo": (lambda: SondeVfo(2, 20_000, 1000), lambda o: o.process(torch.zeros((2, 1000, 2), device=DEV))),
    "detector": (lambda: SondeDetector(2, 2048), lambda o: o.reset()),
    "tuner": (lambda: SondeTuner(1_000_000, 48_000, [(0, 10_000)], 8000), lambda o: o.retune(0, 1000)),
    "scanner": (lambda: SondeScanner(1_000_000, 1536, fft_size=1024), lambda o: o.reset()),
    "tracker": (lambda: SondeTracker(2, 48_000, 2048), lambda o: o.restart(0)),
    "combiner": (lambda: SondeCombiner(1, 2, 48_000, 256, 256), lambda o: o.restart(0)),
}


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_close_twice_then_drop(name):
    make, call = WRAPPERS[name]
    o = make()
    assert o.h
    call(o)                                     # the call works on a live object
    o.close()
    assert o.h is None
    o.close()
    assert o.h is None
    with pytest.raises(SondeError, match="null argument"):
        call(o)
    o.__del__()                                 # what dropping it runs: nothing left to do, nothing raised
    del o


def test_the_channelizers_borrowed_batch_destroys_nothing():
    c = SondeChannelizer(blocks_per_submit=1)
    x = torch.zeros((c.samples_per_submit, 2), device=DEV)
    c.batch.close()
    assert c.batch.h and c.h
    c.submit(x)
    assert len(c.frames()) == 0
    c.close()
    assert c.h is None and c.batch.h is None
    c.close()
