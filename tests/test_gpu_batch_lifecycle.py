"""Create, submit, close and create again for the batch object in each of the ways it owns device memory, events and streams, and for
the channelizer's and the detector's members that release themselves: an object created on the memory that one with dirty carried
state has just given back starts from the same state -- the same submits give the same frames, demodulator state and bits, byte for
byte (case (b) of test_gpu_frontend_lifecycle.py, for the objects that test does not reach).  Each variant is the smallest shape
that still uses the members in question; what it uses is said beside it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeChannelizer
from sdrpp_radiosonde_amd.detect import SondeDetector

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RS41, DFM, IMS, M10, IMET, C50 = 0, 1, 2, 3, 4, 5
UNIT_TYPES = [RS41, RS41, M10, M10, DFM, DFM]      # two demod classes, three sonde types: three launch units when not joined per class


def _noise_and_tone(shape_n, seed, f=0.0137, amp=1.0):
    """[..., n, 2] float32 on the host: fixed-seed noise plus a tone: every carried buffer is left dirty"""
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * f * np.arange(shape_n[-1])
    x = 0.3 * rng.standard_normal(shape_n + (2,)) + amp * np.stack([np.cos(ph), np.sin(ph)], axis=-1)
    return x.astype(np.float32)


def _channel_reads(b):
    """sonde_batch_read_state, sonde_batch_nbits and the newest (up to 256) bits of sonde_batch_read_bits, for every channel"""
    out = []
    for c in range(b.n_channels):
        st = b.state(c)
        nb = b.nbits(c)
        out += [np.array([st["t_next"], st["period"]], dtype=np.int64), np.array([st["bias"], st["amp"], st["afc_u"]], dtype=np.float32),
                np.array([nb], dtype=np.uint64), b.read_bits(c, nb - min(nb, 256), min(nb, 256))]
    return out


def _batch(types, n, seed, flags=0, prepare=None, between=None, after=None):
    """two submits of n samples; frames() of each, then the channel reads; prepare(b) before the first submit, between(b) between the
    two, after(b) -> more outputs behind the channel reads"""
    x = torch.from_numpy(_noise_and_tone((2, len(types), n), seed)).to(DEV)
    b = SondeBatch(len(types), n, types=np.array(types, dtype=np.uint8), flags=flags)
    if prepare:
        prepare(b)
    out = []
    for k in range(2):
        b.submit(x[k])
        out.append(b.frames())
        if k == 0 and between:
            between(b)
    out += _channel_reads(b)
    if after:
        out += after(b)
    return b, x, out


def _plain():
    """timing events (set to every submit, read), ev_done and both slot sets (the first submit's frames fetched by ticket after the second)"""
    x = torch.from_numpy(_noise_and_tone((2, 2, 4096), 11)).to(DEV)
    b = SondeBatch(2, 4096)
    b.set_timing(1)
    assert b.ticket() == 0                     # from here on every submit records its completion event
    b.submit(x[0])
    first = b.ticket()
    b.submit(x[1])
    out = [b.frames_of(first), b.frames()]
    ms = b.kernel_ms()
    assert first == 1 and ms[0] > 0.0
    out += _channel_reads(b)
    b.close()
    return out


def _two_classes():
    """the one-launch mixed path: d_cls"""
    b, _, out = _batch([RS41, RS41, M10, M10], 4096, 12)
    assert b.launch_info() == {"units": 1, "join": 0}
    b.close()
    return out


def _late_join():
    """unit streams, ev_join, ev_fork, done_stream"""
    b, _, out = _batch(UNIT_TYPES, 4096, 13, flags=_lib.FLAG_LATE_JOIN)
    assert b.launch_info() == {"units": 3, "join": 1}
    b.close()
    return out


def _pipeline():
    """the same, never joined: closed right behind a third submit, with no sync of the caller's -- destroy alone waits for it"""
    b, x, out = _batch(UNIT_TYPES, 4096, 13, flags=_lib.FLAG_PIPELINE)
    assert b.launch_info() == {"units": 3, "join": 2}
    b.submit(x[0])
    b.close()
    return out


def _afsk():
    """d_astates, d_wtab, d_wtab_c50, d_afq"""
    b, _, out = _batch([IMET, C50, RS41], 16384, 14)
    b.close()
    return out


def _rescue_diversity():
    """d_pass, d_mrztab, the diversity buffers; restart_channels between the submits: the pinned list buffers and ev_restart"""
    types = [RS41, RS41, RS41, DFM, IMS, M10, IMET]
    info = ["rescue_info", "rescue_info", "rescue_info", "dfm_rescue_info", "ims_rescue_info", "manchester_rescue_info", "afsk_rescue_info"]

    def after(b):
        got = [getattr(b, info[c])(c) for c in range(2, len(types))]           # one read per pass
        div = b.diversity_offsets(0)
        return [np.array([[g["tried"], g["rescued"]] for g in got], dtype=np.uint32),
                np.array(div["offsets"] + [div["locked"], div["learned"], div["duplicates"]], dtype=np.int64)]

    b, _, out = _batch(types, 16384, 15, flags=_lib.rescue_flags(True, True, True, True, True),
                       prepare=lambda b: b.set_diversity([[1, 2]], learn=True, mark_duplicates=True), between=lambda b: b.restart_channels([0]), after=after)
    b.close()
    return out


def _submit_host():
    """d_stage"""
    x = _noise_and_tone((2, 2, 4096), 16)
    b = SondeBatch(2, 4096)
    out = []
    for k in range(2):
        b.submit_host(x[k])
        out.append(b.frames())
    out += _channel_reads(b)
    b.close()
    return out


def _channelizer_overlapped():
    """the two streams, the five events and the second phase buffer of the overlapped form, created at its first submit"""
    c = SondeChannelizer(blocks_per_submit=1, fused=True, overlap=True)
    assert c.fused and c.overlap
    x = torch.from_numpy(_noise_and_tone((2, c.samples_per_submit), 17, f=0.0123)).to(DEV)
    out = []
    for k in range(2):
        c.submit(x[k])
        out += [c.frames(), c.read()[0]]
    c.close()
    return out


def _detector_restart():
    """SdChanLists in the detector"""
    x = torch.from_numpy(_noise_and_tone((2, 2, 2048), 18)).to(DEV)
    d = SondeDetector(2, 2048)
    out = []
    for k in range(2):
        d.submit(x[k])
        out += list(d.read(0)) + list(d.read(1))
        if k == 0:
            d.restart_channels([1])
    r = d.results()
    d.close()
    return out + [r["type"], r["best"], r["pos"], r["inverted"]]


VARIANTS = [_plain, _two_classes, _late_join, _pipeline, _afsk, _rescue_diversity, _submit_host, _channelizer_overlapped, _detector_restart]


@pytest.mark.parametrize("run", VARIANTS, ids=lambda f: f.__name__[1:])
def test_fresh_state_on_reused_memory(run):
    a = run()
    b = run()
    assert len(a) == len(b) and any(np.frombuffer(np.asarray(v).tobytes(), dtype=np.uint8).any() for v in a)
    for va, vb in zip(a, b):
        assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes()


def test_create_then_close_without_a_submit():
    SondeBatch(len(UNIT_TYPES), 4096, types=np.array(UNIT_TYPES, dtype=np.uint8), flags=_lib.FLAG_PIPELINE).close()
    SondeChannelizer(blocks_per_submit=1).close()


def test_close_twice():
    b = SondeBatch(2, 4096)
    b.close()
    b.close()
