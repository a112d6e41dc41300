"""-m gpu: the batch engine's timing path (sonde_batch_set_timing / _kernel_ms / _class_ms) and the stream change of a plain
one-launch batch.  Timing must never change what is decoded: every case compares frames byte for byte with an untimed run."""
import math

import numpy as np
import pytest
import torch

from sdrpp_radiosonde_amd import synth
from sdrpp_radiosonde_amd._lib import FLAG_LATE_JOIN
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
TILE = 2048
RS41, M10, IMET4 = 0, 3, 4


def test_timing_slots_wrap():
    """130 timed submits between two kernel_ms() calls: more than the 128 timing slots the batch holds, so the slots are reused.
    The figures stay finite, the query consumes them, and the frames are those of the untimed run."""
    C, submits = 2, 130
    sb = synth.make_rs41_batch(C, TILE * submits, seed=31, ebn0_db=18.0)
    iq = sb.iq.to("cuda:0")
    tiles = [iq[:, k * TILE:(k + 1) * TILE].contiguous() for k in range(submits)]
    frames = {}
    for every in (1, 0):
        b = SondeBatch(C, TILE)
        b.set_timing(every)
        got = []
        for t in tiles:
            b.submit(t)
            got.append(b.frames())
        frames[every] = np.concatenate(got)
        if every:
            demod_ms, framer_ms = b.kernel_ms()
            assert math.isfinite(demod_ms) and math.isfinite(framer_ms) and demod_ms > 0
            with pytest.raises(SondeError, match="no timed submit"):
                b.kernel_ms()
        b.close()
    assert len(frames[1]) >= 1
    assert frames[1].tobytes() == frames[0].tobytes()


def _class_ms_after_nine_submits(types, flags):
    """9 submits of 8 tiles at the default rule (every eighth submit is timed, and the first): class_ms of the batch"""
    n = TILE * 8
    g = torch.Generator().manual_seed(7)
    x = (0.1 * torch.randn((len(types), n, 2), generator=g)).to("cuda:0")      # which launches are timed does not depend on what they decode
    b = SondeBatch(len(types), n, types=types, flags=flags)
    for _ in range(9):
        b.submit(x)
    b.sync()
    ms = b.class_ms()
    b.close()
    return ms


def test_class_ms_names_the_classes_of_the_launch_units():
    """sonde_batch_class_ms: classes 2 (decimation 4, 8 taps: RS41) and 3 (2, 8: M10) where the batch runs launch units; nothing for
    the one-launch mixed kernel and for a one-class batch; the AFSK tone chain is no class of its own."""
    mixed = [RS41, RS41, M10, M10]
    late = _class_ms_after_nine_submits(mixed, FLAG_LATE_JOIN)
    assert set(late) == {2, 3} and all(v > 0 for v in late.values()), late
    assert _class_ms_after_nine_submits(mixed, 0) == {}
    imet = _class_ms_after_nine_submits(mixed + [IMET4], 0)
    assert set(imet) == {2, 3} and all(v > 0 for v in imet.values()), imet
    assert _class_ms_after_nine_submits([RS41, RS41], 0) == {}


def test_stream_change_of_a_plain_launch():
    """Default flags, one plain launch per submit: consecutive submits on two alternating streams, each buffer written on the
    stream that submits it and the next submit queued before the last one's frames are read.  The library orders the submits
    itself (they share the per-channel state): the frames per submit are those of the same submits on one stream."""
    C, submits, n = 2, 6, TILE * 12
    sb = synth.make_rs41_batch(C, n * submits, seed=37, ebn0_db=18.0)
    host = [sb.iq[:, k * n:(k + 1) * n].contiguous() for k in range(submits)]
    one = SondeBatch(C, n)
    want = []
    for h in host:
        one.submit(h.to("cuda:0"))
        want.append(one.frames())
    assert sum(len(w) for w in want) >= 1
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [torch.empty((C, n, 2), dtype=torch.float32, device="cuda:0") for _ in range(submits)]
    torch.cuda.synchronize()
    two = SondeBatch(C, n)
    assert two.launch_info()["units"] == 1
    two.ticket()                                   # every submit records its own completion from here on
    got = []
    for k in range(submits):
        s = streams[k & 1]
        with torch.cuda.stream(s):
            bufs[k].copy_(host[k], non_blocking=True)
        two.submit(bufs[k], s.cuda_stream)
        if k:
            got.append(two.frames_of(two.ticket() - 1))
    got.append(two.frames())
    assert len(got) == submits
    for k in range(submits):
        assert got[k].tobytes() == want[k].tobytes(), k
