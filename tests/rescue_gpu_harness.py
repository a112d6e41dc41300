"""What the -m gpu test files of the five rescue passes (test_gpu_rescue.py, test_gpu_manchester_rescue.py, test_gpu_dfm_rescue.py,
test_gpu_ims_rescue.py, test_gpu_afsk_rescue.py) share: a scene through a batch in `cuts` submits, its records in (channel, bitpos)
order, a chips getter over the batch's bit rings for the twins, and the counters of a pass against the twin's state.  Each file binds
its own tile, default sonde type, info method and new_state with functools.partial."""
import numpy as np

from sdrpp_radiosonde_amd.batch import SondeBatch


def sorted_frames(parts):
    fr = np.concatenate(parts)
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


def run(iq, flags, cuts=1, via_ticket=False, keep=False, *, tile, default_type=None, after_submit=None, **kw):
    """iq through a batch in `cuts` equal submits (each a multiple of `tile`); default_type: the sonde type of every channel unless
    types= says otherwise (None: the batch's default, RS41); after_submit(b, k): called behind submit k's frames (the stream-age
    tests shift the batch there)"""
    C_, n = iq.shape[0], iq.shape[1]
    assert n % (cuts * tile) == 0
    step = n // cuts
    if default_type is not None:
        kw.setdefault("types", np.full(C_, default_type, dtype=np.uint8))
    b = SondeBatch(C_, step, flags=flags, **kw)
    parts = []
    for k in range(cuts):
        b.submit(iq[:, k * step:(k + 1) * step])
        parts.append(b.frames_of(b.ticket()) if via_ticket else b.frames())
        if after_submit is not None:
            after_submit(b, k)
    out = sorted_frames(parts)
    if keep:
        return out, b
    b.close()
    return out


def gpu_chips(b):
    """a chips getter over the batch's bit rings (the whole stream is still there after ONE submit: the ring holds a submit and a frame)"""
    def get(channel, start, count):
        return b.read_bits(channel, start, count)
    return get


def check_info(b, state, channels, *, method, new_state):
    for c in channels:
        st = state.get(c, new_state())
        assert getattr(b, method)(c) == st, (c, st)
