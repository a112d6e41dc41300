"""-m gpu: DFM09 / M10 / iMS-100 framers + FEC and mixed per-channel dispatch (BASELINE config 3)
against the CPU oracle, bit-exact, through the C ABI."""
import numpy as np
import pytest
import torch

from sdrpp_radiosonde_amd import synth
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu
TILE = 2048
NAMES = {0: "RS41", 1: "DFM09", 2: "iMS100", 3: "M10", 6: "MRZ-N1"}


@pytest.mark.parametrize("stype", [1, 3, 2, 6])
@pytest.mark.parametrize("noisy", [False, True])
def test_single_type_bit_exact(oracle, stype, noisy):
    ebn0 = {1: 10.0, 2: 10.5, 3: 12.5, 6: 11.0}[stype] if noisy else 30.0
    C, n = 12, TILE * (72 if stype == 6 else 40)          # MRZ-N1 sends one frame per second
    sb = synth.make_batch(stype, C, n, seed=40 + stype, ebn0_db=ebn0, invert=(stype == 1 and ebn0 < 20))
    b = SondeBatch(C, n, types=np.full(C, stype, dtype=np.uint8))
    b.submit(sb.iq.to("cuda:0"))
    got = b.frames()
    ref = oracle.batch_run(stype, sb.iq.numpy(), nthreads=4)
    assert len(ref) >= C, NAMES[stype]
    assert got.tobytes() == ref.tobytes(), NAMES[stype]
    for c in range(C):
        ch = oracle.Channel(stype, c)
        ch.feed(sb.iq.numpy()[c])
        nb = len(ch.bits())
        assert b.nbits(c) == nb and np.array_equal(b.read_bits(c, 0, nb), ch.bits())
    if ebn0 > 20:
        sent = sum(len(f) for f in sb.frames)
        exact = sum(any(np.array_equal(tx, f["data"][: f["len"]]) for _, tx in sb.frames[f["channel"]]) for f in got)
        assert exact >= sent - C          # at most the first (acquisition) frame per channel may be lost
    else:
        assert (got["nerr"] != 0).any()   # the FEC / checks are exercised


def test_mixed_types_per_channel_dispatch(oracle):
    """BASELINE config 3 in miniature: type = (RS41, M10, DFM09)[channel % 3], one batch, one submit."""
    C, n = 18, TILE * 48
    types = np.array([(0, 3, 1)[c % 3] for c in range(C)], dtype=np.uint8)
    iq = torch.empty((C, n, 2), dtype=torch.float32)
    refs = []
    for t in (0, 3, 1):
        idx = np.nonzero(types == t)[0]
        sb = synth.make_batch(int(t), len(idx), n, seed=70 + int(t), ebn0_db=17.0)
        iq[idx] = sb.iq
        r = oracle.batch_run(int(t), sb.iq.numpy(), nthreads=4)
        r["channel"] = idx[r["channel"]]
        refs.append(r)
    ref = np.concatenate(refs)
    ref = ref[np.lexsort((ref["bitpos"], ref["channel"]))]
    b = SondeBatch(C, n, types=types)
    b.submit(iq.to("cuda:0"))
    got = b.frames()
    assert len(ref) >= C and got.tobytes() == ref.tobytes()
    assert set(got["type"].tolist()) == {0, 1, 3}
    # streaming in two unequal submits gives the same frames
    b2 = SondeBatch(C, TILE * 30, types=types)
    parts = []
    for lo, hi in ((0, TILE * 18), (TILE * 18, n)):
        b2.submit(iq[:, lo:hi].contiguous().to("cuda:0"))
        parts.append(b2.frames())
    got2 = np.concatenate(parts)
    got2 = got2[np.lexsort((got2["bitpos"], got2["channel"]))]
    assert got2.tobytes() == ref.tobytes()


def test_m20_frames_bit_exact(oracle):
    """M20 (the reference lists the type as "M10/M20" in its table of sonde types, main.hpp): 70-byte frames through the same framer; the length byte
    selects where the checksum sits.  GPU records == oracle records, and equal to what was transmitted."""
    C, n = 8, TILE * 40
    sb = synth.make_batch(3, C, n, seed=47, ebn0_db=28.0, m20=True)
    b = SondeBatch(C, n, types=np.full(C, 3, dtype=np.uint8))
    b.submit(sb.iq.to("cuda:0"))
    got = b.frames()
    ref = oracle.batch_run(3, sb.iq.numpy(), nthreads=4)
    assert len(ref) >= C and got.tobytes() == ref.tobytes()
    assert (got["len"] == 70).all() and (got["nerr"][:, 0] == 0).sum() >= len(got) - C
    sent = sum(len(f) for f in sb.frames)
    exact = sum(any(np.array_equal(tx[:70], f["data"][:70]) for _, tx in sb.frames[f["channel"]]) for f in got)
    assert exact >= sent - C


def test_split_framers_equal_in_kernel_sync(oracle):
    """SONDE_FLAG_SPLIT_FEC: sync search and decode as kernels of their own (the round-1 structure) give the same frame
    records as the default (sync search inside the demod kernel) for DFM / iMS-100 / M10, over two submits."""
    from sdrpp_radiosonde_amd._lib import FLAG_SPLIT_FEC
    C, n = 9, TILE * 48
    types = np.array([(1, 2, 3)[c % 3] for c in range(C)], dtype=np.uint8)
    iq = torch.empty((C, n, 2), dtype=torch.float32)
    for t in (1, 2, 3):
        idx = np.nonzero(types == t)[0]
        iq[idx] = synth.make_batch(int(t), len(idx), n, seed=60 + int(t), ebn0_db=16.0).iq
    dev = iq.to("cuda:0")
    outs = []
    for flags in (0, FLAG_SPLIT_FEC):
        b = SondeBatch(C, n // 2, types=types, flags=flags)
        parts = []
        for lo in (0, n // 2):
            b.submit(dev[:, lo: lo + n // 2].contiguous())
            parts.append(b.frames())
        g = np.concatenate(parts)
        outs.append(g[np.lexsort((g["bitpos"], g["channel"]))])
    assert len(outs[0]) >= 2 * C and outs[0].tobytes() == outs[1].tobytes()


def test_pipelined_mixed_batch_equals_joined(oracle):
    """SONDE_FLAG_PIPELINE: every sonde type's kernels keep their own stream from submit to submit and are never joined into
    the caller's stream; three submits queued back to back, frames fetched per ticket afterwards (the last two) and per
    submit (a second run): the same records as the default (joined) batch, which equal the oracle's."""
    from sdrpp_radiosonde_amd._lib import FLAG_PIPELINE
    C, n, parts = 16, TILE * 24 * 3, 3          # RS41, M10, DFM, iMS-100 + one iMet and one C50 channel (AFSK units: 16384-sample granule)
    types = np.array([(0, 3, 1, 2)[c % 4] for c in range(C)], dtype=np.uint8)
    types[4], types[9] = 4, 5
    iq = torch.empty((C, n, 2), dtype=torch.float32)
    for t in sorted(set(types.tolist())):
        idx = np.nonzero(types == t)[0]
        iq[idx] = synth.make_batch(int(t), len(idx), n, seed=90 + int(t), ebn0_db=15.0).iq
    dev = iq.to("cuda:0")
    chunks = [dev[:, p * (n // parts): (p + 1) * (n // parts)].contiguous() for p in range(parts)]
    key = lambda a: a[np.lexsort((a["bitpos"], a["channel"]))]
    outs = {}
    for flags in (0, FLAG_PIPELINE):
        b = SondeBatch(C, n // parts, types=types, flags=flags)
        fr = []
        for ch in chunks:
            b.submit(ch)
            fr.append(b.frames())
        outs[flags] = key(np.concatenate(fr))
        b.close()
    assert len(outs[0]) >= C and outs[0].tobytes() == outs[FLAG_PIPELINE].tobytes()
    # queued back to back: tickets
    b = SondeBatch(C, n // parts, types=types, flags=FLAG_PIPELINE)
    b.ticket()
    b.submit(chunks[0]); t1 = b.ticket()
    b.submit(chunks[1]); t2 = b.ticket()
    f1 = b.frames_of(t1)
    b.submit(chunks[2]); t3 = b.ticket()
    f2, f3 = b.frames_of(t2), b.frames_of(t3)
    assert key(np.concatenate([f1, f2, f3])).tobytes() == outs[0].tobytes()
    # and the joined result is the oracle's
    refs = []
    for t in sorted(set(types.tolist())):
        idx = np.nonzero(types == t)[0]
        r = oracle.batch_run(int(t), iq[idx].numpy(), nthreads=4, cap_per_channel=4096 if t in (4, 5) else 0)     # C50: 9-byte packets
        r["channel"] = idx[r["channel"]]
        refs.append(r)
    assert key(np.concatenate(refs)).tobytes() == outs[0].tobytes()
