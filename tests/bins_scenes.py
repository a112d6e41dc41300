"""The wideband scene and the helpers that test_bins_reference.py (the oracle, on the CPU) and test_gpu_bins_reference.py
(sd_bins_kernel) share: one 10 MS/s stream of 8 blocks, generated on the CPU from fixed seeds, so that what the CPU half establishes
about the block replay (which spans stay unresolved) carries over to the GPU half, which sees the same samples.

Transmitters (synth.make_wideband_scene, one white noise floor, exact carrier offsets):
  all four bin types (RS41, DFM, iMS-100, MRZ-N1), each at Eb/N0 10 and 20 dB;
  carriers at 0, +2 kHz and -4.5 kHz from the bin centre (the last makes the 16-bit phase difference wrap under noise);
  bins 0 and 511; four types in the eight bins 64 .. 71 of one workgroup of the bins kernel, two of them silent (65, 67);
  two transmitters half a bin off (odd bins 100 and 333, for the dual bank).
A second, small scene (late_scene: two blocks, one carrier that comes on the air late) holds the one-sided round of SPEC 3.2."""
from __future__ import annotations

import numpy as np

import demod_reference as D
import fe_reference as F

BLOCK = 1_280_000            # wideband samples per block = 2560 steps = 1536 decimated samples = 3 tiles per bin
STEPS = F.STEPS
NBLK = 8
TILES_PER_BLOCK = 3
SEED = 4242
RS41, DFM, IMS, MRZ = 0, 1, 2, 6

# (bin, carrier offset from the bin centre in Hz, sonde type, Eb/N0 dB)
EVEN_TX = [(0, 0.0, RS41, 20.0), (511, 2000.0, DFM, 10.0),
           (64, -4500.0, RS41, 10.0), (66, 0.0, DFM, 20.0), (68, 2000.0, IMS, 10.0), (70, -4500.0, MRZ, 20.0),
           (130, 2000.0, RS41, 20.0), (200, 0.0, IMS, 20.0), (300, 2000.0, MRZ, 10.0), (400, -4500.0, DFM, 10.0)]
ODD_TX = [(100, 0.0, RS41, 20.0), (333, 2000.0, DFM, 10.0)]          # centred (k + 1/2) bin spacings up: the odd-stacked bank's bins
SILENT = [(65, DFM), (67, MRZ)]                                       # noise only (and what leaks from the neighbours)
WORKGROUP_TYPES = {64: RS41, 65: DFM, 66: DFM, 67: MRZ, 68: IMS, 69: RS41, 70: MRZ, 71: IMS}      # eight bins = one workgroup: four tap slots

_cache: dict = {}


def bin_types(dual: bool = False) -> np.ndarray:
    """the per-bin type array of the mixed runs ([512], or [1024] = even bank | odd bank)"""
    t = np.zeros(1024 if dual else 512, np.uint8)
    for k, _, ty, _ in EVEN_TX:
        t[k] = ty
    for k, ty in WORKGROUP_TYPES.items():
        t[k] = ty
    if dual:
        for k, _, ty, _ in ODD_TX:
            t[512 + k] = ty
    return t


def watched_even():
    """[(bin, type, Eb/N0 or None for a silent bin)] of the even bank"""
    return [(k, ty, e) for k, _, ty, e in EVEN_TX] + [(k, ty, None) for k, ty in SILENT]


def scene() -> np.ndarray:
    """the float32 stream [NBLK * BLOCK, 2]"""
    if "iq" not in _cache:
        from sdrpp_radiosonde_amd import synth
        tx = [(k * F.BIN_HZ + df, ty) for k, df, ty, _ in EVEN_TX] + [((k + 0.5) * F.BIN_HZ + df, ty) for k, df, ty, _ in ODD_TX]
        eb = [e for _, _, _, e in EVEN_TX + ODD_TX]
        iq, _, _ = synth.make_wideband_scene(tx, NBLK * BLOCK, ebn0_db=eb, seed=SEED, cfo_max_hz=0.0)
        _cache["iq"] = iq.numpy()
    return _cache["iq"]


# The late carrier: one stream of two blocks, one RS41 transmitter 4.5 kHz below its bin centre (beyond its deviation: both levels lie
# on one side of 0) that comes on the air 4.8 ms (23 symbols) before the second block, so that the bank's and the filters' memory of the
# noise is gone by then.  Block 1 is the acquisition (SPEC 3.2b: its three tiles set the threshold to the mean of a round, here of
# noise and at the end a few symbols: about 0); the first tile of block 2 is then a ONE-SIDED round (every symbol below the threshold:
# no level estimate, the threshold moves to the round's mean), behind the acquisition boundary and on a state carried over a submit.
# No round of scene() takes that branch of the loop update: a carrier that is there from the start is found by the acquisition rule.
LATE_TX = (130, -4500.0, RS41, 20.0)     # (an RS41 bin of bin_types())
LATE_NBLK = 2
LATE_LEAD = 48_000          # wideband samples


def late_scene() -> np.ndarray:
    """the float32 stream [LATE_NBLK * BLOCK, 2]"""
    if "late" not in _cache:
        from sdrpp_radiosonde_amd import synth
        k, df, ty, e = LATE_TX
        iq, _, _ = synth.make_wideband_scene([(k * F.BIN_HZ + df, ty)], LATE_NBLK * BLOCK, ebn0_db=[e], seed=SEED + 1, cfo_max_hz=0.0,
                                             active=[(BLOCK - LATE_LEAD, LATE_NBLK * BLOCK)])
        _cache["late"] = iq.numpy()
    return _cache["late"]


INT16_SCALE = 200000.0      # the noise floor (sigma 0.02) at 4000 counts: the sum of the carriers stays inside 16 bits, clipped beyond


def scene_int16() -> np.ndarray:
    if "i16" not in _cache:
        _cache["i16"] = np.clip(np.rint(scene().astype(np.float64) * INT16_SCALE), -32767, 32767).astype(np.int16)
    return _cache["i16"]


def to_q16(ph: np.ndarray) -> np.ndarray:
    """phases in quadrants (float32, multiples of 2^-14 in [-2, 2)) -> the 16-bit integers"""
    return np.rint(np.asarray(ph, np.float64) * 16384.0).astype(np.int64)


def hide(states: list, every: int) -> list:
    """keep every `every`-th state, None elsewhere"""
    return [s if (j + 1) % every == 0 else None for j, s in enumerate(states)]


def replay_bin(q: np.ndarray, stype: int, states: list, bits: list, every: int, **kw) -> D.Check:
    """one bin: q = its phases over the whole stream, states / bits = one entry per `every` tiles"""
    d, bd = F.composite_rows(q)
    full = []
    for s in states:
        full += [None] * (every - 1) + [s]
    return D.replay(d, bd, D.modem(stype), full, bits, afc=False, **kw)


def summarise(tag: str, chks: list, ebn0: list, amb_limit: float) -> str:
    """assert what every block-replay test asserts of its watched channels and return the line it prints.  The unresolved cap is a
    condition: at most 5 % of all spans, and no channel more than a quarter of its spans."""
    worst, amb, nbits, spans, unres, cands = {}, 0, 0, 0, 0, 0
    for (name, chk), e in zip(chks, ebn0):
        assert not chk.failures(), chk.line(f"{tag} {name}")
        if e is not None and e >= 10.0:
            assert chk.amb <= amb_limit * chk.nbits, chk.line(f"{tag} {name}")
        assert 4 * chk.unresolved <= chk.spans, chk.line(f"{tag} {name}")
        for k, v in chk.worst.items():
            worst[k] = max(worst.get(k, 0.0), v)
        amb, nbits, spans, unres, cands = amb + chk.amb, nbits + chk.nbits, spans + chk.spans, unres + chk.unresolved, max(cands, chk.cands)
    w = " ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items()))
    line = (f"DEMOD-REF bins {tag}: channels={len(chks)} spans={spans} unresolved={unres} candidates<={cands} bits={nbits} "
            f"ambiguous={amb} ({amb / max(nbits, 1):.2e}) {w}")
    assert 20 * unres <= spans, line
    assert nbits > 0, line
    return line
