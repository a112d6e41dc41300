"""Scenes for the SONDE_FLAG_RS41_RESCUE tests: RS41 bit streams with byte errors injected into the on-air bits (as
tests/test_gpu_fec_edges.py does), modulated at 40 dB, so that every record's damage is known exactly.  Shared by the CPU test
of the twin (test_rescue_reference.py) and the GPU tests (test_gpu_rescue.py); each scene and its oracle frames are built once."""
from __future__ import annotations

import functools

import numpy as np

from sdrpp_radiosonde_amd import synth

TILE = 2048
# block offsets of the generator's frames (synth.RS41_SUBFRAMES_STD / _EXT): (offset of the type byte, body length)
STATUS, MEAS, GPSINFO, GPSRAW, GPSPOS = (57, 40), (101, 42), (147, 30), (181, 89), (274, 21)
XDATA = (299, 60)                    # extended frames only
STD_OFFSETS = [57, 101, 147, 181, 274, 299]


def _par(rng, c, k):
    """k distinct parity-byte offsets of codeword c"""
    return [int(o) for o in rng.choice(np.arange(8 + 24 * c, 32 + 24 * c), size=k, replace=False)]


def _case_offsets(case, rng):
    """frame byte offsets a case makes wrong"""
    if case == "meas_burst40":               # 40-byte burst inside the 46-byte measurement block
        return list(range(104, 144))
    if case in ("status_par1", "status_par2"):     # the whole status block wrong + 1 / 2 wrong parity bytes per codeword
        k = 1 if case == "status_par1" else 2
        return list(range(57, 101)) + _par(rng, 0, k) + _par(rng, 1, k)
    if case == "gpsraw_burst30":             # 30-byte burst in the 93-byte GPS-raw block
        return list(range(200, 230))
    if case == "gpsinfo_cw1_13":             # 13 wrong bytes of codeword 1 in the GPS-info block
        return list(range(149, 175, 2))
    if case == "typelen_par8":               # all 12 type / len bytes + eight parity bytes per codeword
        return [o + d for o in STD_OFFSETS for d in (0, 1)] + _par(rng, 0, 8) + _par(rng, 1, 8)
    if case == "gpspos_whole":               # extended: the whole 25-byte GPS-position block
        return list(range(274, 299))
    if case == "xdata_burst30":              # extended: a burst in the 64-byte XDATA block
        return list(range(310, 340))
    raise KeyError(case)


# what the rule must do with each case once the channel has a layout
EXPECT = {"meas_burst40": "rescued", "status_par1": "rescued", "status_par2": "undecodable", "gpsraw_burst30": "too_many",
          "gpsinfo_cw1_13": "rescued", "typelen_par8": "rescued", "gpspos_whole": "rescued", "xdata_burst30": "too_many"}
STD_CASES = ["meas_burst40", "status_par1", "status_par2", "gpsraw_burst30", "gpsinfo_cw1_13", "typelen_par8", None]
EXT_CASES = ["gpspos_whole", "xdata_burst30", None]


def _inject(bits, pos, byte_off, val):
    for b in range(8):
        if (val >> b) & 1:
            bits[pos + 8 * byte_off + b] ^= 1


def cw_of(o):
    return (o - 8) // 24 if o < 56 else (o - 56) & 1


class Scene:
    """iq [C, n, 2] float32 numpy; frames[c] = [(tx bit position, transmitted frame bytes)]; plan[(c, pos)] = (case or None,
    [wrong bytes in codeword 0, in codeword 1]); early[(c, pos)]: damaged before the channel's first clean frame"""


def _build(extended, clean=False):
    C, n = (8, TILE * 150) if extended else (9, TILE * 100)
    flen = 518 if extended else 320
    nbits = int(n * 4800 / 48000) + 16
    bits, frames = synth.rs41_bitstreams(311 + int(extended), np.arange(C), nbits, extended)
    bits = bits.copy()
    rng = np.random.default_rng(17 + int(extended))
    cases = EXT_CASES if extended else STD_CASES
    first_case = cases[0]
    sc = Scene()
    sc.plan, sc.early = {}, set()
    for c in range(C):
        for k, (pos, _) in enumerate(frames[c]):
            case = None
            if not clean:
                if c >= C - 2:                      # these channels start damaged: no layout until frame 2, the same damage later
                    case = first_case if k != 2 else None
                    if k < 2:
                        sc.early.add((c, pos))
                elif k >= 2:
                    case = cases[(c + k) % len(cases)]
            cnt = [0, 0]
            if case:
                for o in _case_offsets(case, rng):
                    _inject(bits[c], pos, o, int(rng.integers(1, 256)))
                    cnt[cw_of(o)] += 1
            sc.plan[(c, pos)] = (case, cnt)
    iq, *_ = synth.gfsk_modulate(bits, n, 4800.0, seed=5, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.frames, sc.flen, sc.C, sc.n, sc.extended = frames, flen, C, n, extended
    return sc


@functools.lru_cache(maxsize=None)
def scene(extended=False, clean=False):
    return _build(extended, clean)


@functools.lru_cache(maxsize=None)
def oracle_frames(extended=False, clean=False):
    """the first pass's records of the scene, from the CPU oracle (read-only: callers copy before they change anything)"""
    import oracle_lib
    oracle_lib.build()
    fr = oracle_lib.batch_run(0, scene(extended, clean).iq, nthreads=4)
    fr.setflags(write=False)
    return fr


def tx_of(sc, f):
    """(tx bit position, transmitted bytes) of the record f"""
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in sc.frames[c]), key=lambda t: t[0])
    assert d < 64, (c, int(f["bitpos"]))
    return pos, tx


def ptu_stream(n_frames=9, first_idx=22, wiped=6, channel=0):
    """One RS41 channel whose frames carry the calibration fragments the PTU conversion needs (3..7: frame numbers 1023..1027) and
    then a frame (index `wiped` of the stream) whose 46-byte measurement block is wholly wrong.  Returns (iq [1, n, 2], n,
    frame number of the wiped frame)."""
    flen, pre = 320, 40
    idx = np.arange(first_idx, first_idx + n_frames)
    fr = synth.rs41_build_frames(5, np.full(n_frames, channel), idx)
    air = synth.bytes_to_bits_lsb(synth.rs41_scramble(fr))
    stride = 8 * (flen + pre)
    lead = 400
    nb = lead + stride * n_frames + 800
    n = -(-(nb * 10) // TILE) * TILE
    bits = (np.arange(n // 10 + 16) & 1).astype(np.uint8)[None, :].copy()
    rng = np.random.default_rng(3)
    for k in range(n_frames):
        pos = lead + k * stride + 8 * pre
        bits[0, pos: pos + 8 * flen] = air[k]
        if k == wiped:
            for o in range(MEAS[0], MEAS[0] + MEAS[1] + 4):
                _inject(bits[0], pos, o, int(rng.integers(1, 256)))
    iq, *_ = synth.gfsk_modulate(bits, n, 4800.0, seed=9, ebn0_db=40.0)
    return (iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)), n, 1000 + first_idx + wiped
