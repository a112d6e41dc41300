"""Scenes for the SONDE_FLAG_MANCHESTER_RESCUE tests (DESIGN SPEC 3.3f): M10, M20 and MRZ-N1 chip streams with single chips flipped
before the modulator (as tests/rescue_scenes.py does for RS41 bits), at 40 dB, so that every record's damage is known exactly.  Shared
by the CPU tests of the twin (test_manchester_rescue_reference.py) and the GPU tests (test_gpu_manchester_rescue.py); each scene and
its oracle records are built once.  No frame is damaged before a channel's first frame.

A case is a list of (frame bit, which chips of its pair to flip): "a" the first chip (the data bit turns and the pair is marked),
"c" the second (the data bit stays and the pair is marked), "ac" both (the data bit turns and NOTHING marks it)."""
from __future__ import annotations

import functools

import numpy as np

from sdrpp_radiosonde_amd import synth

TILE = 2048
M10, MRZN1 = 3, 6
# kind -> (sonde type, m20, channels, tiles, frame bytes, header chips, seed)
KINDS = {"m10": (M10, False, 5, 100, 101, 32, 71), "m20": (M10, True, 2, 100, 70, 32, 72), "mrz": (MRZN1, False, 3, 150, 45, 48, 73)}
EXPECT = {"first1": ("rescued", 1), "second1": ("clean", 0), "mix8": ("rescued", 4), "nine": ("too_many", 0), "hidden2": ("unsolved", 0),
          "in_check": ("rescued", 1), "byte0": ("length_doubtful", 0), "dep4": ("ambiguous", 0), None: ("clean", 0)}
CASES = {"m10": ["first1", "second1", "mix8", "nine", "hidden2", "in_check", "byte0", "dep4", None],
         "m20": ["first1", "second1", "mix8", "nine", "hidden2", "in_check", "byte0", "dep4", None],
         "mrz": ["first1", "mix8", "nine", "hidden2", "in_check", "dep4", "second1", None]}


def _check(kind_type, msg):
    msg = np.asarray(msg, dtype=np.uint8)[None, :]
    return int(synth.m10_checksum(msg, msg.shape[1])[0]) if kind_type == M10 else int(synth.crc16_modbus(msg)[0])


@functools.lru_cache(maxsize=None)
def dependent_four(kind):
    """four covered data bits (none in byte 0) whose columns XOR to zero, as two pairs (a, b), (c, d) with col a ^ col b = col c ^ col d:
    a collision search over the pair XORs of a few hundred columns.  A column = the change of the check when the bit is flipped."""
    typ, _, _, _, ln, _, _ = KINDS[kind]
    zero = np.zeros(ln - 2, dtype=np.uint8)
    base = _check(typ, zero)
    cols = {}
    for k in range(8, min(8 * (ln - 2), 8 + 320)):
        m = zero.copy()
        m[k // 8] = 0x80 >> (k % 8)
        cols[k] = _check(typ, m) ^ base
    seen = {}
    for a in cols:
        for b in cols:
            if b <= a:
                continue
            x = cols[a] ^ cols[b]
            if x in seen and not {a, b} & set(seen[x]):
                return seen[x], (a, b)
            seen.setdefault(x, (a, b))
    raise AssertionError("no dependent four among the columns")


def _case_flips(kind, case, rng):
    typ, _, _, _, ln, _, _ = KINDS[kind]
    data_bits = np.arange(8, 8 * (ln - 2))                     # covered bytes behind byte 0
    pick = lambda n: [int(k) for k in rng.choice(data_bits, size=n, replace=False)]      # noqa: E731
    if case == "first1":
        return [(pick(1)[0], "a")]
    if case == "second1":
        return [(pick(1)[0], "c")]
    if case == "mix8":
        return [(k, "ac"[i & 1]) for i, k in enumerate(sorted(pick(8)))]
    if case == "nine":
        return [(k, "a") for k in pick(9)]
    if case == "hidden2":
        k = pick(3)
        return [(k[0], "ac"), (k[1], "a"), (k[2], "c")]
    if case == "in_check":
        return [(int(rng.integers(8 * (ln - 2), 8 * ln)), "a"), (pick(1)[0], "c")]
    if case == "byte0":
        return [(int(rng.integers(0, 8)), "c"), (pick(1)[0], "a")]
    if case == "dep4":
        (a, b), (c, d) = dependent_four(kind)
        return [(a, "a"), (b, "a"), (c, "c"), (d, "c")]
    raise KeyError(case)


class Scene:
    """iq [C, n, 2] float32 numpy; frames[c] = [(tx chip position of the sync, transmitted frame bytes)]; plan[(c, pos)] = case or None"""


def _build(kind, clean):
    typ, m20, C, tiles, ln, H, seed = KINDS[kind]
    n = TILE * tiles
    baud = synth.SONDE_BAUD[typ]
    nchips = int(n * baud / 48000) + 16
    chips, frames = synth.chip_streams(typ, seed, np.arange(C), nchips, m20=m20)
    chips = chips.copy()
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.plan = {}
    slot = 0
    for c in range(C):
        for k, (pos, _) in enumerate(frames[c]):
            case = None
            if not clean and k >= 1:
                case = CASES[kind][slot % len(CASES[kind])]
                slot += 1
            if case:
                for bit, which in _case_flips(kind, case, rng):
                    for w in which:
                        chips[c, pos + H + 2 * bit + (w == "c")] ^= 1
            sc.plan[(c, pos)] = case
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=seed, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.frames, sc.kind, sc.type, sc.len, sc.C, sc.n = frames, kind, typ, ln, C, n
    return sc


@functools.lru_cache(maxsize=None)
def scene(kind, clean=False):
    return _build(kind, clean)


# ---- the noisy scene: M10 at Eb/N0 10 dB.  The seed was picked on the CPU among the first few: over the oracle's records and chips the twin
# rescues 30 frames or more and every rescued frame is a transmitted one (seeds with a wrongly rescued frame exist too: DESIGN 3.3f
# "false accepts"; this is one with none, so that the test can assert it).
NOISY = dict(channels=8, tiles=100, ebn0_db=10.0, seed=3)


@functools.lru_cache(maxsize=None)
def noisy_scene():
    sb = synth.make_batch(M10, NOISY["channels"], TILE * NOISY["tiles"], seed=NOISY["seed"], ebn0_db=NOISY["ebn0_db"])
    sc = Scene()
    sc.iq = sb.iq.numpy()
    sc.frames, sc.kind, sc.type, sc.len, sc.C, sc.n, sc.plan = sb.frames, "noisy", M10, 101, NOISY["channels"], TILE * NOISY["tiles"], {}
    return sc


def _scene_of(kind, clean=False):
    return noisy_scene() if kind == "noisy" else scene(kind, clean)


@functools.lru_cache(maxsize=None)
def oracle_run(kind, clean=False):
    """(records in (channel, time) order, [chip stream of each channel]) of the scene from the CPU oracle (read-only)"""
    import oracle_lib
    oracle_lib.build()
    sc = _scene_of(kind, clean)
    recs, streams = [], []
    for c in range(sc.C):
        ch = oracle_lib.Channel(sc.type, c)
        ch.feed(sc.iq[c])
        recs.append(ch.frames())
        bits = ch.bits()
        bits.setflags(write=False)
        streams.append(bits)
    fr = np.concatenate(recs)
    fr.setflags(write=False)
    return fr, streams


def tx_of(sc, f):
    """(tx chip position, transmitted bytes) of the record f; None: no transmitted frame there (a false sync)"""
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in sc.frames[c]), key=lambda t: t[0])
    return (pos, tx) if d < 64 else None
