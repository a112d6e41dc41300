"""Scenes for the SONDE_FLAG_DFM_RESCUE tests (DESIGN SPEC 3.3g): DFM chip streams with single chips flipped before the modulator (as
tests/manchester_rescue_scenes.py does), at 40 dB, so that every record's damage is known exactly.  Shared by the CPU tests of the twin
(test_dfm_rescue_reference.py) and the GPU tests (test_gpu_dfm_rescue.py); each scene and its oracle records are built once.  No
frame is damaged before a channel's first frame.  The last channel of the designed scene has Q negated: its records carry inverted
polarity (flags bit 0).

A case is a list of (codeword, bit of it, which chips of the bit's pair to flip): "a" the first chip (the data bit turns and the pair is
marked), "c" the second (the data bit stays and the pair is marked), "ac" both (the data bit turns and NOTHING marks it).  Every
case is placed, in turn, in a word of each of the three interleaved blocks (words 0-6, 7-19, 20-32).

`aa_ac` (two marked wrong bits and an unmarked one) is THREE wrong bits, like `aaa`: the first pass takes the word for a single error
and miscorrects it, the record says nerr[1] = 0 and the pass never sees it.  The damage that does reach the decoder with e = 2 and
v = 1 has an even number of wrong bits: `a_c_ac`, one marked wrong bit, one marked right bit and one unmarked wrong bit."""
from __future__ import annotations

import functools

import numpy as np

from sdrpp_radiosonde_amd import synth

TILE = 2048
DFM = 1
BLOCKS = ((0, 7), (7, 13), (20, 13))            # (first codeword, codewords) of the three interleaved blocks (synth.dfm_build_frames)
# case -> (outcome, words decoded by the pass, the record's data is the transmitted frame)
EXPECT = {"aa": ("rescued", 1, True), "a_ac": ("rescued", 1, True), "aac": ("rescued", 1, True), "two_words": ("rescued", 2, True),
          "ac_ac": ("unsolved", 0, False), "aacc": ("unsolved", 0, False), "a_c_ac": ("unsolved", 0, False), "one_bad_of_two": ("unsolved", 0, False),
          "aa_ac": ("clean", 0, False), "a": ("clean", 0, True), "aaa": ("clean", 0, False), "nine": ("too_many", 0, False), None: ("clean", 0, True)}
CASES = ["aa", "a_ac", "aac", "two_words", "ac_ac", "aacc", "a_c_ac", "aa_ac", "one_bad_of_two", "a", "aaa", "nine", None]
DESIGNED = dict(channels=4, tiles=100, seed=81, inverted=(3,))
LONG = dict(channels=1, tiles=200, seed=82, inverted=())


def chip_of(i, j):
    """the chip offset, from the first sync chip, of the first chip of bit j (0 = MSB) of codeword i"""
    for first, n in BLOCKS:
        if first <= i < first + n:
            return 32 + 2 * (8 * first + j * n + (i - first))
    raise IndexError(i)


def block_of(i):
    return 0 if i < 7 else (1 if i < 20 else 2)


def _case_flips(case, blk, rng):
    first, n = BLOCKS[blk]
    w0 = int(first + rng.integers(0, n))
    others = [int(w) for w in rng.permutation([w for w in range(33) if w != w0])]
    bits = lambda k: [int(b) for b in rng.choice(8, size=k, replace=False)]      # noqa: E731
    word = lambda w, kinds: [(w, j, kind) for j, kind in zip(bits(len(kinds)), kinds)]      # noqa: E731
    one = {"aa": ["a", "a"], "a_ac": ["a", "ac"], "aac": ["a", "a", "c"], "ac_ac": ["ac", "ac"], "aacc": ["a", "a", "c", "c"],
           "a_c_ac": ["a", "c", "ac"], "aa_ac": ["a", "a", "ac"], "a": ["a"], "aaa": ["a", "a", "a"]}
    if case in one:
        return word(w0, one[case])
    if case == "two_words":
        return word(w0, ["a", "a"]) + word(others[0], ["a", "a"])
    if case == "one_bad_of_two":
        return word(w0, ["a", "a"]) + word(others[0], ["ac", "ac"])
    if case == "nine":
        return [t for w in [w0] + others[:8] for t in word(w, ["a", "a"])]
    raise KeyError(case)


class Scene:
    """iq [C, n, 2] float32 numpy; frames[c] = [(tx chip position of the sync, transmitted codewords)]; plan[(c, pos)] = (case, block)"""


def _build(name, clean):
    par = LONG if name == "long" else DESIGNED
    C, tiles, seed = par["channels"], par["tiles"], par["seed"]
    n = TILE * tiles
    baud = synth.SONDE_BAUD[DFM]
    nchips = int(n * baud / 48000) + 16
    chips, frames = synth.chip_streams(DFM, seed, np.arange(C), nchips)
    chips = chips.copy()
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.plan = {}
    slot = 0
    seen = {}
    for c in range(C):
        for k, (pos, _) in enumerate(frames[c]):
            case, blk = None, 0
            if name == "long":
                if not clean and 60 <= k <= 70:
                    case, blk = ("aa", "ac_ac")[k & 1], k % 3
            elif not clean and k >= 1:
                case = CASES[slot % len(CASES)]
                slot += 1
                blk = seen.get(case, 0) % 3
                seen[case] = seen.get(case, 0) + 1
            if case:
                for w, j, which in _case_flips(case, blk, rng):
                    for x in which:
                        chips[c, pos + chip_of(w, j) + (x == "c")] ^= 1
            sc.plan[(c, pos)] = (case, blk)
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=seed, ebn0_db=40.0)
    sc.iq = (iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)).copy()
    for c in par["inverted"]:
        sc.iq[c, :, 1] *= -1.0
    sc.frames, sc.kind, sc.type, sc.len, sc.C, sc.n, sc.inverted = frames, name, DFM, 33, C, n, tuple(par["inverted"])
    return sc


@functools.lru_cache(maxsize=None)
def scene(name="designed", clean=False):
    return _build(name, clean)


# ---- the noisy scene: DFM at Eb/N0 9 dB.  Over the oracle's records and chips 22 records have a failed word (20 with one, 2 with two),
# the twin rescues all 22 and every one is the transmitted frame; the same with Q negated.
NOISY = dict(channels=8, tiles=100, ebn0_db=9.0, seed=5)


@functools.lru_cache(maxsize=None)
def noisy_scene(negate_q=False):
    sb = synth.make_batch(DFM, NOISY["channels"], TILE * NOISY["tiles"], seed=NOISY["seed"], ebn0_db=NOISY["ebn0_db"])
    sc = Scene()
    sc.iq = sb.iq.numpy().copy()
    if negate_q:
        sc.iq[:, :, 1] *= -1.0
    sc.frames, sc.kind, sc.type, sc.len, sc.C, sc.n, sc.plan = sb.frames, "noisy", DFM, 33, NOISY["channels"], TILE * NOISY["tiles"], {}
    sc.inverted = tuple(range(sc.C)) if negate_q else ()
    return sc


def scene_of(name, clean=False):
    if name == "noisy":
        return noisy_scene()
    if name == "noisy_negq":
        return noisy_scene(True)
    return scene(name, clean)


@functools.lru_cache(maxsize=None)
def oracle_run(name, clean=False):
    """(records in (channel, time) order, [chip stream of each channel]) of the scene from the CPU oracle (read-only)"""
    import oracle_lib
    oracle_lib.build()
    sc = scene_of(name, clean)
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
    """(tx chip position, transmitted codewords) of the record f; None: no transmitted frame there (a false sync)"""
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in sc.frames[c]), key=lambda t: t[0])
    return (pos, tx) if d < 64 else None
