"""Scenes for the SONDE_FLAG_IMS_RESCUE tests (DESIGN SPEC 3.3h): iMS-100 chip streams with single chips flipped before the modulator (as
tests/dfm_rescue_scenes.py does), at 40 dB, so that every record's damage is known exactly.  Shared by the CPU tests of the twin
(test_ims_rescue_reference.py) and the GPU tests (test_gpu_ims_rescue.py); each scene and its oracle records are built once.  No
frame is damaged before a channel's first frame.

Damage is a list of (cell n of the frame, 0..551, kind): "a" flips the first chip of the cell (the bit flips, boundary n is marked),
"c" the second (the bit flips, boundary n + 1 is marked), "ac" both (the bit stays, two boundaries are marked), "ca" the second chip
of cell n - 1 and the first of cell n (two bits flip, NOTHING is marked).  Every position is picked by a seeded search through the
twin (tests/ims_rescue_reference.py) over the chips as transmitted, so that each case has the outcome it is named for, and, where a
case is there to catch one mutation of the rule, so that the mutated twin decides otherwise.

`three_miscorrected` is three lone chips the first pass takes for two errors elsewhere: it "corrects" the block to another
codeword, the record says nerr[1] = 0, and the pass never sees it.  It is kept with its real outcome: clean and wrong."""
from __future__ import annotations

import functools

import numpy as np

import ims_rescue_reference as ir
from sdrpp_radiosonde_amd import synth

TILE = 2048
IMS = 2
# case -> (outcome, blocks decoded by the pass, the record's data is the transmitted frame)
EXPECT = {"one": ("clean", 0, True), "two": ("clean", 0, True), "three": ("rescued", 1, True), "four": ("rescued", 1, True),
          "six": ("rescued", 1, True), "three_miscorrected": ("clean", 0, False), "seven": ("unsolved", 0, False),
          "ac_three": ("rescued", 1, True), "ca_one": ("unsolved", 0, False), "first_cell": ("rescued", 1, True),
          "last_cell": ("unsolved", 0, False), "two_blocks": ("rescued", 2, True), "neighbours": ("rescued", 2, True),
          "one_bad_of_two": ("unsolved", 0, False), None: ("clean", 0, True)}
CASES = list(EXPECT)
# the mutation of the twin (keyword arguments of ir.rescue) under which the case must come out differently
CATCHES = {"seven": dict(cap=7), "last_cell": dict(use_next_chip=True), "ac_three": dict(cancel=False)}
DESIGNED = dict(channels=4, tiles=100, seed=91)


def _lone(rng, L, k, must=()):
    """k lone chips in distinct cells of block L, the cells of `must` (cell, kind) among them"""
    taken = {n for n, _ in must}
    free = [n for n in range(46 * L, 46 * L + 46) if n not in taken]
    cells = [int(n) for n in rng.choice(free, size=k - len(must), replace=False)]
    return list(must) + [(n, ("a", "c")[int(rng.integers(0, 2))]) for n in cells]


def _case_flips(case, rng):
    L = int(rng.integers(0, 12))
    if case in ("one", "two", "three", "four", "six", "seven", "three_miscorrected"):
        k = {"one": 1, "two": 2, "three": 3, "four": 4, "six": 6, "seven": 7, "three_miscorrected": 3}[case]
        return _lone(rng, L, k)
    if case == "ac_three":
        n = 46 * L + int(rng.integers(1, 45))
        return [(n, "ac")] + _lone(rng, L, 4, must=[(n, "x")])[1:]
    if case == "ca_one":
        n = 46 * L + int(rng.integers(1, 46))
        return [(n, "ca")] + _lone(rng, L, 3, must=[(n - 1, "x"), (n, "x")])[2:]
    if case == "first_cell":
        return _lone(rng, 0, 3, must=[(0, "a")])
    if case == "last_cell":
        return _lone(rng, 11, 3, must=[(551, "c")])
    if case == "two_blocks":
        L2 = int(rng.choice([x for x in range(12) if abs(x - L) > 1]))
        return _lone(rng, L, 3) + _lone(rng, L2, 3)
    if case == "neighbours":
        L = int(rng.integers(0, 11))
        edge = [(46 * L + 45, "c")] if rng.integers(0, 2) else []
        other = [] if edge else [(46 * L + 46, "a")]
        return _lone(rng, L, 3, must=edge) + _lone(rng, L + 1, 3, must=other)
    if case == "one_bad_of_two":
        L2 = int(rng.choice([x for x in range(12) if abs(x - L) > 1]))
        n = 46 * L2 + int(rng.integers(1, 46))
        return _lone(rng, L, 3) + [(n, "ca")] + _lone(rng, L2, 3, must=[(n - 1, "x"), (n, "x")])[2:]
    raise KeyError(case)


def _apply(chips_row, pos, flips):
    for n, kind in flips:
        first = pos + 48 + 2 * n
        for c in {"a": (first,), "c": (first + 1,), "ac": (first, first + 1), "ca": (first - 1, first)}[kind]:
            chips_row[c] ^= 1


def first_pass_record(chips_row, pos, channel=0):
    """the record the first pass writes for the frame whose sync begins at chip `pos` of an error-free reception of chips_row:
    SPEC 3.3h step 2's restatement of the first pass, block by block through the twin's brute force"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rec = np.zeros(1, dtype=FRAME_DTYPE)
    f = rec[0]
    f["channel"], f["type"], f["len"], f["bitpos"] = channel, IMS, 51, pos
    bits = []
    for blk in ir.received_blocks(chips_row[pos:pos + ir.FRAME_CHIPS]):
        cw, n = ir.first_pass_block(blk)
        f["nerr"][0 if n >= 0 else 1] += n if n >= 0 else 1
        bits += [(cw >> (45 - b)) & 1 for b in range(34)]
    f["data"][:51] = np.packbits(np.array(bits, dtype=np.uint8))
    return rec


def predict(chips_row, pos, tx, **mut):
    """(outcome, blocks decoded, data == tx) of the frame at `pos` under the (mutated) twin, the chips received as they are"""
    rec = first_pass_record(chips_row, pos)
    out, outcomes, _ = ir.rescue(rec, ir.chips_of_streams([chips_row]), **mut)
    return outcomes[0], (int(out[0]["flags"]) >> 8) & 0xF, bool(np.array_equal(out[0]["data"][:51], tx))


def _place(case, chips_row, pos, tx, rng, catch=True):
    """flips for the case at this frame, searched until the twin gives the case's outcome (and the mutated twin another).  A frame
    whose last chip equals the idle chip behind it cannot show `last_cell` to the twin that reads chip p + 1152 (the flip REMOVES a
    mark there); such a frame gets the case without that condition, and the tests ask that at least one frame shows it."""
    if case == "last_cell" and catch and chips_row[pos + 1151] == chips_row[pos + 1152]:
        catch = False
    for _ in range(2000):
        flips = _case_flips(case, rng)
        trial = chips_row.copy()
        _apply(trial, pos, flips)
        if predict(trial, pos, tx) != EXPECT[case]:
            continue
        if catch and case in CATCHES and predict(trial, pos, tx, **CATCHES[case])[0] != "rescued":
            continue
        shared = 46 * (min(n for n, _ in flips) // 46 + 1)       # neighbours: the boundary the two blocks share must be a violated one
        if case == "neighbours" and trial[pos + 47 + 2 * shared] != trial[pos + 48 + 2 * shared]:
            continue
        return flips
    raise RuntimeError(f"no placement found for {case}")


class Scene:
    """iq [C, n, 2] float32 numpy; frames[c] = [(tx chip position of the sync, transmitted data bytes)]; plan[(c, pos)] = (case, flips)"""


def _build(clean):
    C, tiles, seed = DESIGNED["channels"], DESIGNED["tiles"], DESIGNED["seed"]
    n = TILE * tiles
    baud = synth.SONDE_BAUD[IMS]
    nchips = int(n * baud / 48000) + 16
    chips, frames = synth.chip_streams(IMS, seed, np.arange(C), nchips)
    chips = chips.copy()
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.plan = {}
    slot = 0
    for c in range(C):
        for k, (pos, tx) in enumerate(frames[c]):
            case, flips = None, []
            if not clean and k >= 1:
                case = CASES[slot % len(CASES)]
                slot += 1
            if case:
                flips = _place(case, chips[c], pos, tx, rng)
                _apply(chips[c], pos, flips)
            sc.plan[(c, pos)] = (case, flips)
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=seed, ebn0_db=40.0)
    sc.iq = (iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)).copy()
    sc.frames, sc.kind, sc.type, sc.len, sc.C, sc.n = frames, "designed", IMS, 51, C, n
    return sc


@functools.lru_cache(maxsize=None)
def scene(name="designed", clean=False):
    assert name == "designed"
    return _build(clean)


# ---- the noisy scene: iMS-100 at Eb/N0 9.5 dB, chosen on the CPU so that the oracle alone leaves at least 10 records with a rejected
# block.  Over the oracle's records and chips: 127 records, 105 without a rejected block (100 of them the transmitted frame: the first
# pass miscorrects, and nothing behind the code can tell), 22 with one (18 with one rejected block, 4 with two); the twin rescues 12
# of the 22 and leaves 10 unsolved; all 12 rescued records are the transmitted frame.
NOISY = dict(channels=8, tiles=100, ebn0_db=9.5, seed=5)
NOISY_COUNTS = dict(records=127, failed=22, by_blocks=[0, 18, 4], rescued=12, rescued_equal_tx=12)


@functools.lru_cache(maxsize=None)
def noisy_scene():
    """8 iMS-100 channels x 100 tiles at Eb/N0 9.5 dB, seed 5.  CPU oracle: 127 records, 22 with a rejected block (18 with one, 4 with
    two); the twin rescues 12 of them, and all 12 equal the transmitted frame (NOISY_COUNTS; the tests assert these counts)."""
    sb = synth.make_batch(IMS, NOISY["channels"], TILE * NOISY["tiles"], seed=NOISY["seed"], ebn0_db=NOISY["ebn0_db"])
    sc = Scene()
    sc.iq = sb.iq.numpy().copy()
    sc.frames, sc.kind, sc.type, sc.len, sc.C, sc.n, sc.plan = sb.frames, "noisy", IMS, 51, NOISY["channels"], TILE * NOISY["tiles"], {}
    return sc


def scene_of(name, clean=False):
    if name == "noisy":
        return noisy_scene()
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
    """(tx chip position, transmitted data bytes) of the record f; None: no transmitted frame there (a false sync)"""
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in sc.frames[c]), key=lambda t: t[0])
    return (pos, tx) if d < 64 else None


# ---- (block, violation mask) pairs for the block decoder alone (SPEC step 3): sonde_batch_test_ims_block against ir.decode_block
def window_of(block, before, after, first_level=0):
    """the 94 chips of a block as transmitted, from the last chip of the cell before it to the first chip of the cell behind it"""
    bits = [before] + [(int(block) >> (45 - b)) & 1 for b in range(46)] + [after]
    chips = synth.biphase_s(np.array(bits, dtype=np.uint8)) ^ np.uint8(first_level)
    return chips[1:95].copy()


def pair_of_window(w):
    """(received block, violation mask) of a 94-chip window: SPEC step 1 with the block's own numbering"""
    blk = sum(int(w[1 + 2 * b] == w[2 + 2 * b]) << (45 - b) for b in range(46))
    viol = sum(int(w[2 * n] == w[2 * n + 1]) << n for n in range(47))
    return blk, viol


@functools.lru_cache(maxsize=None)
def weight5_codewords(count=8):
    """codewords q of weight 5 and degree <= 44: three wrong bits that the first pass completes with two more"""
    found = []
    for i in range(45):
        for j in range(i + 1, 45):
            for k in range(j + 1, 45):
                cw, n = ir.first_pass_block(1 << i | 1 << j | 1 << k)
                if n == 2 and cw.bit_length() <= 45 and bin(cw).count("1") == 5 and cw not in found:
                    found.append(cw)
                    if len(found) == count:
                        return tuple(found)
    return tuple(found)


def ambiguous_pair(q, codeword):
    """SPEC 3.3h's ambiguous case at m = 5: exactly the boundaries of q violated (coefficient i of q = boundary 45 - i) and the cell LEFT
    of each wrong.  All-left gives the codeword back, all-right gives codeword ^ (1 + x) q, a codeword too: no decode."""
    viol = [45 - i for i in range(46) if (q >> i) & 1]
    e_left = 0
    for v in viol:
        e_left ^= 1 << (45 - (v - 1))
    return int(codeword) ^ e_left, sum(1 << v for v in viol)


@functools.lru_cache(maxsize=None)
def block_pairs(seed=7, n_chip=13000, n_random=6000, n_amb=400):
    """(blocks [n] uint64, viol [n] uint64, index of the first ambiguous pair): codewords with 0..8 wrong chips in the chip model,
    random words near codewords with random masks of 1..7 boundaries, and the ambiguous case over several q and codewords"""
    rng = np.random.default_rng(seed)
    blocks, viols = [], []
    for _ in range(n_chip):
        w = window_of(ir.encode(int(rng.integers(0, 1 << 34))), int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        for c in rng.choice(94, size=int(rng.integers(0, 9)), replace=False):
            w[c] ^= 1
        blk, viol = pair_of_window(w)
        blocks.append(blk)
        viols.append(viol)
    for _ in range(n_random):
        blk = ir.encode(int(rng.integers(0, 1 << 34)))
        for i in rng.choice(46, size=int(rng.integers(0, 5)), replace=False):
            blk ^= 1 << int(i)
        blocks.append(blk)
        viols.append(sum(1 << int(v) for v in rng.choice(47, size=int(rng.integers(1, 8)), replace=False)))
    qs = weight5_codewords()
    for k in range(n_amb):
        blk, viol = ambiguous_pair(qs[k % len(qs)], ir.encode(int(rng.integers(0, 1 << 34))))
        blocks.append(blk)
        viols.append(viol)
    return np.array(blocks, dtype=np.uint64), np.array(viols, dtype=np.uint64), n_chip + n_random


@functools.lru_cache(maxsize=None)
def block_pairs_decoded():
    """the twin over block_pairs(): (decoded blocks [n] uint64, status [n] int32), status = bits flipped, -1 = no decode, block unchanged"""
    blocks, viols, _ = block_pairs()
    out, status = blocks.copy(), np.full(len(blocks), -1, dtype=np.int32)
    for i, (blk, viol) in enumerate(zip(blocks.tolist(), viols.tolist())):
        d = ir.decode_block(blk, [v for v in range(47) if (viol >> v) & 1])
        if d is not None:
            out[i], status[i] = d
    out.setflags(write=False)
    status.setflags(write=False)
    return out, status
