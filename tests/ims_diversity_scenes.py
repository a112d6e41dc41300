"""Scenes for the tests of sonde_batch_set_diversity on iMS-100 groups (SONDE_FLAG_IMS_DIVERSITY, DESIGN SPEC 3.3n), after the pattern of
dfm_diversity_scenes.py (one chip stream per sonde, copied once per receiver with a lead-in of `delay` more idle chips) and of
ims_rescue_scenes.py (chips flipped before the modulator, 40 dB: every record's damage is known exactly).  Shared by the CPU tests of
the twin and the GPU tests; each scene and its oracle records are built once.  A frame is damaged only if it is not its stream's
first and every receiver's copy of it lies inside the scene.

14 channels, 5 groups and an ungrouped channel (a second, part-filled workgroup of the kernel runs): a pair, a pair with a 300-chip delay (its offsets given), a
triple, an ungrouped channel, a quad, and a pair whose second receiver is GIVEN one frame period (1248 chips) later than it is.  The
members of the pairs, the triple and the quad are 3 chips late each on the one before, with offsets zero: a record's position can be
a chip off, and so member order is the order of the visits whatever the jitter.

A case is, per copy, a list of cells of the frame (0..551) whose bit is turned: the FIRST chip of the cell is flipped ("a" of
ims_rescue_scenes.py; the violated boundary that goes with it means nothing to this pass).  rescued_partner_scene, for a batch with
SONDE_FLAG_IMS_RESCUE as well, uses the "ca" kind where SPEC 3.3h must have nothing to go on.  Every position is picked by a seeded
search through the twin (tests/ims_diversity_reference.py) over the blocks as transmitted, so that each case has the outcome it is
named for and, where a case is there to catch one mutation of the rule, so that the mutated twin decides otherwise.  The cases
marked asymmetric depend on which copy is visited first; they are planned only in groups with offsets zero."""
from __future__ import annotations

import functools

import numpy as np

import ims_diversity_reference as idr
import ims_rescue_reference as ir
import ims_rescue_scenes as isc
from sdrpp_radiosonde_amd import synth

TILE = 2048
IMS = 2
TILES = 100
WINDOW = 576
FRAME_CHIPS = 1152
FRAME_PERIOD = 1248                  # chips from sync to sync in synth.chip_streams
SEED = 93
LISTED_AFTER = FRAME_CHIPS           # chips a record needs before it is listed

# (stream, delay) of every channel; groups and offsets as set_diversity takes them
MEMBERS = [(0, 0), (0, 3), (1, 0), (1, 300), (2, 0), (2, 3), (2, 6), (3, 0), (4, 0), (4, 3), (4, 6), (4, 9), (5, 0), (5, 3)]
GROUPS = [[0, 1], [2, 3], [4, 5, 6], [8, 9, 10, 11], [12, 13]]
OFFSETS = [0, 0, 0, 300] + [0] * 9 + [FRAME_PERIOD]
WRONG_GROUP = 4
# the scene of the align tests (set_diversity with learn=True and no offsets): the triple's members are 0, 300 and 2700 chips late
ALIGN_MEMBERS = [(2, {4: 0, 5: 300, 6: 2700}[ch]) if s == 2 else (s, d) for ch, (s, d) in enumerate(MEMBERS)]
PAIR_STREAM, DELAYED_STREAM, TRIPLE_STREAM, LONELY_STREAM, QUAD_STREAM, WRONG_STREAM = range(6)

# case -> (expected outcome in a scene, status of the combining rule alone on the copies in order, blocks decoded by 5b,
#          the mutation that must decide otherwise or None)
# dist6: copy 0 stays; copy 1, visited next, takes its own rejected block from copy 0 and is combined -- with the block it holds as a
# miscorrection left as it is (blocks accepted in r are never touched), so that record is NOT the transmitted frame
EXPECT = {"r_only": ("combined", 2, 0, None), "partner_good": ("untouched", None, 0, None), "v6": ("combined", 2, 1, None),
          "v7": ("untouched", -2, 0, dict(cap=7)), "dist6": ("miscorrected", -2, 0, dict(max_dist=6)),
          "two_blocks": ("untouched", -2, 0, None), "a5": ("untouched", -1, 0, dict(min_agreed=5)),
          "triple_majority": ("combined", 3, 1, None), "triple_taken": ("combined", 3, 0, None), "quad_tie": ("combined", 4, 1, None),
          "wrong_offset": ("untouched", None, 0, dict(min_agreed=0, max_differ=12)), "lonely": ("untouched", None, 0, None),
          None: ("untouched", None, 0, None)}
PAIR_CASES = ["r_only", "partner_good", "v6", "v7", "dist6", "two_blocks", "a5", None]       # dist6, two_blocks: asymmetric
DELAYED_CASES = ["r_only", "v6", "partner_good", "v7", "a5", None]
TRIPLE_CASES = ["triple_majority", "triple_taken", None]
QUAD_CASES = ["quad_tie", None]


def tx_blocks(tx):
    """the 12 codewords of a transmitted frame's 51 data bytes (bit b of a block = coefficient 45 - b)"""
    bits = np.unpackbits(np.asarray(tx[:51], dtype=np.uint8))
    return [ir.encode(int("".join(str(int(b)) for b in bits[34 * L:34 * L + 34]), 2)) for L in range(12)]


def received(tx, cells):
    """the blocks a copy receives when the bits of `cells` (0..551) are turned"""
    blocks = tx_blocks(tx)
    for n in cells:
        blocks[n // 46] ^= 1 << (45 - n % 46)
    return blocks


def record_of_blocks(blocks, channel=0, bitpos=0):
    """the record the first pass writes of these received blocks (SPEC 3.3h step 2 through the twin's brute force)"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rec = np.zeros((), dtype=FRAME_DTYPE)
    rec["channel"], rec["type"], rec["len"], rec["bitpos"] = channel, IMS, 51, bitpos
    bits = []
    for blk in blocks:
        cw, n = ir.first_pass_block(blk)
        rec["nerr"][0 if n >= 0 else 1] += n if n >= 0 else 1
        bits += [(cw >> (45 - b)) & 1 for b in range(34)]
    rec["data"][:51] = np.packbits(np.array(bits, dtype=np.uint8))
    return rec


def _in_block(rng, L, k, avoid=()):
    free = [n for n in range(46 * L, 46 * L + 46) if n not in avoid]
    return [int(n) for n in rng.choice(free, size=k, replace=False)]


def case_damage(case, rng, steady=()):
    """[cells turned in copy 0, in copy 1, ...] of a case (steady: the blocks that do not change from this frame to the next)"""
    Ls = [int(L) for L in rng.permutation(12)]
    if case in ("r_only", "lonely"):
        return [_in_block(rng, Ls[0], 3), _in_block(rng, Ls[1], 3)]
    if case == "partner_good":
        return [_in_block(rng, Ls[0], 3), []]
    if case in ("v6", "v7"):         # the same block rejected in both copies, three wrong bits each (v7: four in copy 1), all distinct
        a = _in_block(rng, Ls[0], 3)
        return [a, _in_block(rng, Ls[0], 3 if case == "v6" else 4, avoid=a)]
    if case == "dist6":              # copy 1 holds block L as a miscorrection q away from the truth; copy 0's block shares one bit with q
        q = isc.weight5_codewords()[int(rng.integers(8))]
        support = [46 * Ls[0] + 45 - i for i in range(46) if (q >> i) & 1]
        inside = [int(n) for n in rng.choice(support, size=3, replace=False)]
        return [[int(rng.choice(support))] + _in_block(rng, Ls[0], 2, avoid=support), inside + _in_block(rng, Ls[1], 3)]
    if case == "two_blocks":         # block Ls[0]: copy 1 holds it; block Ls[1]: rejected in both, 7 positions differ
        b = _in_block(rng, Ls[1], 3)
        return [_in_block(rng, Ls[0], 3) + b, _in_block(rng, Ls[1], 4, avoid=b)]
    if case == "a5":                 # four blocks rejected in copy 0, three others in copy 1: five accepted in both
        return [[n for L in Ls[:4] for n in _in_block(rng, L, 3)], [n for L in Ls[4:7] for n in _in_block(rng, L, 3)]]
    if case == "triple_majority":    # rejected in all three; the majority is wrong in one bit, which the first-pass rule corrects
        a = _in_block(rng, Ls[0], 3)
        b = [a[0]] + _in_block(rng, Ls[0], 2, avoid=a)
        return [a, b, _in_block(rng, Ls[0], 3, avoid=a + b)]
    if case == "triple_taken":       # copies 1 and 2 hold block Ls[0]; each has a rejected block of its own
        return [_in_block(rng, Ls[0], 3), _in_block(rng, Ls[1], 3), _in_block(rng, Ls[2], 3)]
    if case == "quad_tie":           # rejected in all four; copies 0 and 1 share two wrong bits: two against two there
        a = _in_block(rng, Ls[0], 3)
        b = a[:2] + _in_block(rng, Ls[0], 1, avoid=a)
        c = _in_block(rng, Ls[0], 3, avoid=a + b)
        return [a, b, c, _in_block(rng, Ls[0], 3, avoid=a + b + c)]
    if case == "wrong_offset":       # copy 0 rejects a block that is the same in the next frame, copy 1 another one
        L = int(rng.choice(steady))
        return [_in_block(rng, L, 3), _in_block(rng, int(rng.choice([x for x in range(12) if x != L])), 3)]
    raise KeyError(case)


def _status(tx_of_copy, dmg, **mut):
    """status of the combining rule alone on the copies in order (None: copy 0 has not failed, or a partner is good: not tried),
    the result is the transmitted frame, its SONDE_FRAME_JOINT"""
    blocks = [received(tx, cells) for tx, cells in zip(tx_of_copy, dmg)]
    recs = [record_of_blocks(b) for b in blocks]
    if int(recs[0]["nerr"][1]) == 0 or any(int(r["nerr"][1]) == 0 for r in recs[1:]):
        return None, False, 0
    out, st = idr.combine(recs[0], blocks, **mut)
    return st, bytes(out["data"][:51]) == bytes(tx_of_copy[0][:51]), idr.joint(out["flags"])


def place(case, rng, tx, tx_next=None):
    """damage for the case at this frame, searched until the twin gives the case's outcome (and the mutated twin another)"""
    want, status, J, mut = EXPECT[case]
    steady = [L for L in range(12) if tx_next is not None and tx_blocks(tx)[L] == tx_blocks(tx_next)[L]]
    for _ in range(400):
        dmg = case_damage(case, rng, steady)
        if case in ("lonely", "partner_good"):
            if int(record_of_blocks(received(tx, dmg[0]))["nerr"][1]) > 0:
                return dmg
            continue
        if case == "wrong_offset":   # copy 0 of this frame meets copy 1 of the NEXT frame (searched as if that had this draw's damage)
            st, _, _ = _status([tx, tx_next], dmg)
            mst, same, _ = _status([tx, tx_next], dmg, **mut)
            if st == -1 and mst == 2 and same:
                return dmg
            continue
        st, same, j = _status([tx] * len(dmg), dmg)
        if st != status or (st is not None and st > 0 and not (same and j == J)):
            continue
        if case in ("r_only", "lonely", "triple_taken") and _status([tx] * len(dmg), dmg[::-1])[0] is None:
            continue                 # every copy has failed, whichever is visited first
        if mut is not None and not _status([tx] * len(dmg), dmg, **mut)[0] > 0:
            continue
        return dmg
    raise RuntimeError(f"no placement found for {case}")


class Scene:
    """iq [C, n, 2] float32 numpy; groups, offsets, window as set_diversity takes them; sonde[ch] = (stream, delay); stream_frames[s] =
    [(chip position of the sync, transmitted data bytes)]; plan[(stream, k)] = (case, expected outcome) for frame k of the stream;
    damage[(stream, k)] = [cells turned in each copy]"""


def _copy_row(row, delay, nchips):
    idle = (np.arange(delay) & 1).astype(np.uint8)
    return np.concatenate([idle, row])[:nchips].copy()


def _build(clean, align=False):
    members = ALIGN_MEMBERS if align else MEMBERS
    n = TILE * TILES
    baud = synth.SONDE_BAUD[IMS]
    nchips = int(n * baud / 48000) + 16
    n_streams = 1 + max(s for s, _ in members)
    rows, frames = synth.chip_streams(IMS, SEED, np.arange(n_streams), nchips)
    frames = [[(pos, tx[:51].copy()) for pos, tx in lst] for lst in frames]
    rng = np.random.default_rng(SEED)
    max_delay = {s: max(d for t, d in members if t == s) for s in range(n_streams)}
    lists = {PAIR_STREAM: PAIR_CASES, DELAYED_STREAM: DELAYED_CASES, TRIPLE_STREAM: TRIPLE_CASES, QUAD_STREAM: QUAD_CASES,
             LONELY_STREAM: ["lonely", None], WRONG_STREAM: ["wrong_offset"]}
    sc = Scene()
    sc.plan, sc.damage = {}, {}
    for s in range(n_streams):
        slot = 0
        for k, (pos, tx) in enumerate(frames[s]):
            case = None
            if not clean and k >= 1 and pos + max_delay[s] + FRAME_CHIPS + 64 <= nchips:
                case = lists[s][slot % len(lists[s])]
                slot += 1
            if case == "wrong_offset" and k + 1 >= len(frames[s]):
                case = None
            sc.plan[(s, k)] = (case, EXPECT[case][0])
            sc.damage[(s, k)] = place(case, rng, tx, frames[s][k + 1][1] if k + 1 < len(frames[s]) else None) if case else []
    chips = np.zeros((len(members), nchips), dtype=np.uint8)
    for ch, (s, delay) in enumerate(members):
        chips[ch] = _copy_row(rows[s], delay, nchips)
        copy_no = sum(1 for t, _ in members[:ch] if t == s)
        for k, (pos, _) in enumerate(frames[s]):
            dmg = sc.damage[(s, k)]
            isc._apply(chips[ch], pos + delay, [(c, "a") for c in (dmg[copy_no] if copy_no < len(dmg) else [])])
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=SEED, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.type, sc.len, sc.C, sc.n, sc.nchips = IMS, 51, len(members), n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames, sc.listed_after = GROUPS, OFFSETS, WINDOW, members, frames, LISTED_AFTER
    return sc


@functools.lru_cache(maxsize=None)
def scene(clean=False, align=False):
    return _build(clean, align)


def sort_records(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


def _oracle(sc):
    import oracle_lib
    oracle_lib.build()
    recs, streams = [], []
    for c in range(sc.C):
        ch = oracle_lib.Channel(sc.type, c)
        ch.feed(sc.iq[c])
        recs.append(ch.frames())
        bits = ch.bits()
        bits.setflags(write=False)
        streams.append(bits)
    fr = sort_records(np.concatenate(recs))
    fr.setflags(write=False)
    return fr, streams


@functools.lru_cache(maxsize=None)
def oracle_run(clean=False, align=False):
    """(the first pass's records of the scene in (channel, bitpos) order, [chip stream of each channel]) from the CPU oracle (read-only:
    callers copy before they change anything)"""
    return _oracle(scene(clean, align))


def ring_chips(b):
    """a chips getter over a batch's bit rings as they are now: None where sonde_batch_read_bits refuses the range (the chips are not
    all written yet, or no longer held)"""
    from sdrpp_radiosonde_amd.batch import SondeError

    def get(channel, start, count):
        try:
            return b.read_bits(channel, start, count)
        except SondeError:
            return None
    return get


def frame_of(sc, f):
    """(stream, frame number k, transmitted data bytes) of the record f; None: no transmitted frame there (a false sync)"""
    stream, delay = sc.sonde[int(f["channel"])]
    d, k = min((abs(int(f["bitpos"]) - (pos + delay)), k) for k, (pos, _) in enumerate(sc.stream_frames[stream]))
    return (stream, k, sc.stream_frames[stream][k][1]) if d < 64 else None


def cut(records, sc, cuts):
    """the records as `cuts` equal submits would list them: a record is listed in the submit in which the last chip it needs arrives"""
    end = records["bitpos"].astype(np.int64) + sc.listed_after
    which = np.minimum(end * cuts // (sc.nchips - 16), cuts - 1)
    return [records[which == s] for s in range(cuts)]


def late_cut_tiles(sc):
    """tiles of a first submit that ends between the two copies of a frame of the delayed pair which the plan combines: the undelayed
    copy is listed in the first submit, the other one 300 chips later in the second"""
    cpt = TILE * (sc.nchips - 16) / sc.n                        # chips per tile
    for k, (pos, _) in enumerate(sc.stream_frames[DELAYED_STREAM]):
        if sc.plan[(DELAYED_STREAM, k)][1] != "combined":
            continue
        target = pos + sc.listed_after + 150
        tiles = round(target / cpt)
        if abs(tiles * cpt - target) <= 90:
            return tiles
    raise AssertionError("no tile boundary falls between the copies of a combined frame")


@functools.lru_cache(maxsize=None)
def unit_cases():
    """The cases of the scenes as caller-made records and blocks for the combining rule alone, random damage on 2..4 copies, copies of
    two different frames, and records whose nerr[1] is not what their blocks say.  Returns (records [n] FRAME_DTYPE, n_copies [n],
    blocks [n, 4, 12] uint64, names, expected status or None [n])."""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(7)
    txs, _ = synth.ims_build_frames(SEED + 100, np.zeros(10, dtype=np.int64), np.arange(10) + 3)
    recs, ks, blks, names, want = [], [], [], [], []

    def add(name, txs_of, dmg, status, patch=0):
        txs_of = txs_of if isinstance(txs_of, list) else [txs_of] * len(dmg)
        blocks = [received(tx, cells) for tx, cells in zip(txs_of, dmg)]
        rec = record_of_blocks(blocks[0], channel=len(recs) % 7, bitpos=1000 + len(recs))
        if int(rec["nerr"][1]) <= 0:
            return                                              # copy 0 must have failed
        rec["nerr"][1] += patch
        recs.append(rec)
        ks.append(len(dmg))
        blks.append(blocks + [[0] * 12] * (4 - len(blocks)))
        names.append(name)
        want.append(status)

    for rep in range(3):
        for case in PAIR_CASES[:-1] + TRIPLE_CASES[:-1] + QUAD_CASES[:-1]:
            st = EXPECT[case][1]
            if case == "partner_good":                          # the rule alone does not look at the partners' nerr: the block is taken
                st = 2
            add(case, txs[rep], place(case, rng, txs[rep]), st)
    for rep in range(90):                                       # random damage: 1..4 wrong bits in 1..4 blocks of each of 2..4 copies
        K = 2 + rep % 3
        dmg = []
        for _ in range(K):
            Ls = rng.choice(12, size=int(rng.integers(1, 5)), replace=False)
            if rep % 2:
                Ls[0] = 5                                       # half of the cases: block 5 is damaged in every copy
            dmg.append([n for L in Ls for n in _in_block(rng, int(L), int(rng.integers(1, 5)))])
        add(f"random_{K}", txs[rep % 10], dmg, None)
    for rep in range(6):                                        # copies of two different frames: the pairing guard
        K = 2 + rep % 3
        add("wrong_pairing", [txs[rep]] + [txs[rep + 1]] * (K - 1), [_in_block(rng, 3, 3)] + [_in_block(rng, 9, 3)] * (K - 1), -1)
    for rep in range(4):                                        # the record does not say what its blocks say: stays, status 0
        add("mismatch", txs[rep], place("r_only", rng, txs[rep]), 0, patch=1 + rep % 2)
    records = np.zeros(len(recs), dtype=FRAME_DTYPE)
    for i, r in enumerate(recs):
        records[i] = r[()]
    return records, np.array(ks, dtype=np.uint32), np.array(blks, dtype=np.uint64), names, want


def twin_unit(records, n_copies, blocks, i):
    """what the unit entry returns for case i, from the twin: (record, status); status 0 is SPEC step 3's refusal of copy 0"""
    b = [[int(x) for x in blocks[i, j]] for j in range(int(n_copies[i]))]
    if sum(1 for x in b[0] if ir.first_pass_rejects(x)) != int(records[i]["nerr"][1]):
        return records[i].copy(), 0
    return idr.combine(records[i], b)


@functools.lru_cache(maxsize=None)
def rescued_partner_scene():
    """Two iMS-100 receivers of one sonde (the second 3 chips late), for a batch with SONDE_FLAG_IMS_RESCUE.  Frames 1, 3, 5, ...
    ("rescued_partner"): receiver 0 has two "ca" pairs in a block (four wrong bits and no violated boundary: SPEC 3.3h has nothing to go on
    and the frame stays failed), receiver 1 has three lone "a" chips in another block (each marks its boundary: SPEC 3.3h rescues the
    frame).  Frames 2, 4, ... ("both_hidden"): each receiver has a block of its own with two "ca" pairs, so both stay failed and the pass
    combines them.  plan[k] = the case of frame k (None: clean)."""
    n = TILE * 60
    baud = synth.SONDE_BAUD[IMS]
    nchips = int(n * baud / 48000) + 16
    rows, frames = synth.chip_streams(IMS, SEED + 7, np.arange(1), nchips)
    rng = np.random.default_rng(SEED + 7)
    members = [(0, 0), (0, 3)]
    chips = np.stack([_copy_row(rows[0], d, nchips) for _, d in members])
    sc = Scene()
    sc.plan = {}

    def hidden(L):
        """two "ca" pairs in block L that the first pass rejects: cells n - 1, n of each turn, nothing is marked"""
        while True:
            a, b = sorted(int(x) for x in rng.choice(np.arange(46 * L + 1, 46 * L + 46), size=2, replace=False))
            if b - a >= 3 and ir.first_pass_rejects(sum(1 << (45 - c % 46) for c in (a - 1, a, b - 1, b))):
                return [(a, "ca"), (b, "ca")]

    for k, (pos, tx) in enumerate(frames[0]):
        case = None if k == 0 or pos + FRAME_CHIPS + 64 > nchips else ("rescued_partner", "both_hidden")[(k - 1) % 2]
        sc.plan[k] = case
        if case:
            La, Lb = (int(L) for L in rng.choice(12, size=2, replace=False))
            isc._apply(chips[0], pos, hidden(La))
            if case == "both_hidden":
                isc._apply(chips[1], pos + 3, hidden(Lb))
            else:
                trial = chips[1].copy()
                flips = isc._place("three", trial, pos + 3, tx[:51], rng)
                isc._apply(chips[1], pos + 3, flips)
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=SEED, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.type, sc.len, sc.C, sc.n, sc.nchips = IMS, 51, 2, n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde = [[0, 1]], None, WINDOW, members
    sc.stream_frames = [[(pos, tx[:51].copy()) for pos, tx in frames[0]]]
    return sc


@functools.lru_cache(maxsize=None)
def rescued_partner_oracle():
    return _oracle(rescued_partner_scene())


# ---- the align step alone on caller-made iMS-100 records (sonde_batch_test_diversity_align_kind against ims_diversity_reference.align)
def _align_case(name, members, carried=None, off=None, locked=0, mode=3):
    nm = len(members)
    return {"name": name, "members": members, "carried": carried or [None] * nm, "off": list(off or [0] * nm) + [0] * (4 - nm),
            "locked": locked, "mode": mode}


@functools.lru_cache(maxsize=None)
def align_unit_cases():
    """The cases of SPEC 3.3k on iMS-100 records (51 bytes: thirteen words, the last of three bytes; the quick-reject key is made of
    words 11 and 12): pairs that lock, re-base, agree, join a locked member and follow a jump; records equal in words 11 and 12 and
    different before them, so that the byte compare decides alone; records that differ in the key's words only, in byte 50 only and in
    byte 51 only (behind the frame: not looked at); failed copies; every pair order under every lock state; the mode bits; 70 records;
    four copies; random cases."""
    rng = np.random.default_rng(19)
    txs, _ = synth.ims_build_frames(SEED + 200, np.zeros(12, dtype=np.int64), np.arange(12) + 3)
    X, Y, Z = txs[0], txs[1], txs[2]

    def rec(t, pos, bad=False):
        cells = _in_block(rng, 4, 3) if bad else []
        while bad and int(record_of_blocks(received(t, cells))["nerr"][1]) == 0:
            cells = _in_block(rng, 4, 3)
        return record_of_blocks(received(t, cells), 0, pos)

    def changed(t, pos, lo, hi, bit=1):
        r = rec(t, pos)
        r["data"][lo:hi] ^= bit
        return r

    cases = [
        _align_case("pair_lock", [[rec(X, 1000)], [rec(X, 1450)]]),
        _align_case("pair_lock_initial_offset_kept", [[rec(X, 1000)], [rec(X, 1450)]], off=[70, 0]),
        _align_case("chain_of_three", [[rec(X, 1000)], [rec(X, 1100, True), rec(Y, 3980)], [rec(X, 6000), rec(Y, 8880)]]),
        _align_case("rebase_higher", [[rec(X, 1000)], [rec(X, 1450)]], off=[0, 100], locked=3),
        _align_case("agree_nothing_learned", [[rec(X, 1000)], [rec(X, 1450)]], off=[0, 450], locked=3),
        _align_case("lower_joins_locked_higher", [[rec(X, 1000)], [rec(X, 1450)]], off=[0, 500], locked=2),
        _align_case("a_jump_is_followed", [[rec(X, 1000), rec(Y, 2248)], [rec(X, 1450), rec(Y, 2698 + 17)]], off=[0, 450], locked=3),
        _align_case("carried_only", [[], [rec(X, 980)]], carried=[rec(X, 500), None]),
        _align_case("carried_failed_is_no_candidate", [[], [rec(X, 980)]], carried=[rec(X, 500, True), None]),
        _align_case("latest_in_b_wins", [[rec(X, 1000), rec(Y, 2248)], [rec(X, 1450), rec(Y, 2700)]]),
        _align_case("failed_copies_teach_nothing", [[rec(X, 1000, True)], [rec(X, 1450, True)]]),
        _align_case("two_sondes", [[rec(X, 1000), rec(Y, 2248)], [rec(Z, 1450), rec(txs[3], 2698)]]),
        # words 11 and 12 equal, so the key is: the byte compare decides alone
        _align_case("same_key_byte_0_differs", [[rec(X, 1000)], [changed(X, 1450, 0, 1, 0x80)]]),
        _align_case("same_key_byte_43_differs", [[rec(X, 1000)], [changed(X, 1450, 43, 44)]]),
        _align_case("same_key_words_0_to_10_differ", [[rec(X, 1000)], [changed(X, 1450, 0, 44, 0xFF)]]),
        # the key's words: word 11 (bytes 44..47) and the three bytes of word 12 (48..50); byte 51 lies behind the frame
        _align_case("byte_44_differs", [[rec(X, 1000)], [changed(X, 1450, 44, 45)]]),
        _align_case("byte_47_differs", [[rec(X, 1000)], [changed(X, 1450, 47, 48, 0x10)]]),
        _align_case("byte_48_differs", [[rec(X, 1000)], [changed(X, 1450, 48, 49)]]),
        _align_case("last_byte_differs", [[rec(X, 1000)], [changed(X, 1450, 50, 51)]]),
        _align_case("byte_behind_the_frame_differs_and_matches", [[rec(X, 1000)], [changed(X, 1450, 51, 52, 0xFF)]]),
        _align_case("bytes_behind_the_frame_differ_in_the_carried", [[], [rec(X, 980)]], carried=[changed(X, 500, 51, 60, 0xA5), None]),
    ]
    other_len = rec(X, 1450)
    other_len["len"] = 45
    cases.append(_align_case("same_bytes_other_len", [[rec(X, 1000)], [other_len]]))
    for a in range(4):               # every pair order: four members, only the pair (a, b) shares a frame, under every lock state of the two
        for b in range(a + 1, 4):
            for lk in range(4):
                mem = [[rec(txs[4 + m], 1000 + 10 * m)] for m in range(4)]
                mem[b].append(rec(txs[4 + a], 4000 + 100 * b))
                cases.append(_align_case(f"pair_{a}{b}_locks_{lk}", mem, off=[5, 60, 700, 8000], locked=((lk & 1) << a) | ((lk >> 1) << b)))
    for mode in (0, 1, 2):
        cases.append(_align_case(f"mode_{mode}", [[rec(X, 1000), rec(Y, 2248)], [rec(X, 1450)], [rec(Y, 9000)]], carried=[None, rec(Y, 2698), None], mode=mode))
    many = [rec(txs[4 + i % 8], 100 + 1248 * i, bad=i % 3 == 0) for i in range(69)] + [rec(X, 300000)]
    cases.append(_align_case("seventy_records", [[rec(X, 299000)], many]))
    cases.append(_align_case("seventy_records_lower", [many, [rec(X, 301000), rec(txs[5], 5000)]]))
    cases.append(_align_case("four_copies", [[rec(X, 1000)], [rec(X, 1040)], [rec(X, 6000)], [rec(X, 900)]]))
    for i in range(60):              # random: frames of a small pool, good or failed, in the submit or carried, any lock state and mode
        nm = int(rng.integers(2, 5))
        pool = [txs[j] for j in rng.choice(12, size=3, replace=False)]
        mem, car = [], []
        for m in range(nm):
            base = int(rng.integers(3000, 20000))
            mem.append([rec(pool[int(rng.integers(3))], base + 1248 * j + int(rng.integers(-2, 3)), bad=rng.random() < 0.25)
                        for j in range(int(rng.integers(0, 4)))])
            car.append(rec(pool[int(rng.integers(3))], base - 1248, bad=rng.random() < 0.25) if rng.random() < 0.5 else None)
        cases.append(_align_case(f"random_{i}", mem, carried=car, off=[int(v) for v in rng.integers(-500, 500, size=nm)],
                                 locked=int(rng.integers(0, 1 << nm)), mode=int(rng.integers(0, 4))))
    return cases


def twin_align_case(case):
    """ims_diversity_reference.align on a case -> (records per member with their flags, off [4], locked, learned, duplicates)"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    nm = len(case["members"])
    groups = [list(range(nm))]
    flat = np.zeros(sum(len(m) for m in case["members"]), dtype=FRAME_DTYPE)
    i = 0
    for m, recs in enumerate(case["members"]):
        for r in recs:
            flat[i] = r[()]
            flat[i]["channel"] = m
            i += 1
    st = idr.new_state(groups)
    for m in range(nm):
        st["off"][m] = case["off"][m]
        st["locked"][m] = bool((case["locked"] >> m) & 1)
        if case["carried"][m] is not None:
            c = case["carried"][m].copy()
            c["channel"] = m
            st["div"]["carried"][m] = c
    out = idr.align(flat, groups, st, case["mode"])
    per = [out[out["channel"] == m] for m in range(nm)]
    off = [st["off"][m] for m in range(nm)] + case["off"][nm:]
    locked = sum(int(st["locked"][m]) << m for m in range(nm))
    return per, off, locked, st["learned"][0], st["duplicates"][0]


# ---- a partner that step 3 leaves out: its chips are no longer held
LEFT_OUT = dict(tiles=64, submit_tiles=4, delay=8000, seed=SEED + 11)


@functools.lru_cache(maxsize=None)
def left_out_scene():
    """A triple fed in submits of 4 tiles (819 chips; the bit ring is then 8192 chips).  Receiver 0 hears frames 0 and 1 of the sonde and
    then nothing (idle chips: no sync, no record), so its carried record stays frame 1.  Receivers 1 and 2 hear the same stream 8000
    and 8003 chips later, their offsets given.  Frame 1 is damaged as "triple_taken": each copy rejects a block of its own.  When
    receiver 1's copy of frame 1 is visited, its partners are receiver 0's carried record -- failed, and 9000 chips old: its chips are
    no longer in the ring, so step 3 leaves it out -- and receiver 2's copy: two copies remain, members 1 and 2 of three."""
    n = TILE * LEFT_OUT["tiles"]
    baud = synth.SONDE_BAUD[IMS]
    nchips = int(n * baud / 48000) + 16
    rows, frames = synth.chip_streams(IMS, LEFT_OUT["seed"], np.arange(1), nchips)
    frames = [(pos, tx[:51].copy()) for pos, tx in frames[0]]
    rng = np.random.default_rng(LEFT_OUT["seed"])
    D = LEFT_OUT["delay"]
    members = [(0, 0), (0, D), (0, D + 3)]
    dmg = place("triple_taken", rng, frames[1][1])
    chips = np.zeros((3, nchips), dtype=np.uint8)
    for ch, (_, delay) in enumerate(members):
        chips[ch] = _copy_row(rows[0], delay, nchips)
        isc._apply(chips[ch], frames[1][0] + delay, [(c, "a") for c in dmg[ch]])
    end = frames[1][0] + FRAME_CHIPS + 24
    chips[0, end:] = (np.arange(nchips - end) & 1).astype(np.uint8)
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=LEFT_OUT["seed"], ebn0_db=40.0)
    sc = Scene()
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.type, sc.len, sc.C, sc.n, sc.nchips = IMS, 51, 3, n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames = [[0, 1, 2]], [0, D, D + 3], WINDOW, members, [frames]
    sc.step = TILE * LEFT_OUT["submit_tiles"]
    return sc
