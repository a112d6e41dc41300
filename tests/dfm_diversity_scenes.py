"""Scenes for the tests of sonde_batch_set_diversity on DFM groups (DESIGN SPEC 3.3m), after the pattern of check_diversity_scenes.py (one
chip stream per sonde, copied once per receiver with a lead-in of `delay` more idle chips) and of dfm_rescue_scenes.py (chips flipped
before the modulator, 40 dB: every record's damage is known exactly).  BOTH chips of a pair are flipped ("ac"), so the data bit turns
and no Manchester violation marks it: the pass of SPEC 3.3g has nothing to go on, and what is tested is the pass of SPEC 3.3m.  Shared
by the CPU tests of the twin and the GPU tests; each scene and its oracle records are built once.  A frame is damaged only if it is
not its stream's first and every receiver's copy of it lies inside the scene.

12 channels: a pair, a pair with a 300-chip delay (its offsets given), a triple, an ungrouped channel and a quad.  The members of
the pair, the triple and the quad are 3 chips late each on the one before, with offsets zero: a record's position can be a chip off,
and so member order is the order of the visits whatever the jitter.

A case is, per copy, a list of (word, bit of it) to turn.  Two wrong bits in a word: the first pass gives the word up and the record
keeps it as received.  Three wrong bits inside the support of a weight-4 codeword: the first pass takes it for one wrong bit and
"corrects" the fourth, so the record holds a WRONG codeword, four bits from the truth (a miscorrection).  The cases marked asymmetric
depend on which copy is visited first; they are planned only in those groups, not in the delayed pair."""
from __future__ import annotations

import functools

import numpy as np

import dfm_rescue_reference as dfr
import dfm_rescue_scenes as dsc
from sdrpp_radiosonde_amd import synth

TILE = 2048
DFM = 1
TILES = 60
WINDOW = 960
FRAME_CHIPS = 560
SEED = 91
LISTED_AFTER = FRAME_CHIPS           # chips a record needs before it is listed
W4 = [c for c in dfr.CODEWORDS if bin(c).count("1") == 4]       # the 14 codewords of weight 4, as masks (0x80 = bit 0)

# (stream, delay) of every channel; groups and offsets as set_diversity takes them
MEMBERS = [(0, 0), (0, 3), (1, 0), (1, 300), (2, 0), (2, 3), (2, 6), (3, 0), (4, 0), (4, 3), (4, 6), (4, 9)]
GROUPS = [[0, 1], [2, 3], [4, 5, 6], [8, 9, 10, 11]]
OFFSETS = [0, 0, 0, 300] + [0] * 8
# the same groups with the first pair's second receiver taken for one frame (560 chips) later than it is
OFFSETS_WRONG = [0, FRAME_CHIPS, 0, 300] + [0] * 8
# the scene of the align tests (set_diversity with learn=True and no offsets): the triple's members are 0, 300 and 5000 chips late
ALIGN_MEMBERS = [(2, {4: 0, 5: 300, 6: 5000}[ch]) if s == 2 else (s, d) for ch, (s, d) in enumerate(MEMBERS)]
PAIR_STREAM, DELAYED_STREAM, TRIPLE_STREAM, LONELY_STREAM, QUAD_STREAM = 0, 1, 2, 3, 4

# case -> (expected outcome in a scene, status of the combining rule alone on the copies in order, words decoded jointly)
EXPECT = {"r_only": ("combined", 2, 0), "joint": ("combined", 2, 1), "same_bits": ("untouched", -3, 0), "dist4": ("untouched", -2, 0),
          "miscorrected_partner": ("combined", 2, 0), "three_differ": ("untouched", -1, 0), "seventeen": ("untouched", -1, 0),
          "partner_good": ("untouched", None, 0), "triple_vote": ("combined", 3, 0), "triple_mixed": ("combined", 3, 0),
          "quad_tie": ("combined", -3, 0), "quad_majority": ("combined", 4, 0), "quad_joint": ("combined", 4, 1),
          "lonely": ("untouched", None, 0), None: ("untouched", None, 0)}
PAIR_CASES = ["r_only", "joint", "same_bits", "dist4", "miscorrected_partner", "three_differ", "seventeen", "partner_good", None]
DELAYED_CASES = ["r_only", "joint", "same_bits", "dist4", "three_differ", "seventeen", "partner_good", None]       # the symmetric ones
TRIPLE_CASES = ["triple_vote", "triple_mixed", None]
QUAD_CASES = ["quad_tie", "quad_majority", "quad_joint", None]


def _bits_of(mask):
    return [j for j in range(8) if mask & (0x80 >> j)]


def _pair(rng):
    return [int(j) for j in rng.choice(8, size=2, replace=False)]


def _joint_pairs(rng, n):
    """n pairs of bits of one word, the first two disjoint with a union that is no codeword's support: the one codeword two bits from
    every damaged copy is the truth (further pairs may be anything but equal to an earlier one)"""
    while True:
        ps = [sorted(_pair(rng)) for _ in range(n)]
        union = sum(0x80 >> j for j in ps[0] + ps[1])
        if not set(ps[0]) & set(ps[1]) and union not in W4 and len({tuple(p) for p in ps}) == n:
            return ps


def _miscorrection(rng, avoid=None):
    """three bits inside the support of a weight-4 codeword (avoid: not this support)"""
    while True:
        w = W4[int(rng.integers(len(W4)))]
        if w != avoid:
            return [int(j) for j in rng.choice(_bits_of(w), size=3, replace=False)]


def case_damage(case, rng):
    """[[(word, bit), ...] of copy 0, of copy 1, ...] of a case"""
    ws = [int(w) for w in rng.permutation(33)]
    two = lambda w: [(w, j) for j in _pair(rng)]              # noqa: E731
    if case in ("r_only", "lonely"):
        return [two(ws[0]), two(ws[1])]
    if case == "joint":
        a, b = _joint_pairs(rng, 2)
        return [[(ws[0], j) for j in a], [(ws[0], j) for j in b]]
    if case == "same_bits":
        p = _pair(rng)
        return [[(ws[0], j) for j in p], [(ws[0], j) for j in p]]
    if case == "dist4":              # in each copy's failed word the other copy holds a miscorrection four bits from the received word
        d = [[], []]
        for k, w in enumerate(ws[:2]):
            cw = W4[int(rng.integers(len(W4)))]
            inside, outside = _bits_of(cw), [j for j in range(8) if j not in _bits_of(cw)]
            d[k] += [(w, int(rng.choice(inside))), (w, int(rng.choice(outside)))]
            d[1 - k] += [(w, int(j)) for j in rng.choice(inside, size=3, replace=False)]
        return d
    if case == "miscorrected_partner":
        return [two(ws[0]), two(ws[1]) + [(ws[2], j) for j in _miscorrection(rng)]]
    if case == "three_differ":
        return [two(ws[0]), two(ws[1]) + [(w, j) for w in ws[2:5] for j in _miscorrection(rng)]]
    if case == "seventeen":
        return [[t for w in ws[:9] for t in two(w)], [t for w in ws[9:17] for t in two(w)]]
    if case == "partner_good":
        return [two(ws[0]), []]
    if case == "triple_vote":
        return [two(ws[0]), two(ws[1]), two(ws[2])]
    if case == "triple_mixed":       # word ws[0] failed in copies 0 and 1, copy 2 holds it
        a, b = _joint_pairs(rng, 2)
        return [[(ws[0], j) for j in a], [(ws[0], j) for j in b], two(ws[2])]
    if case == "quad_tie":           # word ws[0] failed in copies 0 and 3; copy 1 holds the truth, copy 2 a miscorrection: one against one
        return [two(ws[0]), two(ws[1]), two(ws[2]) + [(ws[0], j) for j in _miscorrection(rng)], two(ws[0])]
    if case == "quad_majority":      # word ws[0]: copies 1 and 3 hold the truth, copy 2 a miscorrection
        return [two(ws[0]), two(ws[1]), two(ws[2]) + [(ws[0], j) for j in _miscorrection(rng)], two(ws[3])]
    if case == "quad_joint":
        ps = _joint_pairs(rng, 4)
        return [[(ws[0], j) for j in p] for p in ps]
    raise KeyError(case)


class Scene:
    """iq [C, n, 2] float32 numpy; groups, offsets, window as set_diversity takes them; sonde[ch] = (stream, delay); stream_frames[s] =
    [(chip position of the sync, transmitted codewords)]; plan[(stream, k)] = (case, expected outcome) for frame k of the stream;
    damage[(stream, k)] = [(word, bit) turned in each copy]"""


def _copy_row(row, delay, nchips):
    idle = (np.arange(delay) & 1).astype(np.uint8)
    return np.concatenate([idle, row])[:nchips].copy()


def _build(clean, align=False):
    members = ALIGN_MEMBERS if align else MEMBERS
    n = TILE * TILES
    baud = synth.SONDE_BAUD[DFM]
    nchips = int(n * baud / 48000) + 16
    n_streams = 1 + max(s for s, _ in members)
    rows, frames = synth.chip_streams(DFM, SEED, np.arange(n_streams), nchips)
    frames = [[(pos, tx[:33].copy()) for pos, tx in lst] for lst in frames]
    rng = np.random.default_rng(SEED)
    max_delay = {s: max(d for t, d in members if t == s) for s in range(n_streams)}
    lists = {PAIR_STREAM: PAIR_CASES, DELAYED_STREAM: DELAYED_CASES, TRIPLE_STREAM: TRIPLE_CASES, QUAD_STREAM: QUAD_CASES, LONELY_STREAM: ["lonely", None]}
    sc = Scene()
    sc.plan, sc.damage = {}, {}
    for s in range(n_streams):
        slot = 0
        for k, (pos, _) in enumerate(frames[s]):
            case = None
            if not clean and k >= 1 and pos + max_delay[s] + FRAME_CHIPS + 64 <= nchips:
                case = lists[s][slot % len(lists[s])]
                slot += 1
            sc.plan[(s, k)] = (case, EXPECT[case][0])
            sc.damage[(s, k)] = case_damage(case, rng) if case else []
    chips = np.zeros((len(members), nchips), dtype=np.uint8)
    for ch, (s, delay) in enumerate(members):
        chips[ch] = _copy_row(rows[s], delay, nchips)
        copy_no = sum(1 for t, _ in members[:ch] if t == s)
        for k, (pos, _) in enumerate(frames[s]):
            dmg = sc.damage[(s, k)]
            for w, j in (dmg[copy_no] if copy_no < len(dmg) else []):
                c = pos + delay + dsc.chip_of(w, j)
                chips[ch, c] ^= 1                               # both chips of the pair: the bit turns, nothing marks it
                chips[ch, c + 1] ^= 1
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=SEED, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.type, sc.len, sc.C, sc.n, sc.nchips = DFM, 33, len(members), n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames, sc.listed_after = GROUPS, OFFSETS, WINDOW, members, frames, LISTED_AFTER
    return sc


@functools.lru_cache(maxsize=None)
def scene(clean=False, align=False):
    return _build(clean, align)


def sort_records(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


@functools.lru_cache(maxsize=None)
def oracle_frames(clean=False, align=False):
    """the first pass's records of the scene in (channel, bitpos) order, from the CPU oracle (read-only: callers copy before they change
    anything)"""
    import oracle_lib
    oracle_lib.build()
    sc = scene(clean, align)
    fr = sort_records(oracle_lib.batch_run(sc.type, sc.iq, nthreads=4))
    fr.setflags(write=False)
    return fr


def frame_of(sc, f):
    """(stream, frame number k, transmitted codewords) of the record f; None: no transmitted frame there (a false sync)"""
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


def make_record(tx, wrong, channel=0, bitpos=0):
    """the record a first pass leaves of the transmitted codewords `tx` received with the (word, bit) of `wrong` turned: one wrong bit
    of a word is corrected, two are given up on (the word stays as received), three are miscorrected to the codeword one bit away"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rec = np.zeros((), dtype=FRAME_DTYPE)
    d = [int(b) for b in tx[:33]]
    for w, j in wrong:
        d[w] ^= 0x80 >> j
    n_corr = n_lost = 0
    for i in range(33):
        if not any(dfr.syndrome(d[i])):
            continue
        near = [c for c in dfr.CODEWORDS if bin(c ^ d[i]).count("1") == 1]
        if near:
            d[i] = near[0]
            n_corr += 1
        else:
            n_lost += 1
    rec["channel"], rec["type"], rec["len"], rec["bitpos"] = channel, DFM, 33, bitpos
    rec["nerr"] = [n_corr, n_lost]
    rec["data"][:33] = d
    return rec


@functools.lru_cache(maxsize=None)
def unit_cases():
    """The cases of the scenes as caller-made records for the combining rule alone, and random damage on 2..4 copies.  Returns (copies
    [n, 4] FRAME_DTYPE, n_copies [n], names, expected status or None [n])."""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(7)
    txs, _ = synth.dfm_build_frames(SEED + 100, np.arange(8), np.arange(8) + 3)
    rows, names, ks, want = [], [], [], []

    def add(name, txs_of, dmg, status):
        """txs_of: the transmitted frame of every copy, or one for all"""
        txs_of = txs_of if isinstance(txs_of, list) else [txs_of] * len(dmg)
        recs = [make_record(tx, d, channel=j, bitpos=1000 + j) for j, (tx, d) in enumerate(zip(txs_of, dmg))]
        if int(recs[0]["nerr"][1]) <= 0:
            return                                              # copy 0 must have failed
        rows.append(recs)
        names.append(name)
        ks.append(len(dmg))
        want.append(status)

    for rep in range(3):
        for case in PAIR_CASES[:-1] + TRIPLE_CASES[:-1] + QUAD_CASES[:-1]:
            st = EXPECT[case][1]
            if case == "partner_good":                          # the rule alone does not look at the partners' nerr: the word is taken
                st = 2
            add(case, txs[rep], case_damage(case, rng), st)
    for rep in range(60):                                       # random damage: 1..3 wrong bits in 1..6 words of each of 2..4 copies
        K = 2 + rep % 3
        dmg = []
        for _ in range(K):
            words = rng.choice(33, size=int(rng.integers(1, 7)), replace=False)
            dmg.append([(int(w), int(j)) for w in words for j in rng.choice(8, size=int(rng.integers(1, 4)), replace=False)])
        add(f"random_{K}", txs[rep % 8], dmg, None)
    for rep in range(6):                                        # copies of two different frames: the pairing guard
        K = 2 + rep % 3
        add("wrong_pairing", [txs[rep]] + [txs[rep + 1]] * (K - 1), [[(3, 0), (3, 5)]] + [[(9, 1), (9, 2)]] * (K - 1), -1)
    copies = np.zeros((len(rows), 4), dtype=FRAME_DTYPE)
    for i, row in enumerate(rows):
        for j, r in enumerate(row):
            copies[i, j] = r[()]
    return copies, np.array(ks, dtype=np.uint32), names, want


@functools.lru_cache(maxsize=None)
def rescued_partner_scene():
    """Two DFM receivers of one sonde (the second 3 chips late), for a batch with SONDE_FLAG_DFM_RESCUE.  Frames 1, 3, 5, ...
    ("rescued_partner"): receiver 0 has two bits of a word wrong with BOTH chips flipped (nothing marks them: SPEC 3.3g has no erasure
    and the frame stays failed), receiver 1 has two bits of another word wrong with their FIRST chips flipped alone (the pairs are marked:
    SPEC 3.3g rescues the frame).  Frames 2, 4, ... ("both_hidden"): each receiver has a word of its own with two unmarked wrong bits, so
    both stay failed and the pass combines them.  plan[k] = the case of frame k (None: clean)."""
    n = TILE * 30
    baud = synth.SONDE_BAUD[DFM]
    nchips = int(n * baud / 48000) + 16
    rows, frames = synth.chip_streams(DFM, SEED + 7, np.arange(1), nchips)
    rng = np.random.default_rng(SEED + 7)
    members = [(0, 0), (0, 3)]
    chips = np.stack([_copy_row(rows[0], d, nchips) for _, d in members])
    sc = Scene()
    sc.plan = {}
    for k, (pos, _) in enumerate(frames[0]):
        case = None if k == 0 or pos + FRAME_CHIPS + 64 > nchips else ("rescued_partner", "both_hidden")[(k - 1) % 2]
        sc.plan[k] = case
        if case:
            wa, wb = (int(w) for w in rng.choice(33, size=2, replace=False))
            for j in _pair(rng):
                chips[0, pos + dsc.chip_of(wa, j)] ^= 1
                chips[0, pos + dsc.chip_of(wa, j) + 1] ^= 1
            for j in _pair(rng):
                chips[1, pos + 3 + dsc.chip_of(wb, j)] ^= 1
                if case == "both_hidden":
                    chips[1, pos + 3 + dsc.chip_of(wb, j) + 1] ^= 1
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=SEED, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.type, sc.len, sc.C, sc.n, sc.nchips = DFM, 33, 2, n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde = [[0, 1]], None, WINDOW, members
    sc.stream_frames = [[(pos, tx[:33].copy()) for pos, tx in frames[0]]]
    return sc
