"""Scenes for the tests of sonde_batch_set_diversity on M10 / M20 / MRZ-N1 groups (DESIGN SPEC 3.3l), after the pattern of
diversity_scenes.py (one chip stream per sonde, copied once per receiver with a lead-in of `delay` more idle chips) and of
manchester_rescue_scenes.py (chips flipped before the modulator, 40 dB: every record's damage is known exactly).  BOTH chips of a pair
are flipped ("ac"), so the data bit turns and no Manchester violation marks it: the pass of SPEC 3.3f has nothing to go on, and what is
tested is the pass of SPEC 3.3l.  Shared by the CPU tests of the twin and the GPU tests; each scene and its oracle records are built
once.  A frame is damaged only if it is not its stream's first and every receiver's copy of it lies inside the scene.

16 channels per kind: three pairs (one with a 300-chip delay, its offsets given and its copies exchanged), a triple (delays 0 / 37 / 300,
offsets zero), an ungrouped channel, a pair whose true delay the window does not cover, and a quad (one member 120 chips late).

The case `byte0` (a wrong length-byte bit that keeps the recorded len) exists for M10 only: the M10 framer takes every first byte but
0x45 as a 101-byte frame, so 0x64 with one bit turned still is one, while an M20 frame whose 0x45 has a bit turned is recorded with
len 101 and finds no partner of its own length -- the framer admits no such case for M20, and MRZ-N1 has no length byte."""
from __future__ import annotations

import functools

import numpy as np

import manchester_rescue_scenes as ms
from sdrpp_radiosonde_amd import synth

TILE = 2048
M10, MRZN1 = 3, 6
WINDOW = 960
FAR = WINDOW + 200                   # a delay the window does not cover
# kind -> (sonde type, m20, tiles, frame bytes, header chips, chips a record needs before it is listed, seed)
KINDS = {"m10": (M10, False, 100, 101, 32, 1648, 81), "m20": (M10, True, 100, 70, 32, 1648, 82), "mrz": (MRZN1, False, 200, 45, 48, 768, 83)}

# (stream, delay) of every channel; groups and offsets as set_diversity takes them
MEMBERS = [(0, 0), (0, 0), (1, 0), (1, 300), (2, 0), (2, 0), (3, 0), (3, 37), (3, 300), (4, 0), (5, 0), (5, FAR), (6, 0), (6, 0), (6, 120), (6, 0)]
GROUPS = [[0, 1], [2, 3], [4, 5], [6, 7, 8], [10, 11], [12, 13, 14, 15]]
OFFSETS = [0, 0, 0, 300] + [0] * 12
# the scene of the align tests (set_diversity with learn=True and no offsets): the triple's members are 0, 300 and 5000 chips late
ALIGN_MEMBERS = [(3, {6: 0, 7: 300, 8: 5000}[ch]) if s == 3 else (s, d) for ch, (s, d) in enumerate(MEMBERS)]
PAIR_STREAMS, TRIPLE_STREAM, LONELY_STREAMS, QUAD_STREAM = (0, 1, 2), 3, (4, 5), 6
SWAPPED = {0: False, 1: True, 2: False}

# case -> (expected outcome in a scene, status of the combining rule alone; None: depends on which copy comes first)
EXPECT = {"disjoint_3_3": ("combined", 2), "one_vs_seven": ("combined", 2), "nine": ("untouched", -1), "identical_damage": ("untouched", -1),
          "common_bit": ("untouched", -2), "dep4": ("untouched", -3), "in_check": ("combined", 2), "byte0": ("untouched", -1),
          "partner_good": ("untouched", None), "triple_majority": ("combined", 3), "triple_two_wrong": ("combined", 3),
          "quad_tie": ("combined", 4), "lonely": ("untouched", None), None: ("untouched", None)}
PAIR_CASES = {"m10": ["disjoint_3_3", "one_vs_seven", "nine", "identical_damage", "common_bit", "dep4", "in_check", "byte0", "partner_good"],
              "m20": ["disjoint_3_3", "one_vs_seven", "nine", "identical_damage", "common_bit", "dep4", "in_check", "partner_good"],
              "mrz": ["disjoint_3_3", "one_vs_seven", "nine", "identical_damage", "common_bit", "dep4", "in_check", "partner_good"]}
TRIPLE_CASES = ["triple_majority", "triple_two_wrong", None]
QUAD_CASES = ["quad_tie", None]


def case_damage(kind, case, rng, swap=False):
    """[frame bits wrong in copy 0, in copy 1, ...] of a case (swap: the order of the copies reversed)"""
    ln = KINDS[kind][3]
    data_bits = np.arange(8, 8 * (ln - 2))                     # covered bytes behind byte 0
    pick = lambda n: [int(k) for k in rng.choice(data_bits, size=n, replace=False)]      # noqa: E731
    if case in ("disjoint_3_3", "lonely"):
        p = pick(6)
        d = [p[0::2], p[1::2]]
    elif case == "one_vs_seven":
        p = pick(8)
        d = [p[:1], p[1:]]
    elif case == "nine":
        p = pick(9)
        d = [p[:5], p[5:]]
    elif case == "identical_damage":
        p = pick(2)
        d = [list(p), list(p)]
    elif case == "common_bit":
        p = pick(3)
        d = [[p[0], p[1]], [p[0], p[2]]]
    elif case == "dep4":
        (a, b), (c, e) = ms.dependent_four(kind)
        d = [[a, b], [c, e]]
    elif case == "in_check":
        d = [[int(rng.integers(8 * (ln - 2), 8 * ln))], pick(1)]
    elif case == "byte0":
        d = [[int(rng.integers(0, 8))], pick(1)]
    elif case == "partner_good":
        d = [pick(3), []]
    elif case == "triple_majority":
        p = pick(15)
        d = [p[0:5], p[5:10], p[10:15]]
    elif case == "triple_two_wrong":                           # p[0] is wrong in two of three copies: the majority has it wrong
        p = pick(5)
        d = [[p[0], p[1]], [p[0], p[2]], [p[3], p[4]]]
    elif case == "quad_tie":                                   # p[0]: two against two
        p = pick(5)
        d = [[p[0], p[1]], [p[0], p[2]], [p[3]], [p[4]]]
    else:
        raise KeyError(case)
    return d[::-1] if swap else d


class Scene:
    """iq [C, n, 2] float32 numpy; groups, offsets, window as set_diversity takes them; sonde[ch] = (stream, delay); stream_frames[s] =
    [(chip position of the sync, transmitted frame bytes)]; plan[(stream, k)] = (case, expected outcome) for frame k of the stream;
    damage[(stream, k)] = [wrong frame bits of each copy]"""


def _copy_row(row, delay, nchips):
    idle = (np.arange(delay) & 1).astype(np.uint8)
    return np.concatenate([idle, row])[:nchips].copy()


def _build(kind, clean, align=False):
    MEMBERS = ALIGN_MEMBERS if align else globals()["MEMBERS"]
    typ, m20, tiles, ln, H, _, seed = KINDS[kind]
    n = TILE * tiles
    baud = synth.SONDE_BAUD[typ]
    nchips = int(n * baud / 48000) + 16
    n_streams = 1 + max(s for s, _ in MEMBERS)
    rows, frames = synth.chip_streams(typ, seed, np.arange(n_streams), nchips, m20=m20)
    frames = [[(pos, tx[:ln].copy()) for pos, tx in lst] for lst in frames]
    rng = np.random.default_rng(seed)
    flen = H + 16 * ln
    max_delay = {s: max(d for t, d in MEMBERS if t == s) for s in range(n_streams)}
    sc = Scene()
    sc.plan, sc.damage = {}, {}
    slot = {"pair": 0, "triple": 0, "quad": 0, "lonely": 0}
    for s in range(n_streams):
        for k, (pos, _) in enumerate(frames[s]):
            case = None
            if not clean and k >= 1 and pos + max_delay[s] + max(flen, KINDS[kind][5]) <= nchips:
                if s in PAIR_STREAMS:
                    case = PAIR_CASES[kind][slot["pair"] % len(PAIR_CASES[kind])]
                    slot["pair"] += 1
                elif s == TRIPLE_STREAM:
                    case = TRIPLE_CASES[slot["triple"] % 3]
                    slot["triple"] += 1
                elif s == QUAD_STREAM:
                    case = QUAD_CASES[slot["quad"] % 2]
                    slot["quad"] += 1
                else:                                          # ungrouped, too far apart: damaged, and nothing happens
                    case = ("lonely", None)[slot["lonely"] % 2]
                    slot["lonely"] += 1
            sc.plan[(s, k)] = (case, EXPECT[case][0])
            sc.damage[(s, k)] = case_damage(kind, case, rng, SWAPPED.get(s, False)) if case else []
    chips = np.zeros((len(MEMBERS), nchips), dtype=np.uint8)
    copy_no = {}
    for ch, (s, delay) in enumerate(MEMBERS):
        chips[ch] = _copy_row(rows[s], delay, nchips)
        copy_no[ch] = sum(1 for t, _ in MEMBERS[:ch] if t == s)
        for k, (pos, _) in enumerate(frames[s]):
            dmg = sc.damage[(s, k)]
            for bit in (dmg[copy_no[ch]] if copy_no[ch] < len(dmg) else []):
                chips[ch, pos + delay + H + 2 * bit] ^= 1      # both chips of the pair: the bit turns, nothing marks it
                chips[ch, pos + delay + H + 2 * bit + 1] ^= 1
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=seed, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.kind, sc.type, sc.len, sc.C, sc.n, sc.nchips = kind, typ, ln, len(MEMBERS), n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames, sc.listed_after = GROUPS, OFFSETS, WINDOW, MEMBERS, frames, KINDS[kind][5]
    return sc


@functools.lru_cache(maxsize=None)
def scene(kind, clean=False, align=False):
    return _build(kind, clean, align)


@functools.lru_cache(maxsize=None)
def rescued_partner_scene():
    """Two M10 receivers of one sonde, for a batch with SONDE_FLAG_MANCHESTER_RESCUE.  Frames 1, 3, 5, ... ("rescued_partner"): receiver
    0 has one bit wrong with BOTH chips flipped (nothing marks it: SPEC 3.3f has no hint and the frame stays failed), receiver 1 has
    another bit wrong with its FIRST chip flipped alone (the pair is marked: SPEC 3.3f rescues the frame).  Frames 2, 4, ...
    ("both_hidden"): each receiver has a bit of its own wrong with both chips flipped, so both stay failed and the pass combines them.
    plan[k] = the case of frame k (None: clean)."""
    typ, m20, tiles, ln, H, _, seed = KINDS["m10"]
    n = TILE * 60
    baud = synth.SONDE_BAUD[typ]
    nchips = int(n * baud / 48000) + 16
    rows, frames = synth.chip_streams(typ, seed + 7, np.arange(1), nchips)
    rng = np.random.default_rng(seed + 7)
    chips = np.stack([rows[0], rows[0]]).copy()
    sc = Scene()
    sc.plan = {}
    for k, (pos, _) in enumerate(frames[0]):
        case = None if k == 0 else ("rescued_partner", "both_hidden")[(k - 1) % 2]
        sc.plan[k] = case
        if case:
            a, b = (int(v) for v in rng.choice(np.arange(8, 8 * (ln - 2)), size=2, replace=False))
            chips[0, pos + H + 2 * a] ^= 1
            chips[0, pos + H + 2 * a + 1] ^= 1
            chips[1, pos + H + 2 * b] ^= 1
            if case == "both_hidden":
                chips[1, pos + H + 2 * b + 1] ^= 1
    iq, *_ = synth.gfsk_modulate(chips, n, baud, seed=seed, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.kind, sc.type, sc.len, sc.C, sc.n, sc.nchips = "m10", typ, ln, 2, n, nchips
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames = [[0, 1]], None, WINDOW, [(0, 0), (0, 0)], frames
    return sc


def sort_records(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


@functools.lru_cache(maxsize=None)
def oracle_frames(kind, clean=False, align=False):
    """the first pass's records of the scene in (channel, bitpos) order, from the CPU oracle (read-only: callers copy before they change
    anything)"""
    import oracle_lib
    oracle_lib.build()
    sc = scene(kind, clean, align)
    fr = sort_records(oracle_lib.batch_run(sc.type, sc.iq, nthreads=4))
    fr.setflags(write=False)
    return fr


def frame_of(sc, f):
    """(stream, frame number k, transmitted bytes) of the record f; None: no transmitted frame there (a false sync)"""
    stream, delay = sc.sonde[int(f["channel"])]
    d, k = min((abs(int(f["bitpos"]) - (pos + delay)), k) for k, (pos, _) in enumerate(sc.stream_frames[stream]))
    return (stream, k, sc.stream_frames[stream][k][1]) if d < 64 else None


def cut(records, sc, cuts):
    """the records as `cuts` equal submits would list them: a record is listed in the submit in which the last chip it needs arrives"""
    end = records["bitpos"].astype(np.int64) + sc.listed_after
    which = np.minimum(end * cuts // (sc.nchips - 16), cuts - 1)
    return [records[which == s] for s in range(cuts)]


def late_cut_tiles(sc):
    """tiles of a first submit that ends between the two copies of a frame of the delayed pair (stream 1) which the plan combines: the
    undelayed copy is listed in the first submit, the other one 300 chips later in the second"""
    cpt = TILE * (sc.nchips - 16) / sc.n                        # chips per tile
    for k, (pos, _) in enumerate(sc.stream_frames[1]):
        if sc.plan[(1, k)][1] != "combined":
            continue
        target = pos + sc.listed_after + 150
        tiles = round(target / cpt)
        if abs(tiles * cpt - target) <= 90:
            return tiles
    raise AssertionError("no tile boundary falls between the copies of a combined frame")


def _tx(kind, n):
    typ, m20, _, ln, _, _, seed = KINDS[kind]
    build = synth.mrz_build_frames if typ == MRZN1 else synth.m20_build_frames if m20 else synth.m10_build_frames
    return build(seed + 100, np.arange(n), np.arange(n) + 3)[:, :ln]


def make_record(kind, tx, wrong_bits, channel=0, bitpos=0):
    """the record a first pass leaves of the transmitted frame `tx` received with `wrong_bits` turned: the check fails on any"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rec = np.zeros((), dtype=FRAME_DTYPE)
    d = np.unpackbits(np.asarray(tx, dtype=np.uint8))
    for k in wrong_bits:
        d[k] ^= 1
    rec["channel"], rec["type"], rec["len"], rec["bitpos"] = channel, KINDS[kind][0], len(tx), bitpos
    rec["nerr"] = [-1 if len(wrong_bits) else 0, 0]
    rec["data"][:len(tx)] = np.packbits(d)
    return rec


@functools.lru_cache(maxsize=None)
def unit_cases():
    """The cases of the scenes as caller-made records for the combining rule alone, in both copy orders, and random damage on 2..4
    copies.  Returns (copies [n, 4] FRAME_DTYPE, n_copies [n], names, expected status or None [n])."""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(6)
    rows, names, ks, want = [], [], [], []

    def add(name, kind, tx, dmg, status):
        if not dmg[0]:
            return                                              # copy 0 must have failed
        rows.append([make_record(kind, tx, d, channel=j, bitpos=1000 + j) for j, d in enumerate(dmg)])
        names.append(f"{kind}_{name}")
        ks.append(len(dmg))
        want.append(status)

    for kind in KINDS:
        txs = _tx(kind, 8)
        ln = KINDS[kind][3]
        for rep in range(2):
            for case in PAIR_CASES[kind] + TRIPLE_CASES[:2] + QUAD_CASES[:1]:
                for swap in (False, True):
                    st = EXPECT[case][1]
                    if case == "partner_good":                  # the rule alone does not look at the partners' nerr: three unknowns, solved
                        st = 2
                    add(f"{case}{'_swapped' if swap else ''}", kind, txs[rep], case_damage(kind, case, rng, swap), st)
        for rep in range(40):                                   # random damage anywhere in the frame, 2..4 copies
            K = 2 + rep % 3
            dmg = [[int(k) for k in rng.choice(8 * ln, size=int(rng.integers(1, 5)), replace=False)] for _ in range(K)]
            add(f"random_{K}", kind, txs[rep % 8], dmg, None)
    copies = np.zeros((len(rows), 4), dtype=FRAME_DTYPE)
    for i, row in enumerate(rows):
        for j, r in enumerate(row):
            copies[i, j] = r[()]
    return copies, np.array(ks, dtype=np.uint32), names, want
