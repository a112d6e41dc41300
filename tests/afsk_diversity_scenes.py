"""Scenes for the tests of sonde_batch_set_diversity on iMet and SRS-C50 groups (DESIGN SPEC 3.3o), after the pattern of
check_diversity_scenes.py (one stream per sonde, copied once per receiver with a lead-in of `delay` more idle symbols) and of
afsk_rescue_scenes.py (data bits flipped before the modulator, 40 dB: every record's damage is known exactly; never a start or stop
bit, never a stream's first packet).  Shared by the CPU tests of the twin and the GPU tests; each scene and its oracle records are
built once.  A packet is damaged only if every receiver's copy of it lies inside the scene.

Frame bit k of a packet (bit 7 - k % 8 of byte k / 8) that starts at symbol `pos` is on the air at pos + 10 (k / 8) + 1 + (7 - k % 8)
(8N1, LSB first).

16 channels per kind: three pairs -- one of them delayed: iMet by 300 symbols, its offsets given and its copies exchanged; C50 by 30
symbols, inside the window --, a triple, an ungrouped channel, a pair whose true delay the window does not cover, and a quad.  The
delayed pair's stream is led in so that a boundary of the AFSK chain's 16 384-sample granule falls between the two copies of one
packet, and that packet is planned as a combined case (late_cut_granules).

The iMet streams carry XDATA packets, so that all three lengths occur.  `xdata_len_byte` (iMet): copy 0 has the set bit of XDATA's
length byte cleared, so the framer records a 5-byte packet there, which finds no partner of its length.  `type_byte` is in the unit
cases only: the framer takes the length from the type byte, and no wrong bit of it keeps the length.  C50's byte sums are weak
(afsk_rescue_scenes.py), so its damage stays in bits 0..5 of a byte except for `alias`, and every planned damage of either kind is drawn
again until the twin's brute force gives the case's status on it -- for a combined case: exactly one subset fits."""
from __future__ import annotations

import functools

import numpy as np

from sdrpp_radiosonde_amd import synth

TILE = 2048
GRANULE = 16384                      # a batch with an AFSK channel takes rows in multiples of this
IMET4, C50 = 4, 5
# kind -> (sonde type, tiles, seed, symbols per second, default window, delays of the delayed pair / the triple / the quad / the far pair)
KINDS = {"imet": (IMET4, 64, 91, synth.IMET_BAUD, 160, 300, (0, 37, 120), 60, 250),
         "c50": (C50, 32, 92, synth.C50_BAUD, 40, 30, (0, 7, 30), 20, 47)}
GROUPS = [[0, 1], [2, 3], [4, 5], [6, 7, 8], [10, 11], [12, 13, 14, 15]]
PAIR_STREAMS, TRIPLE_STREAM, LONELY_STREAMS, QUAD_STREAM = (0, 1, 2), 3, (4, 5), 6
DELAYED_STREAM = 1
ALIGN_TILES = 160                    # the scene of the align tests (set_diversity with learn=True and no offsets; iMet only): 20 granules


def members(kind, align=False):
    """(stream, delay) of every channel"""
    _, _, _, _, _, d, tr, q, far = KINDS[kind]
    if align:
        tr = (0, 300, 5000)
    return [(0, 0), (0, 0), (1, 0), (1, d), (2, 0), (2, 0), (3, tr[0]), (3, tr[1]), (3, tr[2]), (4, 0), (5, 0), (5, far), (6, 0), (6, 0), (6, q), (6, 0)]


def offsets(kind):
    """as set_diversity takes them: iMet's delayed pair has its delay given, C50's lies inside the window"""
    return [0, 0, 0, 300] + [0] * 12 if kind == "imet" else None


SWAPPED = {"imet": {1: True}, "c50": {}}

# case -> (expected outcome in a scene, status of the combining rule alone; None: depends on which copy comes first)
EXPECT = {"disjoint_3_3": ("combined", 2), "one_vs_seven": ("combined", 2), "nine": ("untouched", -1), "identical_damage": ("untouched", -1),
          "common_bit": ("untouched", -2), "dep4": ("untouched", -3), "alias": ("untouched", -3), "in_check": ("combined", 2),
          "type_byte": ("untouched", -1), "xdata_len_byte": ("untouched", -1), "partner_good": ("untouched", None),
          "triple_majority": ("combined", 3), "triple_two_wrong": ("combined", 3), "quad_tie": ("combined", 4), "lonely": ("untouched", None),
          None: ("untouched", None)}
PAIR_CASES = {"imet": ["disjoint_3_3", "one_vs_seven", "nine", "identical_damage", "common_bit", "dep4", "in_check", "xdata_len_byte", "partner_good", None],
              "c50": ["disjoint_3_3", "one_vs_seven", "nine", "identical_damage", "common_bit", "alias", "in_check", "partner_good", None]}
UNIT_ONLY = {"imet": ["type_byte"], "c50": []}
TRIPLE_CASES = ["triple_majority", "triple_two_wrong", None]
QUAD_CASES = ["quad_tie", None]


def first_data_byte(kind, pkt):
    """the first byte whose bits may be unknowns of step 5"""
    return 2 if kind == "c50" else (3 if int(pkt[1]) == 3 else 2)


def case_damage(kind, case, pkt, rng, swap=False):
    """[frame bits wrong in copy 0, in copy 1, ...] of a case on the packet pkt (swap: the order of the copies reversed)"""
    ln = len(pkt)
    lo, top = first_data_byte(kind, pkt), (6 if kind == "c50" else 8)          # C50: bits 0..5 of a byte (LSB index)
    bits_of = lambda i0, i1: np.array([8 * i + 7 - j for i in range(i0, i1) for j in range(top)])      # noqa: E731
    data_bits, check_bits = bits_of(lo, ln - 2), bits_of(ln - 2, ln)
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
    elif case == "dep4":                  # iMet: x^16 + x^12 + x^5 + 1 itself, anywhere behind the header: the four columns cancel
        e = int(rng.integers(8 * lo + 16, 8 * ln))
        d = [[e, e - 5], [e - 12, e - 16]]
    elif case == "alias":                 # C50: bit 7 of byte 2 and bit 7 of byte 4 both change the sums by (128, 128)
        d = [[8 * 2], [8 * 4]]
    elif case == "in_check":
        d = [[int(rng.choice(check_bits))], pick(1)]
    elif case == "type_byte":
        d = [[8 + int(rng.integers(0, 8))], pick(1)]
    elif case == "xdata_len_byte":        # the lowest set bit of the length byte (the streams': 8, and the framer records 5 bytes)
        assert kind == "imet" and int(pkt[1]) == 3 and int(pkt[2]) != 0
        j = (int(pkt[2]) & -int(pkt[2])).bit_length() - 1
        d = [[8 * 2 + 7 - j], pick(1)]
    elif case == "partner_good":
        d = [pick(3), []]
    elif case == "triple_majority":
        p = pick(12)
        d = [p[0:4], p[4:8], p[8:12]]
    elif case == "triple_two_wrong":                           # p[0] is wrong in two of three copies: the majority has it wrong
        p = pick(5)
        d = [[p[0], p[1]], [p[0], p[2]], [p[3], p[4]]]
    elif case == "quad_tie":                                   # p[0]: two against two
        p = pick(5)
        d = [[p[0], p[1]], [p[0], p[2]], [p[3]], [p[4]]]
    else:
        raise KeyError(case)
    return d[::-1] if swap else d


def make_record(kind, tx, wrong_bits, channel=0, bitpos=0):
    """the record a first pass leaves of the transmitted packet `tx` received with `wrong_bits` turned: the check fails on any"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rec = np.zeros((), dtype=FRAME_DTYPE)
    d = np.unpackbits(np.asarray(tx, dtype=np.uint8))
    for k in wrong_bits:
        d[k] ^= 1
    rec["channel"], rec["type"], rec["len"], rec["bitpos"] = channel, KINDS[kind][0], len(tx), bitpos
    rec["nerr"] = [-1 if len(wrong_bits) else 0, 0]
    rec["data"][:len(tx)] = np.packbits(d)
    return rec


def rule_status(kind, tx, dmg):
    """what the twin's brute force says to the copies of `tx` with the damage dmg, copy 0 first (None: copy 0 has none)"""
    import afsk_diversity_reference as ad
    if not dmg[0]:
        return None
    out, st = ad.combine([make_record(kind, tx, d, channel=j) for j, d in enumerate(dmg)])
    if st > 0:
        assert bytes(out["data"][:len(tx)]) == bytes(tx), "the only fitting subset is not the damage"
    return st


def drawn_damage(kind, case, pkt, rng, swap=False):
    """case_damage, drawn again until the rule alone gives the case's status (both copy orders of a pair: either may be visited first)"""
    want = EXPECT[case][1]
    for _ in range(200):
        d = case_damage(kind, case, pkt, rng, swap)
        if case == "xdata_len_byte" or want is None:           # the scene's copy 0 has another len: the rule is not reached
            return d
        orders = [d, d[::-1]] if len(d) == 2 else [d]
        if all(rule_status(kind, pkt, o) == want for o in orders):
            return d
    raise AssertionError(f"no damage for {kind} {case} gives status {want}")


class Scene:
    """iq [C, n, 2] float32 numpy; groups, offsets as set_diversity takes them (window 0: the kind's default); sonde[ch] = (stream,
    delay); stream_frames[s] = [(symbol position of the first start bit, transmitted packet bytes)]; plan[(stream, k)] = (case,
    expected outcome) for packet k of the stream; damage[(stream, k)] = [wrong frame bits of each copy]; late_cut_granules: a first
    submit of that many granules ends between the two copies of packet late_cut_packet of the delayed pair's stream"""


def _modulate(kind, bits, n, seed, snr_db):
    if kind == "c50":
        return synth.afsk_modulate(bits, n, seed=seed, snr_db=snr_db, baud=synth.C50_BAUD, mark_hz=synth.C50_MARK_HZ, space_hz=synth.C50_SPACE_HZ,
                                   fm_dev_hz=4000.0)[0]
    return synth.afsk_modulate(bits, n, seed=seed, snr_db=snr_db)[0]


def _streams(kind, seed, n_streams, nbits):
    if kind == "c50":
        return synth.c50_bitstreams(seed, np.arange(n_streams), nbits)
    return synth.imet_bitstreams(seed, np.arange(n_streams), nbits, xdata=True)


def _build(kind, clean, align):
    typ, tiles, seed, baud, window, pair_delay, _, _, _ = KINDS[kind]
    mem = members(kind, align)
    if align:
        tiles = ALIGN_TILES                                    # the 5000-symbol member still has packets inside the scene
    n = TILE * tiles
    nbits = int(n * baud / 48000) + 16
    n_streams = 1 + max(s for s, _ in mem)
    max_delay = {s: max(d for t, d in mem if t == s) for s in range(n_streams)}
    rows, frames = _streams(kind, seed, n_streams, nbits)
    rows = [r.copy() for r in rows]
    # the delayed pair's stream, led in: a granule boundary falls between the ends of the two copies of its packet `late`
    # (a packet of the scene's second half: a channel that idles on marks first takes a while to settle.  The boundary lies 100 / 20
    # symbols behind the first copy's end: the second copy ends 300 / 30 behind it, and the stream's next packet later than that
    # boundary, so the first copy is still its member's newest record -- the carried one -- when the second is listed)
    late = next(k for k, (p, _) in enumerate(frames[DELAYED_STREAM]) if p >= nbits // 2)
    pos, pkt = frames[DELAYED_STREAM][late]
    per_granule = GRANULE * baud / 48000
    end = pos + 10 * len(pkt) + (100 if kind == "imet" else 20)
    g = int(np.ceil(end / per_granule))
    lead = int(round(g * per_granule)) - end
    rows[DELAYED_STREAM] = np.concatenate([np.ones(lead, dtype=np.uint8), rows[DELAYED_STREAM]])[:nbits]
    frames[DELAYED_STREAM] = [(p + lead, t) for p, t in frames[DELAYED_STREAM] if p + lead + 10 * len(t) <= nbits]
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.plan, sc.damage = {}, {}
    slot = {"pair": 0, "triple": 0, "quad": 0, "lonely": 0}
    swapped = SWAPPED[kind]
    for s in range(n_streams):
        for k, (pos, pkt) in enumerate(frames[s]):
            case = None
            if not clean and k >= 1 and pos + max_delay[s] + 10 * len(pkt) + 40 <= nbits:
                if s == DELAYED_STREAM and k == late:
                    case = "disjoint_3_3"
                elif s in PAIR_STREAMS:
                    for _ in range(len(PAIR_CASES[kind])):      # the next case the packet admits
                        case = PAIR_CASES[kind][slot["pair"] % len(PAIR_CASES[kind])]
                        slot["pair"] += 1
                        if case != "xdata_len_byte" or int(pkt[1]) == 3:
                            break
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
            sc.damage[(s, k)] = drawn_damage(kind, case, pkt, rng, swapped.get(s, False)) if case else []
    bits = np.ones((len(mem), nbits), dtype=np.uint8)
    for ch, (s, delay) in enumerate(mem):
        bits[ch] = np.concatenate([np.ones(delay, dtype=np.uint8), rows[s]])[:nbits]
        copy_no = sum(1 for t, _ in mem[:ch] if t == s)
        for k, (pos, _) in enumerate(frames[s]):
            dmg = sc.damage[(s, k)]
            for fb in (dmg[copy_no] if copy_no < len(dmg) else []):
                bits[ch, pos + delay + 10 * (fb >> 3) + 1 + (7 - (fb & 7))] ^= 1
    iq = _modulate(kind, bits, n, seed, 40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.kind, sc.type, sc.C, sc.n, sc.nbits, sc.baud = kind, typ, len(mem), n, nbits, baud
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames = GROUPS, offsets(kind), window, mem, frames
    sc.late_cut_granules, sc.late_cut_packet = g, late
    return sc


@functools.lru_cache(maxsize=None)
def scene(kind, clean=False, align=False):
    return _build(kind, clean, align)


@functools.lru_cache(maxsize=None)
def rescued_partner_scene():
    """Two iMet receivers of one sonde, for a batch with SONDE_FLAG_AFSK_RESCUE.  Packets 1, 3, 5, ... ("rescued_partner"): receiver 0
    has two separated bits wrong (SPEC 3.3i finds no single pattern: the packet stays failed), receiver 1 one bit (SPEC 3.3i repairs
    it: a good copy).  Packets 2, 4, ... ("both_failed"): each receiver has two separated bits of its own wrong, so both stay failed
    and the pass combines them.  plan[k] = the case of packet k (None: clean)."""
    typ, _, seed, baud, window, *_ = KINDS["imet"]
    n = GRANULE * 4
    nbits = int(n * baud / 48000) + 16
    rows, frames = _streams("imet", seed + 7, 1, nbits)
    rng = np.random.default_rng(seed + 7)
    bits = np.stack([rows[0], rows[0]]).copy()
    sc = Scene()
    sc.plan = {}
    for k, (pos, pkt) in enumerate(frames[0]):
        case = None if k == 0 or pos + 10 * len(pkt) + 40 > nbits else ("rescued_partner", "both_failed")[(k - 1) % 2]
        sc.plan[k] = case
        if not case:
            continue
        lo = first_data_byte("imet", pkt)
        for _ in range(200):
            i0, i1, i2, i3 = (int(v) for v in rng.choice(np.arange(lo, len(pkt) - 2), size=4, replace=False))
            j = [int(v) for v in rng.integers(0, 8, size=4)]
            fb = [8 * i + 7 - b for i, b in zip((i0, i1, i2, i3), j)]
            dmg = [[fb[0], fb[1]], [fb[2]]] if case == "rescued_partner" else [[fb[0], fb[1]], [fb[2], fb[3]]]
            if case == "rescued_partner" or rule_status("imet", pkt, dmg) == 2:
                break
        for c in (0, 1):
            for b in dmg[c]:
                bits[c, pos + 10 * (b >> 3) + 1 + (7 - (b & 7))] ^= 1
    iq = _modulate("imet", bits, n, seed + 7, 40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.kind, sc.type, sc.C, sc.n, sc.nbits, sc.baud = "imet", typ, 2, n, nbits, baud
    sc.groups, sc.offsets, sc.window, sc.sonde, sc.stream_frames = [[0, 1]], None, window, [(0, 0), (0, 0)], frames
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
    fr = sort_records(oracle_lib.batch_run(sc.type, sc.iq, nthreads=4, cap_per_channel=sc.n // 2048 + 64))
    fr.setflags(write=False)
    return fr


def frame_of(sc, f):
    """(stream, packet number k, transmitted bytes) of the record f; None: no transmitted packet starts there (a false sync).  The
    demodulators deliver a bit 6..13 bit times after it was sent; packets are 90 symbols or more apart."""
    stream, delay = sc.sonde[int(f["channel"])]
    d, k = min((abs(int(f["bitpos"]) - (pos + delay)), k) for k, (pos, _) in enumerate(sc.stream_frames[stream]))
    return (stream, k, sc.stream_frames[stream][k][1]) if d <= 24 else None


def cut(records, sc, cuts):
    """the records as `cuts` equal submits would list them: a record is listed in the submit in which its last symbol arrives"""
    end = records["bitpos"].astype(np.int64) + 10 * records["len"].astype(np.int64) + 16
    which = np.minimum(end * cuts // (sc.nbits - 16), cuts - 1)
    return [records[which == s] for s in range(cuts)]


def _valid(kind, ln, rng):
    import afsk_rescue_scenes as rs
    return rs.valid_packet(kind, ln, rng)


@functools.lru_cache(maxsize=None)
def unit_cases():
    """The cases of the scenes as caller-made records for the combining rule alone, in both copy orders, on packets of every shape, and
    random damage on 2..4 copies.  Returns (copies [n, 4] FRAME_DTYPE, n_copies [n], names, expected status or None [n])."""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(6)
    rows, names, ks, want = [], [], [], []

    def add(name, kind, tx, dmg, status):
        if not dmg[0]:
            return                                              # copy 0 must have failed
        rows.append([make_record(kind, tx, d, channel=j, bitpos=1000 + j) for j, d in enumerate(dmg)])
        names.append(f"{kind}_{len(tx)}_{name}")
        ks.append(len(dmg))
        want.append(status)

    for kind, lens in (("imet", (14, 18, 13, 20, 64, 9)), ("c50", (9,))):
        for ln in lens:
            tx = _valid(kind, ln, rng)
            cases = [c for c in PAIR_CASES[kind] + UNIT_ONLY[kind] + TRIPLE_CASES[:2] + QUAD_CASES[:1]
                     if c is not None and (c != "xdata_len_byte" or int(tx[1]) == 3)]
            for case in cases:
                for swap in (False, True):
                    st = EXPECT[case][1]
                    if case == "partner_good":                  # the rule alone does not look at the partners' nerr: three unknowns, solved
                        st = 2 if kind == "imet" else None      # (C50: whatever its weak sums admit)
                    # type_byte, xdata_len_byte: caller-made copies keep the length, and the header bit is an unknown in either order
                    dmg = case_damage(kind, case, tx, rng, swap)
                    if st is not None and kind == "c50" and case not in ("alias", "nine", "identical_damage"):
                        dmg = drawn_damage(kind, case, tx, rng, swap)
                    add(f"{case}{'_swapped' if swap else ''}", kind, tx, dmg, st)
            for rep in range(24):                               # random damage anywhere in the packet, 2..4 copies
                K = 2 + rep % 3
                dmg = [[int(k) for k in rng.choice(8 * ln, size=int(rng.integers(1, 4)), replace=False)] for _ in range(K)]
                add(f"random_{K}", kind, tx, dmg, None)
    copies = np.zeros((len(rows), 4), dtype=FRAME_DTYPE)
    for i, row in enumerate(rows):
        for j, r in enumerate(row):
            copies[i, j] = r[()]
    return copies, np.array(ks, dtype=np.uint32), names, want
