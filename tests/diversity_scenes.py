"""Scenes for the sonde_batch_set_diversity tests (DESIGN SPEC 3.3j): one RS41 bit stream per sonde, copied once per receiver with a
lead-in of `delay` more alternating bits, known byte errors injected into each copy's on-air bits, modulated at 40 dB -- every
record's damage is known exactly.  Shared by the CPU test of the twin (test_diversity_reference.py) and the GPU tests
(test_gpu_diversity.py); each scene and its oracle records are built once."""
from __future__ import annotations

import functools

import numpy as np

from sdrpp_radiosonde_amd import synth

TILE = 2048
WINDOW = 960
FAR = WINDOW + 200                   # a delay the window does not cover

# damage per case: (frame bytes wrong in copy A, in copy B, what the rule does with the cluster)
_CW0_13 = list(range(150, 176, 2))   # 13 bytes of codeword 0 (GPS-info block)
_CW1_13 = list(range(149, 175, 2))   # 13 bytes of codeword 1
CASES = {
    "disjoint_bursts": (list(range(104, 144)), list(range(185, 265)), "combined"),
    "gpsraw_whole_vs_status_whole": (list(range(181, 274)), list(range(57, 101)), "combined"),
    "same_pos_13_cw1": (_CW1_13, _CW1_13, "combined"),
    "overlap_30": (list(range(190, 220)), list(range(200, 230)), "combined"),
    "overlap_60": (list(range(185, 245)), list(range(185, 245)), "too_many"),
    "same_block_disjoint_halves": (list(range(183, 225)), list(range(228, 272)), "too_many"),
    "common_13": (_CW0_13, _CW0_13, "undecodable"),
    "partner_good": (list(range(104, 144)), [], "untouched"),
    "cw_swap": (_CW0_13, _CW1_13, "combined"),
    "xdata_burst": (list(range(310, 350)), list(range(104, 144)), "combined"),      # extended frames only
}
STD_CASES = [c for c in CASES if c != "xdata_burst"]
EXT_CASES = list(CASES)
TRIPLE = (list(range(185, 225)), list(range(205, 245)), list(range(230, 270)))     # three receivers: 18 + 17 erasures


def case_damage(case, rng, swap=False):
    """[{frame byte: xor value} for copy A, for copy B] of a table case (swap: the two copies exchanged)"""
    a, b, _ = CASES[case]
    da = {o: int(rng.integers(1, 256)) for o in a}
    if case == "common_13":
        db = dict(da)                                       # the same wrong values in both copies
    elif case == "same_pos_13_cw1":
        db = {o: (lambda v: v if v < da[o] else v + 1)(int(rng.integers(1, 255))) for o in b}      # the same positions, other wrong values
    else:
        db = {o: int(rng.integers(1, 256)) for o in b}
    return [db, da] if swap else [da, db]


def triple_damage(rng, middle_clean=False):
    dmg = [{o: int(rng.integers(1, 256)) for o in offs} for offs in TRIPLE]
    if middle_clean:
        dmg[1] = {}
    return dmg


def cw_of(o):
    return (o - 8) // 24 if o < 56 else (o - 56) & 1


def make_record(tx, damage, channel=0, bitpos=0):
    """the record a first pass leaves of the transmitted frame `tx` with `damage` = {frame byte: xor value}: a codeword with at most 12
    wrong bytes is corrected (nerr = their number), one with more fails (nerr = -1, bytes as received)"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rec = np.zeros((), dtype=FRAME_DTYPE)
    flen = len(tx)
    d = np.array(tx, dtype=np.uint8)
    cnt = [sum(1 for o in damage if cw_of(o) == c) for c in (0, 1)]
    for o, v in damage.items():
        if cnt[cw_of(o)] > 12:
            d[o] ^= v
    rec["channel"], rec["type"], rec["len"], rec["bitpos"] = channel, 0, flen, bitpos
    rec["nerr"] = [c if c <= 12 else -1 for c in cnt]
    rec["data"][:flen] = d
    return rec


def _inject(bits, pos, byte_off, val):
    for b in range(8):
        if (val >> b) & 1:
            bits[pos + 8 * byte_off + b] ^= 1


class Scene:
    """iq [C, n, 2] float32 numpy; groups, offsets [C], window as set_diversity takes them; sonde[ch] = (stream, delay); tx[ch] =
    [(bit position in the channel's stream, transmitted frame bytes)]; plan[(stream, k)] = (case or 'triple' / 'triple_middle_clean' /
    None, expected outcome) for frame k of the stream"""


def _copy_row(row, delay, nbits):
    alt = (np.arange(delay) & 1).astype(np.uint8)
    return np.concatenate([alt, row])[:nbits].copy()


def _build(extended, clean=False):
    n = TILE * (140 if extended else 100)
    nbits = int(n * 4800 / 48000) + 16
    rng = np.random.default_rng(91 + int(extended))
    sc = Scene()
    if extended:
        # streams: 0 -> channels 0, 1; 1 -> channels 2, 3 (delay 300, offsets given, copies exchanged)
        members = [(0, 0), (0, 0), (1, 0), (1, 300)]
        sc.groups, sc.offsets = [[0, 1], [2, 3]], [0, 0, 0, 300]
        cases, shift = EXT_CASES, {0: 0, 1: 6}
        n_streams, swap = 2, {0: False, 1: True}
    else:
        # streams: 0 -> 0, 1; 1 -> 2, 3 (delay 300, offsets given, copies exchanged); 2 -> 4, 5, 6 (delays 0, 37, 300, offsets zero);
        # 3 -> 7 (in no group); 4 -> 8, 9 (true delay beyond the window, offsets zero); 5 -> 10, and an EXTENDED stream -> 11
        members = [(0, 0), (0, 0), (1, 0), (1, 300), (2, 0), (2, 37), (2, 300), (3, 0), (4, 0), (4, FAR), (5, 0), (6, 0)]
        sc.groups, sc.offsets = [[0, 1], [2, 3], [4, 5, 6], [8, 9], [10, 11]], [0, 0, 0, 300, 0, 0, 0, 0, 0, 0, 0, 0]
        cases, shift = STD_CASES, {0: 0, 1: 5}
        n_streams, swap = 6, {0: False, 1: True}
    flen = 518 if extended else 320
    rows, frames = synth.rs41_bitstreams(411 + int(extended), np.arange(n_streams), nbits + 2048, extended)
    if not extended:
        erow, eframes = synth.rs41_bitstreams(433, np.array([6]), nbits + 2048, True)
        rows, frames = list(rows) + [erow[0]], list(frames) + [eframes[0]]
    sc.plan, sc.tx, sc.sonde = {}, [], members
    bits = np.zeros((len(members), nbits), dtype=np.uint8)
    copy_no = {}
    for ch, (stream, delay) in enumerate(members):
        bits[ch] = _copy_row(rows[stream], delay, nbits)
        sc.tx.append([(pos + delay, tx) for pos, tx in frames[stream] if pos + delay + 8 * len(tx) <= nbits])
        copy_no[ch] = sum(1 for s, _ in members[:ch] if s == stream)
    # the damage of every stream's frames, drawn once per (stream, frame) so that the copies of a frame share one draw
    damage = {}
    for stream in range(len(rows)):
        for k in range(len(frames[stream])):
            case, expect, dmg = None, "untouched", [{}, {}, {}]
            if not clean:
                if stream in shift:
                    case = cases[(k + shift[stream]) % len(cases)]
                    dmg, expect = case_damage(case, rng, swap[stream]), CASES[case][2]
                elif stream == 2 and not extended:
                    case = ("triple", "triple_middle_clean", None)[k % 3]
                    if case:
                        dmg = triple_damage(rng, case == "triple_middle_clean")
                        expect = "combined" if case == "triple" else "untouched"
                elif k % 2 == 0:                            # ungrouped, too far apart, lengths differ: damaged, and nothing happens
                    case, dmg = "lonely", case_damage("disjoint_bursts", rng)
            sc.plan[(stream, k)] = (case, expect)
            damage[(stream, k)] = dmg
    for ch, (stream, delay) in enumerate(members):
        for k, (pos, tx) in enumerate(frames[stream]):
            if pos + delay + 8 * len(tx) > nbits:
                continue
            for o, v in damage[(stream, k)][copy_no[ch]].items():
                _inject(bits[ch], pos + delay, o, v)
    iq, *_ = synth.gfsk_modulate(bits, n, 4800.0, seed=7, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.window, sc.flen, sc.C, sc.n, sc.extended, sc.stream_frames = WINDOW, flen, len(members), n, extended, frames
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


def frame_of(sc, f):
    """(stream, frame number k, transmitted bytes) of the record f"""
    ch = int(f["channel"])
    stream, delay = sc.sonde[ch]
    d, k = min((abs(int(f["bitpos"]) - (pos + delay)), k) for k, (pos, _) in enumerate(sc.stream_frames[stream]))
    assert d < 64, (ch, int(f["bitpos"]), d)
    return stream, k, sc.stream_frames[stream][k][1]


def cut(records, sc, cuts):
    """the records as `cuts` equal submits would list them: a record belongs to the submit in which its last bit arrives"""
    nbits = sc.n // 10
    end = records["bitpos"].astype(np.int64) + 8 * records["len"].astype(np.int64)
    which = np.minimum(end * cuts // nbits, cuts - 1)
    return [records[which == s] for s in range(cuts)]


@functools.lru_cache(maxsize=None)
def unit_cases():
    """About 200 caller-made cases for the combining rule alone: every table case in both copy orders and both lengths, three and four
    copies, and random damage.  Returns (copies [n, 4] FRAME_DTYPE, n_copies [n], names)."""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(5)
    txs = {False: synth.rs41_build_frames(21, np.arange(8), np.arange(8) + 3, False), True: synth.rs41_build_frames(22, np.arange(8), np.arange(8) + 3, True)}
    rows, names = [], []

    def add(name, tx, dmg):
        recs = [make_record(tx, d, channel=j, bitpos=1000 + j) for j, d in enumerate(dmg)]
        if all(int(v) >= 0 for v in recs[0]["nerr"]):
            return                                          # copy 0 must have a failed codeword
        rows.append(recs)
        names.append((name, len(dmg)))

    for ext in (False, True):
        for rep in range(2):
            tx = txs[ext][rep]
            for case in (EXT_CASES if ext else STD_CASES):
                for swap in (False, True):
                    add(f"{case}{'_swapped' if swap else ''}_{518 if ext else 320}", tx, case_damage(case, rng, swap))
        for rep in range(3):
            tx = txs[ext][2 + rep]
            t3 = triple_damage(rng)
            add("triple", tx, t3)
            add("triple_outer_two", tx, [t3[0], t3[2]])                 # too many erasures without the middle copy
            add("triple_reversed", tx, t3[::-1])
            add("quad", tx, t3 + [{o: int(rng.integers(1, 256)) for o in range(100, 160)}])
            add("quad_clean_last", tx, t3 + [{}])
            # 24 bytes of codeword 1 wrong in both copies with different values and one more with the same wrong value: with 24
            # erasures the code has no redundancy left, the decoder fills in a codeword that was never sent, and the accept step rejects it
            offs = list(range(183, 233, 2))
            da = {o: int(rng.integers(1, 255)) for o in offs}
            add("e24_and_a_common_error", tx, [da, {o: (v + 1 if o != offs[-1] else v) for o, v in da.items()}])
        for rep in range(48):                               # random bursts, 2..4 copies
            tx = txs[ext][rep % 8]
            K = 2 + rep % 3
            dmg = []
            for _ in range(K):
                a = int(rng.integers(8, len(tx) - 30))
                ln = int(rng.integers(14, 90))
                dmg.append({o: int(rng.integers(1, 256)) for o in range(a, min(a + ln, len(tx)))})
            add(f"random_{K}", tx, dmg)
    copies = np.zeros((len(rows), 4), dtype=FRAME_DTYPE)
    for i, row in enumerate(rows):
        for j, r in enumerate(row):
            copies[i, j] = r[()]
    return copies, np.array([k for _, k in names], dtype=np.uint32), [nm for nm, _ in names]
