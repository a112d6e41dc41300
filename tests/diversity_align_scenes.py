"""Scenes for the tests of the align step (sonde_batch_set_diversity_auto, DESIGN SPEC 3.3k), built from the helpers of
tests/diversity_scenes.py: one RS41 bit stream per sonde, copied once per receiver behind a lead-in of `delay` more alternating bits,
known byte errors injected into each copy, modulated at 40 dB.  No offset is given to the library: it has to find them.

    group  channels  delays (bits)      content
    a      0, 1      0 / 300            the damage cases of diversity_scenes cycling, every third frame clean in both copies
    b      2, 3, 4   0 / 37 / 5000      three members: clean, all three damaged (TRIPLE), the middle copy clean, in turn.  The stream's
                                        preamble is stretched so that its frame period (5040 / 5024 bits) is longer than the delay:
                                        the duplicate rule holds for copies up to one frame period apart
    c      5, 6      0 / 0, then 1500   JUMP_BITS more alternating bits go into the second copy's preamble in front of frame JUMP_FRAME;
                                        even frames clean, odd ones damaged
    d      7, 8      0 / 0              two different sondes, clean: never a match
    e      9, 10     0 / 200            one sonde, one copy of every frame damaged, in turn: never good together, never locks
    -      11                           in no group, every second frame damaged

Shared by test_diversity_align_reference.py (CPU) and test_gpu_diversity_align.py; each scene and its oracle records are built once."""
from __future__ import annotations

import functools

import numpy as np

import diversity_scenes as ds
from sdrpp_radiosonde_amd import synth

TILE = ds.TILE
WINDOW = ds.WINDOW
JUMP_BITS = 1500
JUMP_FRAME = {False: 4, True: 2}        # by `extended`: in mid-stream, a frame that is clean in both copies
GROUPS = [[0, 1], [2, 3, 4], [5, 6], [7, 8], [9, 10]]
# (stream, delay) per channel; stream 2's second copy jumps by JUMP_BITS in mid-stream
MEMBERS = [(0, 0), (0, 300), (1, 0), (1, 37), (1, 5000), (2, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 200), (6, 0)]
TRUE_OFFSETS = [0, 300, 0, 37, 5000, 0, 0, 0, 0, 0, 200, 0]       # groups a and b: what a host that knew would give


class Scene:
    """iq [C, n, 2] float32 numpy; groups; tx[ch] = [(bit position in the channel's stream, transmitted frame bytes, stream, k)];
    plan[(stream, k)] = what was done to frame k of the stream"""


def _build(extended):
    n = TILE * (140 if extended else 120)
    nbits = int(n * 4800 / 48000) + 16
    flen = 518 if extended else 320
    rng = np.random.default_rng(191 + int(extended))
    seed = 511 + int(extended)
    rows, frames = synth.rs41_bitstreams(seed, np.arange(7), nbits + 8192, extended)
    rows, frames = list(rows), list(frames)
    # group b's sonde: a frame period longer than its largest delay
    brow, bframes = synth.rs41_bitstreams(seed + 50, np.array([1]), nbits + 8192, extended, preamble_bytes=110 if extended else 310)
    rows[1], frames[1] = brow[0], bframes[0]
    cases = ds.EXT_CASES if extended else ds.STD_CASES
    sc = Scene()
    sc.plan, damage = {}, {}
    for stream in range(7):
        j = 0
        for k in range(len(frames[stream])):
            what, dmg = "clean", [{}, {}, {}]
            if stream == 0 and k % 3 != 2:
                what = cases[j % len(cases)]
                dmg = ds.case_damage(what, rng)
                j += 1
            elif stream == 1 and k % 3:
                what = ("triple", "triple_middle_clean")[k % 3 - 1]
                dmg = ds.triple_damage(rng, what == "triple_middle_clean")
            elif stream == 2 and k % 2:
                what = ("disjoint_bursts", "overlap_30", "cw_swap")[(k // 2) % 3]
                dmg = ds.case_damage(what, rng)
            elif stream == 5:
                what = "one_copy"
                dmg = ds.case_damage("partner_good", rng, swap=bool(k % 2))
            elif stream == 6 and k % 2 == 0:
                what = "lonely"
                dmg = ds.case_damage("disjoint_bursts", rng)
            sc.plan[(stream, k)] = what
            damage[(stream, k)] = dmg
    bits = np.zeros((len(MEMBERS), nbits), dtype=np.uint8)
    sc.tx, copy_no = [], {}
    for ch, (stream, delay) in enumerate(MEMBERS):
        copy_no[ch] = sum(1 for s, _ in MEMBERS[:ch] if s == stream)
        row = ds._copy_row(rows[stream], delay, nbits + 4096)
        pos_of = [pos + delay for pos, _ in frames[stream]]
        if ch == 6:
            # JUMP_BITS more alternating bits in the middle of the 320-bit preamble in front of frame JUMP_FRAME: the inserted run starts
            # at an even index of the preamble and is even, so the alternation goes on without a seam
            at = pos_of[JUMP_FRAME[extended]] - 160
            assert row[at] == 0 and row[at - 1] == 1
            row = np.concatenate([row[:at], (np.arange(JUMP_BITS) & 1).astype(np.uint8), row[at:]])
            pos_of = [p + (JUMP_BITS if k >= JUMP_FRAME[extended] else 0) for k, p in enumerate(pos_of)]
        bits[ch] = row[:nbits]
        lst = []
        for k, (_, tx) in enumerate(frames[stream]):
            if pos_of[k] + 8 * len(tx) > nbits:
                continue
            for o, v in damage[(stream, k)][copy_no[ch]].items():
                ds._inject(bits[ch], pos_of[k], o, v)
            lst.append((pos_of[k], tx, stream, k))
        sc.tx.append(lst)
    iq, *_ = synth.gfsk_modulate(bits, n, 4800.0, seed=9, ebn0_db=40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.groups, sc.window, sc.flen, sc.C, sc.n, sc.extended = GROUPS, WINDOW, flen, len(MEMBERS), n, extended
    return sc


@functools.lru_cache(maxsize=None)
def scene(extended=False):
    return _build(extended)


@functools.lru_cache(maxsize=None)
def oracle_frames(extended=False):
    """the first pass's records of the scene, from the CPU oracle (read-only: callers copy before they change anything)"""
    import oracle_lib
    oracle_lib.build()
    fr = oracle_lib.batch_run(0, scene(extended).iq, nthreads=4)
    fr.setflags(write=False)
    return fr


def frame_of(sc, f):
    """(stream, frame number k, transmitted bytes, bitpos - the frame's true position) of the record f; the record lies within the 64
    bits diversity_scenes.frame_of allows"""
    d, pos, tx, stream, k = min((abs(int(f["bitpos"]) - pos), pos, tx, stream, k) for pos, tx, stream, k in sc.tx[int(f["channel"])])
    assert d < 64, (int(f["channel"]), int(f["bitpos"]), d)
    return stream, k, tx, int(f["bitpos"]) - pos


def cut(records, sc, cuts):
    return ds.cut(records, sc, cuts)


# ---------------------------------------------------------------- caller-made cases for the align step alone
_FAIL = {o: 0x5A for o in range(104, 144)}                 # 20 wrong bytes in each codeword: the first pass gives up


def _case(name, members, carried=None, off=None, locked=0, mode=3):
    nm = len(members)
    return {"name": name, "members": members, "carried": carried or [None] * nm, "off": list(off or [0] * nm) + [0] * (4 - nm),
            "locked": locked, "mode": mode}


@functools.lru_cache(maxsize=None)
def unit_cases():
    """The designed cases of SPEC 3.3k by name, every pair order under every lock state, both mode bits singly, a member with 70
    records, four members, and random cases.  A case: members = per member the records of the submit, carried = per member a record or
    None, off [4], locked (bit per member), mode."""
    rng = np.random.default_rng(17)
    tx = list(synth.rs41_build_frames(31, np.arange(12), np.arange(12) + 5, False)) + list(synth.rs41_build_frames(32, np.arange(4), np.arange(4) + 5, True))
    X, Y, Z, E = tx[0], tx[1], tx[2], tx[12]
    rec = lambda t, pos, bad=False: ds.make_record(t, _FAIL if bad else {}, 0, pos)      # noqa: E731
    cases = [
        _case("pair_lock", [[rec(X, 1000)], [rec(X, 1450)]]),
        _case("pair_lock_initial_offset_kept", [[rec(X, 1000)], [rec(X, 1450)]], off=[70, 0]),
        _case("chain_of_three", [[rec(X, 1000)], [rec(X, 1100, True), rec(Y, 3980)], [rec(X, 6000), rec(Y, 8880)]]),
        _case("rebase_higher", [[rec(X, 1000)], [rec(X, 1450)]], off=[0, 100], locked=3),
        _case("agree_nothing_learned", [[rec(X, 1000)], [rec(X, 1450)]], off=[0, 450], locked=3),
        _case("lower_joins_locked_higher", [[rec(X, 1000)], [rec(X, 1450)]], off=[0, 500], locked=2),
        _case("carried_only", [[], [rec(X, 980)]], carried=[rec(X, 500), None]),
        _case("carried_failed_is_no_candidate", [[], [rec(X, 980)]], carried=[rec(X, 500, True), None]),
        _case("latest_in_b_wins", [[rec(X, 1000), rec(Y, 3880)], [rec(X, 1450), rec(Y, 4400)]]),
        _case("failed_copies_teach_nothing", [[rec(X, 1000, True)], [rec(X, 1450, True)]]),
        _case("two_sondes", [[rec(X, 1000), rec(Y, 3880)], [rec(Z, 1450), rec(tx[3], 4330)]]),
    ]
    longer = ds.make_record(E, {}, 0, 1450)
    longer["data"][:320] = X                                 # the first 320 bytes are X's, the length is not
    cases.append(_case("same_bytes_other_len", [[rec(X, 1000)], [longer]]))
    hdr = rec(X, 1450)
    hdr["data"][:8] ^= 0xFF
    cases.append(_case("header_differs", [[rec(X, 1000)], [hdr]]))
    last = rec(X, 1450)
    last["data"][319] ^= 1
    cases.append(_case("last_byte_differs", [[rec(X, 1000)], [last]]))
    first = rec(X, 1450)
    first["data"][8] ^= 0x80
    cases.append(_case("byte_8_differs", [[rec(X, 1000)], [first]]))
    elast = ds.make_record(E, {}, 0, 1450)
    elast["data"][517] ^= 1
    cases.append(_case("last_byte_differs_518", [[ds.make_record(E, {}, 0, 1000)], [elast]]))
    cases.append(_case("match_518", [[ds.make_record(E, {}, 0, 1000)], [ds.make_record(E, {}, 0, 1451)]]))
    # every pair order: four members, only the pair (a, b) shares a frame, under every lock state of the two
    for a in range(4):
        for b in range(a + 1, 4):
            for lk in range(4):
                mem = [[rec(tx[4 + m], 1000 + 10 * m)] for m in range(4)]
                mem[b].append(rec(tx[4 + a], 4000 + 100 * b))
                locked = ((lk & 1) << a) | ((lk >> 1) << b)
                cases.append(_case(f"pair_{a}{b}_locks_{lk}", mem, off=[5, 60, 700, 8000], locked=locked))
    # both mode bits singly and none, on a submit that has something to learn and something to mark
    for mode in (0, 1, 2):
        cases.append(_case(f"mode_{mode}", [[rec(X, 1000), rec(Y, 3880)], [rec(X, 1450)], [rec(Y, 9000)]], carried=[None, rec(Y, 4330), None], mode=mode))
    # a member with 70 records: the one that matches sits behind the 64th
    many = [rec(tx[4 + i % 8], 100 + 3000 * i, bad=i % 3 == 0) for i in range(69)] + [rec(X, 300000)]
    cases.append(_case("seventy_records", [[rec(X, 299000)], many]))
    cases.append(_case("seventy_records_lower", [many, [rec(X, 301000), rec(tx[5], 5000)]]))
    # four members, all four copies of one frame in one submit: one stays unmarked
    cases.append(_case("four_copies", [[rec(X, 1000)], [rec(X, 1040)], [rec(X, 6000)], [rec(X, 900)]]))
    # random: frames of a small pool, good or failed, in the submit or carried, any lock state and mode
    for i in range(60):
        nm = int(rng.integers(2, 5))
        pool = [tx[j] for j in rng.choice(12, size=3, replace=False)]
        mem, car = [], []
        for m in range(nm):
            base = int(rng.integers(3000, 20000))
            picks = sorted(rng.choice(4, size=int(rng.integers(0, 4)), replace=False).tolist())
            mem.append([rec(pool[j % 3], base + 2880 * j + int(rng.integers(0, 3)), bad=bool(rng.random() < 0.3)) for j in picks])
            car.append(rec(pool[int(rng.integers(0, 3))], base - 2880, bad=bool(rng.random() < 0.3)) if rng.random() < 0.5 else None)
        cases.append(_case(f"random_{i}", mem, carried=car, off=[int(v) for v in rng.integers(-9000, 9000, size=nm)],
                           locked=int(rng.integers(0, 1 << nm)), mode=int(rng.integers(0, 4))))
    return cases


def twin_case(case):
    """the twin on a case -> (records per member with their flags, off [4], locked, learned, duplicates)"""
    import diversity_align_reference as dar
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
    st = dar.new_state(groups)
    for m in range(nm):
        st["off"][m] = case["off"][m]
        st["locked"][m] = bool((case["locked"] >> m) & 1)
        if case["carried"][m] is not None:
            c = case["carried"][m].copy()
            c["channel"] = m
            st["div"]["carried"][m] = c
    out = dar.align(flat, groups, st, case["mode"])
    per = [out[out["channel"] == m] for m in range(nm)]
    off = [st["off"][m] for m in range(nm)] + case["off"][nm:]
    locked = sum(int(st["locked"][m]) << m for m in range(nm))
    return per, off, locked, st["learned"][0], st["duplicates"][0]


def pack_cases(cases):
    """the cases as SondeBatch.test_diversity_align takes them: (records [n, 4, R], counts [n, 4], n_members [n], carried [n, 4],
    off [n, 4], locked [n], mode [n])"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    n, R = len(cases), max(len(m) for c in cases for m in c["members"])
    records, carried = np.zeros((n, 4, R), dtype=FRAME_DTYPE), np.zeros((n, 4), dtype=FRAME_DTYPE)
    counts, nm = np.zeros((n, 4), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for k, c in enumerate(cases):
        nm[k] = len(c["members"])
        for m, recs in enumerate(c["members"]):
            counts[k, m] = len(recs)
            for i, r in enumerate(recs):
                records[k, m, i] = r[()]
                records[k, m, i]["channel"] = m
            if c["carried"][m] is not None:
                carried[k, m] = c["carried"][m][()]
                carried[k, m]["channel"] = m
    off = np.array([c["off"] for c in cases], dtype=np.int64)
    return records, counts, nm, carried, off, np.array([c["locked"] for c in cases], dtype=np.uint32), np.array([c["mode"] for c in cases], dtype=np.uint32)


# ---------------------------------------------------------------- the fades of the DiversityReceiver test
FADE_BITS = 288                                            # 60 ms of nothing


def fade_plan(frames, total_bits, delay_bits, flen=320):
    """Where each of two antennas loses FADE_BITS in every frame period, so that the test's outcome is designed and not hoped for.
    frames[i] = [(bit position, bytes)] of sonde i in antenna 0's stream, the sondes' frames no more than 30 bytes apart; antenna 1
    receives the same stream delay_bits later.  Returns (fades0, fades1, faded): the bit positions, on antenna 0's clock, at which
    antenna 0 / antenna 1 falls silent, and the frame numbers they hit.  Antenna a's fade lies wholly inside bytes 64 .. 300 of both
    sondes' frame (blocks, not the header or the parity bytes), the two antennas' fades 110 bytes or more apart (no block is damaged
    in both copies).  The first period stays whole -- a group locks at its first frame that is good in two members -- and so do the
    periods whose frame is not complete on the delayed antenna."""
    d = frames[1][0][0] - frames[0][0][0]
    assert abs(d) <= 240, d
    lo, hi = 8 * 64 + max(d, 0), 8 * 300 - FADE_BITS + min(d, 0)          # a fade's start, in bits from sonde 0's frame start
    b0, b1 = lo + 16, hi - 16
    assert b1 - b0 >= 8 * 110
    faded = [k for k, (p, _) in enumerate(frames[0])
             if k >= 1 and k < len(frames[1]) and max(p, frames[1][k][0]) + delay_bits + 8 * flen + 64 <= total_bits]
    return [frames[0][k][0] + b0 for k in faded], [frames[0][k][0] + b1 for k in faded], faded
