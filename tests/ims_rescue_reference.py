"""The twin of SONDE_FLAG_IMS_RESCUE (DESIGN SPEC 3.3h), written from the SPEC text alone: plain Python, codeword membership by
polynomial division by 0x1539 (no GF(64) syndromes), the hypotheses by plain enumeration, the first pass's verdict by brute force (a
codeword within distance 2, positions < 46); no code shared with csrc/ims_rescue_kernel.hip.  Test infrastructure only.

    records, outcomes, state = rescue(records, chips, state)

records: FRAME_DTYPE array (not modified; a changed copy is returned); chips(channel, start, count) -> uint8 array of the
channel's on-air chips [start, start + count), or None when they are not available (SPEC step 2, last case); state: {channel:
{"tried", "rescued"}}, carried from call to call.  outcomes[i] is one of OUTCOMES for records[i].

The keyword arguments behind `state` are MUTATIONS of the rule, for the tests that show the designed cases can tell them apart;
nothing else may set them."""
from __future__ import annotations

import itertools

import numpy as np

IMS = 2
FRAME_RESCUED = 2
CAP = 6
FRAME_CHIPS = 1152
NBLK, BLK_BITS, DATA_BITS = 12, 46, 34
G = 0x1539
OUTCOMES = ("other", "clean", "no_chips", "mismatch", "unsolved", "rescued")


def poly_mod(v):
    """the remainder of the polynomial v (bit i = coefficient of x^i) by G"""
    v = int(v)
    while v.bit_length() >= G.bit_length():
        v ^= G << (v.bit_length() - G.bit_length())
    return v


def is_codeword(blk):
    return poly_mod(blk) == 0


def encode(data34):
    v = int(data34) << 12
    return v | poly_mod(v)


# the remainders of every pattern of one or two wrong bits at positions < 46 (division is linear: rem(a ^ b) = rem(a) ^ rem(b))
_NEAR = {0: 0}
_NEAR.update({poly_mod(1 << i): 1 << i for i in range(BLK_BITS)})
_NEAR.update({poly_mod(1 << i ^ 1 << j): 1 << i ^ 1 << j for i, j in itertools.combinations(range(BLK_BITS), 2)})
assert len(_NEAR) == 1 + 46 + 46 * 45 // 2             # distance 5: no two of these patterns share a remainder


def first_pass_rejects(blk):
    """SPEC step 2: the first pass takes a block iff a codeword lies within distance 2 of it"""
    return poly_mod(blk) not in _NEAR


def first_pass_block(blk):
    """what the first pass makes of a block: (the codeword within distance 2, bits corrected), or (the block as received, -1)"""
    e = _NEAR.get(poly_mod(blk))
    return (int(blk), -1) if e is None else (int(blk) ^ e, bin(e).count("1"))


def decode_block(blk, viol, *, cap=CAP, cancel=True, first_fit=False):
    """SPEC step 3 for one block: blk as received (bit b = coefficient 45 - b), viol = the block's violated boundaries (0..46).
    Returns (decoded block, bits flipped) or None."""
    viol = sorted(viol)
    m = len(viol)
    if m == 0 or (cap is not None and m > cap):
        return None
    fits = []
    for picks in itertools.product((-1, 0), repeat=m):
        e = 0
        for v, d in zip(viol, picks):
            cell = v + d
            if 0 <= cell < BLK_BITS:
                unit = 1 << (BLK_BITS - 1 - cell)
                e = (e ^ unit) if cancel else (e | unit)
        if is_codeword(int(blk) ^ e) and e not in fits:
            fits.append(e)
    if not fits or (len(fits) > 1 and not first_fit):
        return None
    return int(blk) ^ fits[0], bin(fits[0]).count("1")


def received_blocks(fc):
    """the 12 blocks of a frame from its chips (fc[0] = the first sync chip): SPEC step 1"""
    out = []
    for L in range(NBLK):
        blk = 0
        for b in range(BLK_BITS):
            n = BLK_BITS * L + b
            blk = (blk << 1) | int(fc[48 + 2 * n] == fc[48 + 2 * n + 1])
        out.append(blk)
    return out


def violations(fc, L, *, use_next_chip=False):
    """the violated boundaries of block L, numbered inside the block (0..46): SPEC step 3"""
    last = NBLK * BLK_BITS - (0 if use_next_chip else 1)
    return [n - BLK_BITS * L for n in range(BLK_BITS * L, BLK_BITS * L + BLK_BITS + 1)
            if n <= last and 48 + 2 * n < len(fc) and fc[47 + 2 * n] == fc[48 + 2 * n]]


def new_state():
    return {"tried": 0, "rescued": 0}


def rescue(records, chips, state=None, *, cap=CAP, use_next_chip=False, cancel=True, first_fit=False, data_stride=DATA_BITS, check_count=True):
    state = {c: dict(v) for c, v in (state or {}).items()}
    out = records.copy()
    outcomes = []
    for f in out:
        ch = int(f["channel"])
        if int(f["type"]) != IMS or int(f["len"]) != 51:
            outcomes.append("other")
            continue
        if int(f["nerr"][1]) < 1:
            outcomes.append("clean")
            continue
        p = int(f["bitpos"])
        fc = chips(ch, p, FRAME_CHIPS)
        if fc is not None and use_next_chip:                 # MUTATION: read the chip behind the frame
            more = chips(ch, p, FRAME_CHIPS + 1)
            fc = more if more is not None else fc
        if fc is None:
            outcomes.append("no_chips")
            continue
        fc = np.asarray(fc, dtype=np.uint8)
        assert len(fc) >= FRAME_CHIPS
        blocks = received_blocks(fc)
        F = [L for L in range(NBLK) if first_pass_rejects(blocks[L])]
        if (check_count and len(F) != int(f["nerr"][1])) or not F:
            outcomes.append("mismatch")
            continue
        st = state.setdefault(ch, new_state())
        st["tried"] += 1
        decoded = {L: decode_block(blocks[L], violations(fc, L, use_next_chip=use_next_chip), cap=cap, cancel=cancel, first_fit=first_fit) for L in F}
        if any(d is None for d in decoded.values()):
            outcomes.append("unsolved")
            continue
        for L, (blk, _) in decoded.items():
            for b in range(DATA_BITS):
                k = data_stride * L + b
                bit = (blk >> (BLK_BITS - 1 - b)) & 1
                f["data"][k >> 3] = (int(f["data"][k >> 3]) & ~(0x80 >> (k & 7))) | (bit << (7 - (k & 7)))
        f["nerr"][0] += sum(n for _, n in decoded.values())
        f["nerr"][1] = 0
        f["flags"] |= FRAME_RESCUED | ((len(F) & 0xF) << 8)
        st["rescued"] += 1
        outcomes.append("rescued")
    return out, outcomes, state


def chips_of_streams(streams):
    """a chips getter over whole recorded chip streams: streams[channel] = uint8 array from chip 0"""
    def get(channel, start, count):
        s = streams[channel]
        return s[start:start + count] if start + count <= len(s) else None
    return get
