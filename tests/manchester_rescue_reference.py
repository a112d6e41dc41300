"""The twin of SONDE_FLAG_MANCHESTER_RESCUE (DESIGN SPEC 3.3f), written from the SPEC text alone: plain Python, subsets by plain
enumeration, no code shared with csrc/check_rescue_kernel.hip.  Test infrastructure only.

    records, outcomes, state = rescue(records, chips, state)

records: FRAME_DTYPE array (not modified; a changed copy is returned); chips(channel, start, count) -> uint8 array of the
channel's on-air chips [start, start + count), or None when they are no longer available (SPEC step 2, last case); state: {channel:
{"tried", "rescued"}}, carried from call to call.  outcomes[i] is one of OUTCOMES for records[i].

The keyword arguments behind `state` are MUTATIONS of the rule, for the tests that show the designed scenes can tell them apart;
nothing else may set them."""
from __future__ import annotations

import functools

import numpy as np

M10, MRZN1 = 3, 6
FRAME_RESCUED = 2
CAP = 8
OUTCOMES = ("other", "clean", "no_hint", "length_doubtful", "too_many", "unsolved", "ambiguous", "rescued")


def m10_check(data, start=0):
    """Meteomodem's 16-bit rolling checksum over the bytes of data (SPEC 3.3b)"""
    cs = start
    for b in data:
        b = int(b)
        c1 = cs & 0xFF
        b = ((b >> 1) | ((b & 1) << 7)) & 0xFF
        b ^= b >> 2
        t6 = (cs ^ (cs >> 2) ^ (cs >> 4)) & 1
        t7 = ((cs >> 1) ^ (cs >> 3) ^ (cs >> 5)) & 1
        t = (cs & 0x3F) | (t6 << 6) | (t7 << 7)
        s = (cs >> 7) & 0xFF
        s ^= s >> 2
        cs = ((c1 << 8) | ((b ^ t ^ s) & 0xFF)) & 0xFFFF
    return cs


def crc16_a001(data, start=0xFFFF):
    crc = start
    for b in data:
        crc ^= int(b)
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    return crc


@functools.lru_cache(maxsize=None)
def _unit_check(kind, bit, zeros_behind, start):
    """the check, from `start`, of the unit byte 1 << bit followed by zeros_behind zero bytes"""
    msg = bytes([1 << bit]) + bytes(zeros_behind)
    return m10_check(msg, start) if kind == M10 else crc16_a001(msg, start)


def syndrome(kind, data, ln):
    """s of SPEC step 3: the check computed over data XOR the stored check"""
    if kind == M10:
        return m10_check(data[:ln - 2]) ^ ((int(data[ln - 2]) << 8) | int(data[ln - 1]))
    return crc16_a001(data[:43]) ^ (int(data[43]) | (int(data[44]) << 8))


def column(kind, ln, k, *, check_cols=True, m20_rows_as_m10=False, mrz_col_start=0):
    """col(k) of SPEC step 3: the change of s when frame bit k (bit 7 - k % 8 of byte k // 8) is flipped"""
    i, j = k // 8, 7 - k % 8
    if i < ln - 2:
        behind = ln - 3 - i
        if kind == M10 and m20_rows_as_m10:
            behind = 101 - 3 - i
        return _unit_check(kind, j, behind, 0 if kind == M10 else mrz_col_start)
    if not check_cols:
        return 0
    hi = (i == ln - 2) if kind == M10 else (i == ln - 1)          # M10: big-endian; MRZ-N1: little-endian
    return 1 << (8 * hi + j)


def new_state():
    return {"tried": 0, "rescued": 0}


def violations(kind, ln, p, chips, channel):
    """V of SPEC step 1, ascending; None: the chips are not available"""
    H = 32 if kind == M10 else 48
    c = chips(channel, p + H, 16 * ln)
    if c is None:
        return None
    c = np.asarray(c, dtype=np.uint8)
    assert c.shape == (16 * ln,)
    return [int(k) for k in np.nonzero(c[0::2] == c[1::2])[0]]


def rescue(records, chips, state=None, *, cap=CAP, first_solution=False, byte0_rule=True, **col_kw):
    state = {c: dict(v) for c, v in (state or {}).items()}
    out = records.copy()
    outcomes = []
    for f in out:
        kind, ln, ch = int(f["type"]), int(f["len"]), int(f["channel"])
        if not ((kind == M10 and ln in (101, 70)) or (kind == MRZN1 and ln == 45)):
            outcomes.append("other")
            continue
        if int(f["nerr"][0]) != -1:
            outcomes.append("clean")
            continue
        V = violations(kind, ln, int(f["bitpos"]), chips, ch)
        if V is None or len(V) == 0:
            outcomes.append("no_hint")
            continue
        if len(V) > cap:
            outcomes.append("too_many")
            continue
        if kind == M10 and byte0_rule and V[0] < 8:
            outcomes.append("length_doubtful")
            continue
        st = state.setdefault(ch, new_state())
        st["tried"] += 1
        s = syndrome(kind, f["data"], ln)
        cols = [column(kind, ln, k, **col_kw) for k in V]
        sols = []
        for m in range(1, 1 << len(V)):
            x = 0
            for j, cj in enumerate(cols):
                if (m >> j) & 1:
                    x ^= cj
            if x == s:
                sols.append(m)
        if not sols:
            outcomes.append("unsolved")
            continue
        if len(sols) > 1 and not first_solution:
            outcomes.append("ambiguous")
            continue
        U = [k for j, k in enumerate(V) if (sols[0] >> j) & 1]
        for k in U:
            f["data"][k // 8] ^= 0x80 >> (k % 8)
        f["nerr"][0] = 0
        f["flags"] |= FRAME_RESCUED | (len(U) << 8)
        st["rescued"] += 1
        outcomes.append("rescued")
    return out, outcomes, state


def chips_of_streams(streams):
    """a chips getter over whole recorded chip streams: streams[channel] = uint8 array from chip 0"""
    def get(channel, start, count):
        s = streams[channel]
        return s[start:start + count] if start + count <= len(s) else None
    return get
