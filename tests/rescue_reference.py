"""An independent numpy / Python twin of SONDE_FLAG_RS41_RESCUE (DESIGN SPEC 3.3c): its own GF(2^8) tables, a textbook
errors-and-erasures RS(255,231) decoder on polynomials (erasure locator, Forney syndromes, Massey's algorithm, exhaustive root
search, Forney's formula over the errata locator, final syndrome check), the layout learner and the acceptance step.

    rescue(frames, state) takes frame records in (channel, time) order -- what SondeBatch.frames() or the oracle return -- and
    returns the records the feature must produce, plus one outcome per record; `state` carries the per-channel layouts and
    counters from call to call (a call per submit, or one call for the whole stream: the same result).

Nothing here is shared with the library: the tests compare byte for byte."""
from __future__ import annotations

import numpy as np

NROOTS = 24
FRAME_RESCUED = 2
RS41 = 0

# ---------------------------------------------------------------- GF(2^8) / 0x11D
EXP = [0] * 512
LOG = [0] * 256
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
for _i in range(255, 512):
    EXP[_i] = EXP[_i - 255]


def gmul(a, b):
    return 0 if a == 0 or b == 0 else EXP[LOG[a] + LOG[b]]


def gdiv(a, b):
    assert b != 0
    return 0 if a == 0 else EXP[LOG[a] + 255 - LOG[b]]


def poly_eval(p, x):
    """p[0] + p[1] x + ... (Horner)"""
    r = 0
    for c in reversed(p):
        r = gmul(r, x) ^ c
    return r


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                out[i + j] ^= gmul(ai, bj)
    return out


def syndromes(word):
    """S_j = word(alpha^j), j = 0..23; coefficient k of the word is word[k]"""
    return [poly_eval(word, EXP[j]) for j in range(NROOTS)]


def rs_encode(msg):
    """systematic codeword of len(msg) + 24 bytes: positions 0..23 parity, 24.. the message (roots alpha^0..alpha^23)"""
    g = [1]
    for j in range(NROOTS):
        g = poly_mul(g, [EXP[j], 1])
    rem = [0] * NROOTS
    for m in reversed([int(v) for v in msg]):
        fb = m ^ rem[-1]
        rem = [0] + rem[:-1]
        if fb:
            rem = [r ^ gmul(fb, gi) for r, gi in zip(rem, g[:NROOTS])]
    return rem + [int(v) for v in msg]


def rs_decode_ee(word, erased):
    """Bounded-distance errors-and-erasures decoding of word[0..n) (n = len(word)): (status, word').  A word decodes iff a codeword
    differs from it in erased positions and in v others with 2 v + e <= 24.  status: bytes changed, or -1 (word' = word)."""
    w = [int(v) for v in word]
    n = len(w)
    E = [k for k in range(n) if erased[k]]
    e = len(E)
    if e > NROOTS:
        return -1, w
    S = syndromes(w)
    if not any(S):
        return 0, w
    gamma = [1]
    for k in E:
        gamma = poly_mul(gamma, [1, EXP[k]])
    T = poly_mul(gamma, S)[:NROOTS]
    U = T[e:]                                   # Forney syndromes: they obey the error locator's recurrence alone
    # Massey
    Cp, Bp, L, m, b = [1], [1], 0, 1, 1
    for r in range(len(U)):
        d = U[r]
        for i in range(1, L + 1):
            if i < len(Cp):
                d ^= gmul(Cp[i], U[r - i])
        if d == 0:
            m += 1
            continue
        coef = gdiv(d, b)
        old = list(Cp)
        shifted = [0] * m + [gmul(coef, c) for c in Bp]
        Cp = [(Cp[i] if i < len(Cp) else 0) ^ (shifted[i] if i < len(shifted) else 0) for i in range(max(len(Cp), len(shifted)))]
        if 2 * L <= r:
            L, Bp, b, m = r + 1 - L, old, d, 1
        else:
            m += 1
    while len(Cp) > 1 and Cp[-1] == 0:
        Cp.pop()
    if len(Cp) - 1 != L or 2 * L + e > NROOTS:
        return -1, w
    roots = [k for k in range(n) if not erased[k] and poly_eval(Cp, EXP[(255 - k) % 255]) == 0]
    if len(roots) != L:
        return -1, w
    psi = poly_mul(Cp, gamma)
    omega = poly_mul(psi, S)[:NROOTS]
    dpsi = [psi[j + 1] if (j + 1) % 2 else 0 for j in range(len(psi) - 1)] or [0]
    out = list(w)
    for k in E + roots:
        xinv = EXP[(255 - k) % 255]
        den = poly_eval(dpsi, xinv)
        if den == 0:
            return -1, w
        out[k] ^= gmul(EXP[k], gdiv(poly_eval(omega, xinv), den))
    if any(syndromes(out)):
        return -1, w
    return sum(1 for a, c in zip(w, out) if a != c), out


# ---------------------------------------------------------------- the frame rule
def crc16(data):
    crc = 0xFFFF
    for v in data:
        crc ^= int(v) << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def block_ok(d, off, ln):
    return crc16(d[off + 2: off + 2 + ln]) == (d[off + 2 + ln] | (d[off + 3 + ln] << 8))


def walk(d, flen):
    """the chain as received from offset 57: [(offset, type, len)] if it lands exactly on flen in at most 16 blocks, else None"""
    off, lay = 57, []
    while off < flen:
        if len(lay) == 16 or off + 4 > flen:
            return None
        ln = d[off + 1]
        if off + ln + 4 > flen:
            return None
        lay.append((off, d[off], ln))
        off += ln + 4
    return lay


def cw_of(o):
    """the codeword frame byte o belongs to (parity bytes 8 + 24 c .. 31 + 24 c, then interleaved from 56)"""
    return (o - 8) // 24 if o < 56 else (o - 56) & 1


def split(d, flen):
    return [list(d[8 + 24 * c: 32 + 24 * c]) + list(d[56 + c: flen: 2]) for c in (0, 1)]


def new_state():
    return {"lay": {320: [], 518: []}, "tried": 0, "rescued": 0}


def rescue(frames, state=None):
    """frames: structured records in (channel, time) order.  Returns (records, outcomes, state); outcomes[i] is one of
    'other' (not RS41), 'clean' (both nerr >= 0), 'no_layout', 'too_many' (> 24 erasures), 'undecodable', 'rejected', 'rescued'."""
    state = {} if state is None else state
    out = frames.copy()
    outcomes = []
    for i, f in enumerate(frames):
        flen = int(f["len"])
        if int(f["type"]) != RS41 or flen not in (320, 518):
            outcomes.append("other")
            continue
        st = state.setdefault(int(f["channel"]), new_state())
        d = [int(v) for v in f["data"][:flen]]
        failed = [int(f["nerr"][0]) < 0, int(f["nerr"][1]) < 0]
        if not any(failed):
            lay = walk(d, flen)
            if lay and all(block_ok(d, off, ln) for off, _, ln in lay):
                st["lay"][flen] = lay
            outcomes.append("clean")
            continue
        lay = st["lay"][flen]
        if not lay:
            outcomes.append("no_layout")
            continue
        st["tried"] += 1
        orig = list(d)
        for off, t, ln in lay:                                  # 1. known bytes
            if failed[cw_of(off)]:
                d[off] = t
            if failed[cw_of(off + 1)]:
                d[off + 1] = ln
        bad = [(off, ln) for off, _, ln in lay if not block_ok(d, off, ln)]       # 2.
        n = 24 + (flen - 56) // 2
        er = [[0] * n, [0] * n]
        for off, ln in bad:                                     # 3.
            for o in range(off + 2, off + ln + 4):
                er[(o - 56) & 1][24 + ((o - 56) >> 1)] = 1
        if any(failed[c] and sum(er[c]) > 24 for c in (0, 1)):
            outcomes.append("too_many")
            continue
        cw = split(d, flen)
        ok = True
        for c in (0, 1):                                        # 4.
            if failed[c]:
                stt, cw[c] = rs_decode_ee(cw[c], er[c])
                if stt < 0:
                    ok = False
                    break
        if not ok:
            outcomes.append("undecodable")
            continue
        for c in (0, 1):
            if failed[c]:
                d[8 + 24 * c: 32 + 24 * c] = cw[c][:24]
                d[56 + c: flen: 2] = cw[c][24:]
        if not (all(d[off] == t and d[off + 1] == ln and block_ok(d, off, ln) for off, t, ln in lay)        # 5.
                and not any(any(syndromes(w)) for w in split(d, flen))):
            outcomes.append("rejected")
            continue
        out[i]["data"][:flen] = d                               # 6.
        for c in (0, 1):
            if failed[c]:
                out[i]["nerr"][c] = sum(1 for o in range(8, flen) if cw_of(o) == c and d[o] != orig[o])
        out[i]["flags"] |= FRAME_RESCUED
        st["rescued"] += 1
        outcomes.append("rescued")
    return out, outcomes, state
