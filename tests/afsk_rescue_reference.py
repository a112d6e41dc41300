"""The twin of SONDE_FLAG_AFSK_RESCUE (DESIGN SPEC 3.3i), written from the SPEC text alone: plain Python, brute force (apply a
pattern, recompute the whole check), no syndrome, no column, no code shared with csrc/afsk_rescue_kernel.hip.  Test infrastructure only.

    records, outcomes, state = rescue(records, state)

records: FRAME_DTYPE array (not modified; a changed copy is returned); state: {channel: {"tried", "rescued"}}, carried from call to
call.  outcomes[i] is one of OUTCOMES for records[i]:
    other      not an iMet / C50 record of a length the pass knows
    clean      the check passed in the first pass
    rescued    exactly one pattern fits: applied
    unsolved   no pattern fits (more damage than one pattern, or damage in a byte that is no candidate)
    ambiguous  several patterns fit: the record stays

The keyword arguments behind `state` are MUTATIONS of the rule, for the tests that show the designed scenes can tell them apart;
nothing else may set them."""
from __future__ import annotations

import numpy as np

IMET4, C50 = 4, 5
FRAME_RESCUED = 2
OUTCOMES = ("other", "clean", "unsolved", "ambiguous", "rescued")
STATUS = {"other": 0, "clean": 0, "unsolved": 0, "rescued": 1, "ambiguous": 2}     # what sonde_batch_test_afsk_repair reports


def _crc_table():
    tab = np.zeros(256, dtype=np.uint32)
    for b in range(256):
        crc = b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
        tab[b] = crc
    return tab


_CRC_TAB = _crc_table()


def check_passes(kind, trials, ln):
    """SPEC step 4 for many trial packets at once: trials [P, >= ln] uint8 -> bool [P], the check of the record type over each row"""
    t = np.asarray(trials, dtype=np.uint32)
    if kind == IMET4:
        crc = np.full(len(t), 0x1D0F, dtype=np.uint32)
        for i in range(ln - 2):
            crc = ((crc << 8) & 0xFFFF) ^ _CRC_TAB[(crc >> 8) ^ t[:, i]]
        return crc == ((t[:, ln - 2] << 8) | t[:, ln - 1])
    c1 = np.zeros(len(t), dtype=np.uint32)
    c2 = np.zeros(len(t), dtype=np.uint32)
    for i in range(2, 7):
        c1 = (c1 + t[:, i]) & 0xFF
        c2 = (c2 + c1) & 0xFF
    return (c1 == t[:, 7]) & (c2 == t[:, 8])


def first_candidate(kind, data):
    """SPEC step 2: the first byte the search may touch"""
    if kind == IMET4:
        return 3 if int(data[1]) == 3 else 2
    return 2


def patterns(pairs=True):
    """SPEC step 3: the masks of one byte, singles first"""
    return [1 << j for j in range(8)] + ([3 << j for j in range(7)] if pairs else [])


def new_state():
    return {"tried": 0, "rescued": 0}


def eligible(kind, ln):
    return (kind == IMET4 and 5 <= ln <= 64) or (kind == C50 and ln == 9)


def rescue(records, state=None, *, first_fit=False, pairs=True, touch_header=False):
    state = {c: dict(v) for c, v in (state or {}).items()}
    out = records.copy()
    outcomes = []
    for f in out:
        kind, ln, ch = int(f["type"]), int(f["len"]), int(f["channel"])
        if not eligible(kind, ln):
            outcomes.append("other")
            continue
        if int(f["nerr"][0]) != -1:
            outcomes.append("clean")
            continue
        st = state.setdefault(ch, new_state())
        st["tried"] += 1
        data = np.array(f["data"][:ln], dtype=np.uint8)
        cand = [(i, m) for i in range(0 if touch_header else first_candidate(kind, data), ln) for m in patterns(pairs)]
        trials = np.tile(data, (len(cand), 1))
        for k, (i, m) in enumerate(cand):
            trials[k, i] ^= m
        fits = [cand[k] for k in np.nonzero(check_passes(kind, trials, ln))[0]]
        if not fits:
            outcomes.append("unsolved")
            continue
        if len(fits) > 1 and not first_fit:
            outcomes.append("ambiguous")
            continue
        i, m = fits[0]
        f["data"][i] ^= m
        f["nerr"][0] = 0
        f["flags"] |= FRAME_RESCUED | (bin(m).count("1") << 8)
        st["rescued"] += 1
        outcomes.append("rescued")
    return out, outcomes, state
