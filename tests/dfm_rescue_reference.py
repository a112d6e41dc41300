"""The twin of SONDE_FLAG_DFM_RESCUE (DESIGN SPEC 3.3g), written from the SPEC text alone: plain Python, the word decoder a search
over the 16 encoded nibbles, no code shared with csrc/dfm_rescue_kernel.hip.  Test infrastructure only.

    records, outcomes, state = rescue(records, chips, state)

records: FRAME_DTYPE array (not modified; a changed copy is returned); chips(channel, start, count) -> uint8 array of the
channel's on-air chips [start, start + count), or None when they are no longer available (SPEC step 3, second case); state: {channel:
{"tried", "rescued"}}, carried from call to call.  outcomes[i] is one of OUTCOMES for records[i].

The keyword arguments behind `state` are MUTATIONS of the rule, for the tests that show the designed scenes can tell them apart;
nothing else may set them."""
from __future__ import annotations

import numpy as np

DFM = 1
FRAME_RESCUED = 2
CAP = 8
FRAME_CHIPS = 560
ROWS = (0x78, 0xB4, 0xD2, 0xE1)
OUTCOMES = ("other", "clean", "no_chips", "too_many", "unsolved", "rescued")


def _encode(nib):
    """the codeword of a data nibble: the nibble in the high half, each parity bit closing one of ROWS"""
    w = nib << 4
    for k, row in enumerate(ROWS):
        if bin(w & row & 0xF0).count("1") & 1:
            w |= 8 >> k
    return w


CODEWORDS = tuple(_encode(n) for n in range(16))


def syndrome(word):
    return tuple(bin(int(word) & row).count("1") & 1 for row in ROWS)


def decode_word(word, erased, *, bound=3):
    """SPEC step 4 for one word: the codeword that differs from `word` in v positions outside `erased` with 2 v + e <= bound, or None.
    (bound = 3: at most one by the distance of the code; a mutated bound takes the first.)"""
    word, erased = int(word), int(erased)
    e = bin(erased).count("1")
    if e == 0 or e > 3:
        return None
    for cw in CODEWORDS:
        v = bin((cw ^ word) & ~erased & 0xFF).count("1")
        if 2 * v + e <= bound:
            return cw
    return None


def frame_bit(i, j, *, stride_of_block0=False):
    """the frame bit (0..263 behind the sync) that holds bit j (0 = MSB) of codeword i: SPEC step 1"""
    if i < 7:
        off, n, k = 0, 7, i
    elif i < 20:
        off, n, k = 56, 13, i - 7
    else:
        off, n, k = 160, 13, i - 20
    if stride_of_block0:
        n = 7
    return off + j * n + k


def new_state():
    return {"tried": 0, "rescued": 0}


def erasures(frame_chips, i, *, second_chip=False, **il_kw):
    """E_i of SPEC step 4 from the 560 chips of the frame"""
    E = 0
    for j in range(8):
        c = 32 + 2 * frame_bit(i, j, **il_kw) + (1 if second_chip else 0)
        if c + 1 < len(frame_chips) and frame_chips[c] == frame_chips[c + 1]:
            E |= 0x80 >> j
    return E


def received_word(frame_chips, i, inverted):
    w = 0
    for j in range(8):
        w |= (int(frame_chips[32 + 2 * frame_bit(i, j)]) ^ inverted) << (7 - j)
    return w


def rescue(records, chips, state=None, *, bound=3, partial_write=False, second_chip=False, stride_of_block0=False, cap=CAP,
           reopen_corrected=False):
    state = {c: dict(v) for c, v in (state or {}).items()}
    out = records.copy()
    outcomes = []
    for f in out:
        ch = int(f["channel"])
        if int(f["type"]) != DFM or int(f["len"]) != 33:
            outcomes.append("other")
            continue
        visit = int(f["nerr"][1]) >= 1 or (reopen_corrected and int(f["nerr"][0]) >= 1)
        if not visit:
            outcomes.append("clean")
            continue
        p = int(f["bitpos"])
        fc = chips(ch, p, FRAME_CHIPS)
        words = [int(b) for b in f["data"][:33]]
        if reopen_corrected and fc is not None:              # MUTATION: work on what was received, corrected words included
            words = [received_word(fc, i, int(f["flags"]) & 1) for i in range(33)]
        F = [i for i in range(33) if any(syndrome(words[i]))]
        if not F:
            outcomes.append("clean")
            continue
        if cap is not None and len(F) > cap:
            outcomes.append("too_many")
            continue
        if fc is None:
            outcomes.append("no_chips")
            continue
        fc = np.asarray(fc, dtype=np.uint8)
        assert fc.shape == (FRAME_CHIPS,)
        st = state.setdefault(ch, new_state())
        st["tried"] += 1
        decoded = {i: decode_word(words[i], erasures(fc, i, second_chip=second_chip, stride_of_block0=stride_of_block0), bound=bound) for i in F}
        good = [i for i in F if decoded[i] is not None]
        if len(good) < len(F) and not (partial_write and good):
            outcomes.append("unsolved")
            continue
        for i in good:
            f["data"][i] = decoded[i]
        f["nerr"][0] += len(good)
        f["nerr"][1] = 0
        f["flags"] |= FRAME_RESCUED | ((len(good) & 0xF) << 8)
        st["rescued"] += 1
        outcomes.append("rescued")
    return out, outcomes, state


def chips_of_streams(streams):
    """a chips getter over whole recorded chip streams: streams[channel] = uint8 array from chip 0"""
    def get(channel, start, count):
        s = streams[channel]
        return s[start:start + count] if start + count <= len(s) else None
    return get
