"""A Python twin of the align step of sonde_batch_set_diversity_auto (DESIGN SPEC 3.3k), written from the rule alone, on top of the
twin of the combining pass (tests/diversity_reference.py, which it imports and does not change).

    align(records, groups, state, mode)   the step over the records of one submit: learns offsets and locks (mode & LEARN), marks
                                          duplicates (mode & MARK).  Returns the records (same order) with their flags.
    run(records, groups, state, mode, window)
                                          one submit as the library runs it: align, then diversity_reference.diversity over the locked
                                          members at the learned offsets, then the carried records of the unlocked members.
    new_state(groups, offsets, mode)      what set_diversity leaves; restart_group(state, groups, g): what a restart leaves.

The step is the same for every kind of group: the twins of the other kinds call align and run with their own good and match, and run
with their own diversity and is_frame.

state: {'off': {ch: int}, 'locked': {ch: bool}, 'learned': [per group], 'duplicates': [per group], 'div': the combining twin's state
(carried records by channel, tried / combined per group), 'initial': (offsets or None, unlocked)}."""
from __future__ import annotations

import diversity_reference as dr

LEARN, MARK = 1, 2
FRAME_DUPLICATE = 8
LENGTHS = dr.LENGTHS
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def new_state(groups, offsets=None, mode=0):
    unlocked = bool(mode & LEARN) and offsets is None
    members = [ch for g in groups for ch in g]
    return {"off": {ch: 0 if offsets is None else int(offsets[ch]) for ch in members}, "locked": {ch: not unlocked for ch in members},
            "learned": [0] * len(groups), "duplicates": [0] * len(groups), "div": dr.new_state(groups),
            "initial": (None if offsets is None else {ch: int(offsets[ch]) for ch in members}, unlocked)}


def restart_group(state, groups, g):
    """what sonde_batch_restart_channels does to a group it lists"""
    dr.restart_group(state["div"], groups, g)
    offsets, unlocked = state["initial"]
    for ch in groups[g]:
        state["off"][ch] = 0 if offsets is None else offsets[ch]
        state["locked"][ch] = not unlocked
    state["learned"][g] = state["duplicates"][g] = 0


def good(r):
    return dr.is_frame(r) and not dr.failed(r)


def match(x, y):
    n = int(x["len"])
    return n == int(y["len"]) and bytes(x["data"][8:n]) == bytes(y["data"][8:n])


def align(records, groups, state, mode, *, good=good, match=match):
    out = records.copy()
    carried = state["div"]["carried"]
    for g, members in enumerate(groups):
        now = {ch: [i for i in range(len(out)) if int(out[i]["channel"]) == ch and good(out[i])] for ch in members}
        old = {ch: carried[ch] for ch in members if ch in carried and good(carried[ch])}
        if mode & LEARN:
            for a, b in PAIRS:
                if b >= len(members):
                    continue
                ca, cb = members[a], members[b]
                cand_a = [out[i] for i in now[ca]] + ([old[ca]] if ca in old else [])
                cand_b = [out[i] for i in now[cb]] + ([old[cb]] if cb in old else [])
                hits = [(int(y["bitpos"]), int(x["bitpos"])) for x in cand_a for y in cand_b if match(x, y)]
                if not hits:
                    continue
                pb, pa = max(hits)                       # the latest in b; of several, the latest in a
                d = pb - pa
                off, lk = state["off"], state["locked"]
                if lk[cb] and not lk[ca]:
                    off[ca] = off[cb] - d
                    state["learned"][g] += 1
                elif not (lk[ca] and lk[cb]) or off[cb] - off[ca] != d:
                    off[cb] = off[ca] + d
                    state["learned"][g] += 1
                lk[ca] = lk[cb] = True
        if mode & MARK:
            for b, cb in enumerate(members):
                for i in now[cb]:
                    dup = any(match(old[ca], out[i]) for ca in members if ca != cb and ca in old)
                    dup = dup or any(match(out[k], out[i]) for ca in members[:b] for k in now[ca])
                    if dup:
                        out[i]["flags"] |= FRAME_DUPLICATE
                        state["duplicates"][g] += 1
    return out


def run(records, groups, state, mode=LEARN | MARK, window=960, *, good=good, match=match, diversity=dr.diversity, is_frame=dr.is_frame):
    """One submit.  Returns (records after both steps in the same order, the combining twin's outcomes, state)."""
    out = align(records, groups, state, mode, good=good, match=match)
    lk = state["locked"]
    locked_groups = [[ch for ch in members if lk[ch]] for members in groups]
    # an unlocked member is to the combining pass a member without records: it is not in the group the twin sees
    out, outcomes, state["div"] = diversity(out, locked_groups, state["off"], window, state["div"])
    for members in groups:
        for ch in members:
            if not lk[ch]:                               # its carried record is kept up to date all the same
                idx = [i for i in range(len(out)) if int(out[i]["channel"]) == ch and is_frame(out[i])]
                if idx:
                    state["div"]["carried"][ch] = out[max(idx, key=lambda i: int(out[i]["bitpos"]))].copy()
    return out, outcomes, state
