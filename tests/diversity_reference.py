"""A Python twin of sonde_batch_set_diversity (DESIGN SPEC 3.3j), written from the rule alone on the primitives of the SPEC 3.3c twin
(tests/rescue_reference.py: the textbook errors-and-erasures RS(255,231) decoder, the block CRC, the chain walk).

    combine(copies, n_copies)  steps 3 to 7 on caller-made records: copy 0 is the record to rewrite.  Returns (record, status):
                               status = the copies used, -1 (more than 24 erasures), -2 (no decode), -3 (rejected).
    diversity(records, groups, offsets, window, state)
                               one submit: `records` are its frame records (any order), `state` carries the members' carried
                               records and the groups' counters from call to call.  Returns (records after the pass in the same
                               order, outcomes per record, state).  Steps 1 and 2 are the same for every kind of group: the twins
                               of the other kinds (check_, dfm_ and ims_diversity_reference.py) call it with their own is_frame,
                               failed, attempt and status names.

Nothing here is shared with the library: the tests compare whole records byte for byte."""
from __future__ import annotations

import numpy as np

from rescue_reference import block_ok, cw_of, rs_decode_ee, split, syndromes, walk

RS41 = 0
FRAME_RESCUED, FRAME_COMBINED = 2, 4
LENGTHS = (320, 518)


def pos_of(o):
    """position of frame byte o in its codeword"""
    return (o - 8) % 24 if o < 56 else 24 + ((o - 56) >> 1)


def combine(copies, n_copies=None):
    """copies: K records (structured, FRAME_DTYPE), copy 0 first.  Steps 3 to 7, and step 8's record."""
    K = len(copies) if n_copies is None else int(n_copies)
    copies = [copies[k] for k in range(K)]
    r = copies[0]
    flen = int(r["len"])
    d = [[int(v) for v in c["data"][:flen]] for c in copies]
    failed = [int(r["nerr"][c]) < 0 for c in (0, 1)]
    work = list(d[0])
    # 3. whole codewords
    settled = [None, None]
    for c in (0, 1):
        if not failed[c]:
            continue
        for j in range(1, K):
            if int(copies[j]["nerr"][c]) >= 0 and not any(syndromes(split(d[j], flen)[c])):
                settled[c] = j
                break
        if settled[c] is not None:
            for o in range(8, flen):
                if cw_of(o) == c:
                    work[o] = d[settled[c]][o]
    is_open = [failed[c] and settled[c] is None for c in (0, 1)]
    # 4. trusted blocks: one walk over all copies
    claimed = {}
    off, nb = 57, 0
    while off + 4 <= flen and nb < 16:
        lens = []
        for j in range(K):
            ln = d[j][off + 1]
            if ln not in lens and off + ln + 4 <= flen:
                lens.append(ln)
        if not lens:
            break
        hit = next(((ln, j) for ln in lens for j in range(K) if block_ok(d[j], off, ln)), None)
        if hit:
            ln, j = hit
            for o in range(off + 1, off + ln + 4):
                claimed[o] = d[j][o]
        else:
            ln = lens[0]
        off += ln + 4
        nb += 1
    # 5. votes
    n = 24 + (flen - 56) // 2
    er = [[0] * n, [0] * n]
    for o in range(8, flen):
        c = cw_of(o)
        if not is_open[c]:
            continue
        if o in claimed:
            work[o] = claimed[o]
            continue
        vals = [d[j][o] for j in range(K)]
        best = max(set(vals), key=vals.count)
        if 2 * vals.count(best) > K:
            work[o] = best
        else:
            er[c][pos_of(o)] = 1
    # 6. decode
    if any(is_open[c] and sum(er[c]) > 24 for c in (0, 1)):
        return r.copy(), -1
    cw = split(work, flen)
    for c in (0, 1):
        if is_open[c]:
            st, cw[c] = rs_decode_ee(cw[c], er[c])
            if st < 0:
                return r.copy(), -2
            work[8 + 24 * c: 32 + 24 * c] = cw[c][:24]
            work[56 + c: flen: 2] = cw[c][24:]
    # 7. accept
    if any(any(syndromes(w)) for w in split(work, flen)):
        return r.copy(), -3
    lay = walk(work, flen)
    if not lay or not all(block_ok(work, o, ln) for o, _, ln in lay):
        return r.copy(), -3
    # 8. record
    out = r.copy()
    out["data"][:flen] = work
    for c in (0, 1):
        if failed[c]:
            out["nerr"][c] = sum(1 for o in range(8, flen) if cw_of(o) == c and work[o] != d[0][o])
    out["flags"] |= FRAME_RESCUED | FRAME_COMBINED | (K << 8)
    return out, K


def new_state(groups):
    return {"carried": {}, "tried": [0] * len(groups), "combined": [0] * len(groups)}


def is_frame(r):
    return int(r["len"]) in LENGTHS


def failed(r):
    return int(r["nerr"][0]) < 0 or int(r["nerr"][1]) < 0


STATUS = {-1: "too_many", -2: "undecodable", -3: "rejected"}


def diversity(records, groups, offsets=None, window=960, state=None, *, is_frame=is_frame, failed=failed,
              attempt=lambda r, partners: combine([r] + partners), status=STATUS):
    """One submit.  groups: [[channel, ...], ...]; offsets: {channel: offset_bits} or a sequence indexed by channel (None: zeros).
    outcomes[i]: 'other' (not visited), 'good', 'no_partner', 'partner_good', 'combined', or what `status` names: 'too_many',
    'undecodable', 'rejected'.  The kind of the groups: is_frame(r) and failed(r) on a record, attempt(r, partners) -> (record, status)
    as combine gives them, or None: nothing is tried and the record does not count ('left_out')."""
    state = new_state(groups) if state is None else state
    off_of = (lambda ch: 0) if offsets is None else (lambda ch: int(offsets[ch]))
    out = records.copy()
    outcomes = ["other"] * len(out)
    for g, members in enumerate(groups):
        idx = {ch: [i for i in range(len(out)) if int(out[i]["channel"]) == ch and is_frame(out[i])] for ch in members}
        t_of = lambda i, ch: int(out[i]["bitpos"]) - off_of(ch)             # noqa: E731
        # 1. visit in ascending t, ties in member order
        for t_r, m_r, i in sorted((t_of(i, ch), m, i) for m, ch in enumerate(members) for i in idx[ch]):
            r = out[i]
            if not failed(r):
                outcomes[i] = "good"
                continue
            # 2. partners: the nearest candidate of the same len within the window, this submit's or the carried one
            partners = []
            for m, ch in enumerate(members):
                if m == m_r:
                    continue
                cands = [out[j] for j in idx[ch]]
                if ch in state["carried"]:
                    cands.append(state["carried"][ch])
                cands = [c for c in cands if int(c["len"]) == int(r["len"]) and abs(int(c["bitpos"]) - off_of(ch) - t_r) <= window]
                if cands:
                    partners.append(min(cands, key=lambda c: (abs(int(c["bitpos"]) - off_of(ch) - t_r), int(c["bitpos"]))))
            if not partners:
                outcomes[i] = "no_partner"
                continue
            if any(not failed(p) for p in partners):
                outcomes[i] = "partner_good"
                continue
            got = attempt(r, partners)
            if got is None:
                outcomes[i] = "left_out"
                continue
            state["tried"][g] += 1
            rec, st = got
            outcomes[i] = status.get(st, "combined")
            if st > 0:
                out[i] = rec
                state["combined"][g] += 1
        # the carried records: each member's newest frame record of this submit, as the pass left it
        for ch in members:
            if idx[ch]:
                state["carried"][ch] = out[max(idx[ch], key=lambda i: int(out[i]["bitpos"]))].copy()
    return out, outcomes, state


def restart_group(state, groups, g):
    """what sonde_batch_restart_channels does to a group it lists"""
    for ch in groups[g]:
        state["carried"].pop(ch, None)
    state["tried"][g] = state["combined"][g] = 0
