"""A Python twin of sonde_batch_set_diversity for M10 / M20 and MRZ-N1 groups (DESIGN SPEC 3.3l), written from the rule alone: plain
Python, subsets by plain enumeration, nothing shared with csrc/check_diversity_kernel.hip.  Test infrastructure only.

    combine(copies, n)         steps 3 to 6 on caller-made records: copy 0 is the record to rewrite.  Returns (record, status):
                               status = the copies used, -1 (not attempted: no unknown, more than 8, length byte in doubt), -2 (no
                               subset fits), -3 (several fit).
    diversity(records, groups, offsets, window, state)
                               one submit: steps 1 and 2 are SPEC 3.3j's with the four substitutions of SPEC 3.3l (the shape of
                               diversity_reference.diversity, whose state -- carried records by channel, tried / combined per group --
                               and restart_group serve here unchanged).  Returns (records after the pass in the same order, outcomes
                               per record, state).
    align(records, groups, state, mode), run(records, groups, state, mode, window), new_state, restart_group
                               the align step of SPEC 3.3k with the two predicates of SPEC 3.3l, and one submit as the library runs
                               it; the state is diversity_align_reference's.

The check and column primitives are those of the SPEC 3.3f twin (manchester_rescue_reference.py), imported and not changed.  A record's
kind is its own `type` field: a group's members are of one type."""
from __future__ import annotations

import numpy as np

import diversity_align_reference as da
import diversity_reference as dr
import manchester_rescue_reference as mr

M10, MRZN1 = mr.M10, mr.MRZN1
FRAME_RESCUED, FRAME_COMBINED, FRAME_DUPLICATE = 2, 4, 8
LEARN, MARK = da.LEARN, da.MARK
CAP = 8
LENGTHS = {M10: (101, 70), MRZN1: (45,)}
STATUS = {-1: "not_attempted", -2: "no_fit", -3: "several_fit"}


def is_frame(r):
    return int(r["len"]) in LENGTHS.get(int(r["type"]), ())


def failed(r):
    return int(r["nerr"][0]) < 0


def unknowns(flags):
    """SONDE_FRAME_UNKNOWNS"""
    return (int(flags) >> 12) & 0xF


def working_frame(copies):
    """step 3: (w as bits, V ascending) of K records of one type and length"""
    K = len(copies)
    ln = int(copies[0]["len"])
    bits = [np.unpackbits(np.asarray(c["data"][:ln], dtype=np.uint8)) for c in copies]      # MSB first
    ones = np.sum(bits, axis=0)
    w = np.where(2 * ones > K, 1, np.where(2 * (K - ones) > K, 0, bits[0])).astype(np.uint8)
    V = [int(k) for k in np.nonzero((ones != 0) & (ones != K))[0]]
    return w, V


def combine(copies, n=None):
    K = len(copies) if n is None else int(n)
    copies = [copies[k] for k in range(K)]
    r = copies[0]
    kind, ln = int(r["type"]), int(r["len"])
    w, V = working_frame(copies)
    # 4. majority alone
    s = mr.syndrome(kind, np.packbits(w), ln)
    if not (s == 0 and len(V) >= 1):
        # 5. solve
        if len(V) == 0 or len(V) > CAP or (kind == M10 and V[0] < 8):
            return r.copy(), -1
        cols = [mr.column(kind, ln, k) for k in V]
        sols = []
        for m in range(1, 1 << len(V)):
            x = 0
            for j, cj in enumerate(cols):
                if (m >> j) & 1:
                    x ^= cj
            if x == s:
                sols.append(m)
        if len(sols) != 1:
            return r.copy(), (-3 if sols else -2)
        for j, k in enumerate(V):
            if (sols[0] >> j) & 1:
                w[k] ^= 1
    # 6. record
    out = r.copy()
    out["data"][:ln] = np.packbits(w)
    out["nerr"][0] = 0
    out["flags"] |= FRAME_RESCUED | FRAME_COMBINED | (K << 8) | (min(len(V), 15) << 12)
    return out, K


new_div_state = dr.new_state


def diversity(records, groups, offsets=None, window=960, state=None):
    """One submit.  groups: [[channel, ...], ...]; offsets: {channel: offset_bits} or a sequence indexed by channel (None: zeros).
    outcomes[i]: 'other' (not visited), 'good', 'no_partner', 'partner_good', 'combined', 'not_attempted', 'no_fit', 'several_fit'."""
    state = dr.new_state(groups) if state is None else state
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
            state["tried"][g] += 1
            rec, st = combine([r] + partners)
            outcomes[i] = STATUS.get(st, "combined")
            if st > 0:
                out[i] = rec
                state["combined"][g] += 1
        # the carried records: each member's newest record of this submit with a length of its type, as the pass left it
        for ch in members:
            if idx[ch]:
                state["carried"][ch] = out[max(idx[ch], key=lambda i: int(out[i]["bitpos"]))].copy()
    return out, outcomes, state


restart_div_group = dr.restart_group

# ---- the align step (SPEC 3.3k) with the predicates of SPEC 3.3l
new_state, restart_group = da.new_state, da.restart_group


def good(r):
    return is_frame(r) and not failed(r)


def match(x, y):
    n = int(x["len"])
    return n == int(y["len"]) and bytes(x["data"][:n]) == bytes(y["data"][:n])


def align(records, groups, state, mode):
    """diversity_align_reference.align, rule for rule, on `good` and `match` above"""
    out = records.copy()
    carried = state["div"]["carried"]
    for g, members in enumerate(groups):
        now = {ch: [i for i in range(len(out)) if int(out[i]["channel"]) == ch and good(out[i])] for ch in members}
        old = {ch: carried[ch] for ch in members if ch in carried and good(carried[ch])}
        if mode & LEARN:
            for a, b in da.PAIRS:
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


def run(records, groups, state, mode=LEARN | MARK, window=960):
    """One submit as the library runs it: align, the pass over the locked members at the learned offsets, the carried records of the
    unlocked members.  Returns (records after both steps in the same order, outcomes, state)."""
    out = align(records, groups, state, mode)
    lk = state["locked"]
    locked_groups = [[ch for ch in members if lk[ch]] for members in groups]
    out, outcomes, state["div"] = diversity(out, locked_groups, state["off"], window, state["div"])
    for members in groups:
        for ch in members:
            if not lk[ch]:
                idx = [i for i in range(len(out)) if int(out[i]["channel"]) == ch and is_frame(out[i])]
                if idx:
                    state["div"]["carried"][ch] = out[max(idx, key=lambda i: int(out[i]["bitpos"]))].copy()
    return out, outcomes, state
