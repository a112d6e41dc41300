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
    """One submit: diversity_reference.diversity on is_frame, failed, combine and STATUS above.  groups: [[channel, ...], ...]; offsets:
    {channel: offset_bits} or a sequence indexed by channel (None: zeros).  outcomes[i]: 'other' (not visited), 'good', 'no_partner',
    'partner_good', 'combined', 'not_attempted', 'no_fit', 'several_fit'."""
    return dr.diversity(records, groups, offsets, window, state, is_frame=is_frame, failed=failed,
                        attempt=lambda r, partners: combine([r] + partners), status=STATUS)


restart_div_group = dr.restart_group

# ---- the align step (SPEC 3.3k) with the predicates of SPEC 3.3l
new_state, restart_group = da.new_state, da.restart_group


def good(r):
    return is_frame(r) and not failed(r)


def match(x, y):
    n = int(x["len"])
    return n == int(y["len"]) and bytes(x["data"][:n]) == bytes(y["data"][:n])


def align(records, groups, state, mode):
    """diversity_align_reference.align on `good` and `match` above"""
    return da.align(records, groups, state, mode, good=good, match=match)


def run(records, groups, state, mode=LEARN | MARK, window=960):
    """One submit as the library runs it (diversity_align_reference.run): align, the pass over the locked members at the learned
    offsets, the carried records of the unlocked members.  Returns (records after both steps in the same order, outcomes, state)."""
    return da.run(records, groups, state, mode, window, good=good, match=match, diversity=diversity, is_frame=is_frame)
