"""A Python twin of sonde_batch_set_diversity for iMS-100 groups (SONDE_FLAG_IMS_DIVERSITY, DESIGN SPEC 3.3n), written from the rule alone:
plain Python, codeword membership by polynomial division, the first pass's verdict and codeword by brute force (the primitives of the
SPEC 3.3h twin, ims_rescue_reference.py: poly_mod, first_pass_block, received_blocks, the chips(channel, start, count) callable,
imported and not changed), the hypotheses by plain enumeration; nothing shared with csrc/ims_diversity_kernel.hip.  Test
infrastructure only.

    combine(record, blocks, n)   steps 4 to 7 on caller-made cases: record = copy 0's record, blocks[j][L] = block L of copy j as
                                 received.  Returns (record, status): status = the copies used, -1 (the pairing guard refuses), -2 (a
                                 block of F has no solution), -3 (none has none, one has several).
    diversity(records, groups, chips, offsets, window, state)
                                 one submit: steps 1 and 2 are SPEC 3.3j's with the substitutions of SPEC 3.3n (the shape of
                                 dfm_diversity_reference.diversity; the state and restart_group are diversity_reference's), step 3
                                 from the chips.  Returns (records after the pass in the same order, outcomes per record, state).
    align, run, new_state, restart_group
                                 the align step of SPEC 3.3k with the two predicates of SPEC 3.3n, and one submit as the library
                                 runs it; the state is diversity_align_reference's.

The keyword arguments min_agreed, max_differ, max_dist and cap are MUTATIONS of the rule's four constants, for the tests that show the
designed cases can tell them apart; nothing else may set them."""
from __future__ import annotations

import itertools

import numpy as np

import diversity_align_reference as da
import diversity_reference as dr
import ims_rescue_reference as ir

IMS = ir.IMS
LEN = 51
NBLK, BLK_BITS, DATA_BITS, FRAME_CHIPS = ir.NBLK, ir.BLK_BITS, ir.DATA_BITS, ir.FRAME_CHIPS
FRAME_RESCUED, FRAME_COMBINED, FRAME_DUPLICATE = 2, 4, 8
LEARN, MARK = da.LEARN, da.MARK
MIN_AGREED, MAX_DIFFER, MAX_DIST, CAP = 6, 1, 5, 6
WINDOW = 576
STATUS = {-1: "guard", -2: "none", -3: "several"}


def is_frame(r):
    return int(r["type"]) == IMS and int(r["len"]) == LEN


def failed(r):
    return int(r["nerr"][1]) > 0


def dist(a, b):
    return bin(int(a) ^ int(b)).count("1")


def copies_of(flags):
    return (int(flags) >> 8) & 0xF


def joint(flags):
    """SONDE_FRAME_JOINT"""
    return (int(flags) >> 12) & 0xF


def decode_block(words, *, max_dist=MAX_DIST, cap=CAP):
    """step 5 for one block of F: words[j] = the block as received in copy j (copy 0 rejected it).  Returns (value, how): how = 'taken'
    (a), 'joint' (b), 'none' or 'several' (value None)."""
    first = [ir.first_pass_block(w) for w in words]
    held = [cw for cw, n in first[1:] if n >= 0]
    if held:
        count = {v: held.count(v) for v in set(held)}
        top = max(count.values())
        tops = [v for v, n in count.items() if n == top]
        if len(tops) > 1:
            return None, "several"
        v = tops[0]
        lost = [w for w, (_, n) in zip(words, first) if n < 0]
        return (v, "taken") if all(dist(w, v) <= max_dist for w in lost) else (None, "none")
    K = len(words)
    w, V = 0, []
    for i in range(BLK_BITS):
        ones = sum((x >> i) & 1 for x in words)
        if 2 * ones == K:
            V.append(i)
            w |= ((words[0] >> i) & 1) << i
        else:
            w |= (1 if 2 * ones > K else 0) << i
    if not V:
        cw, n = ir.first_pass_block(w)
        return (cw, "joint") if n >= 0 else (None, "none")
    if len(V) > cap:
        return None, "none"
    fits = []
    for k in range(len(V) + 1):
        for sub in itertools.combinations(V, k):
            h = w
            for i in sub:
                h ^= 1 << i
            if ir.poly_mod(h) == 0:
                fits.append(h)
    if len(fits) == 1:
        return fits[0], "joint"
    return None, ("several" if fits else "none")


def combine(record, blocks, n=None, *, min_agreed=MIN_AGREED, max_differ=MAX_DIFFER, max_dist=MAX_DIST, cap=CAP):
    K = len(blocks) if n is None else int(n)
    x = [[int(b) for b in blocks[j]] for j in range(K)]
    first = [[ir.first_pass_block(b) for b in c] for c in x]
    # 4. pairing guard
    A = [L for L in range(NBLK) if all(c[L][1] >= 0 for c in first)]
    D = [L for L in A if any(c[L][0] != first[0][L][0] for c in first)]
    if len(A) < min_agreed or len(D) > max_differ:
        return record.copy(), -1
    # 5., 6.
    F = [L for L in range(NBLK) if first[0][L][1] < 0]
    got = {L: decode_block([c[L] for c in x], max_dist=max_dist, cap=cap) for L in F}
    if any(how == "none" for _, how in got.values()):
        return record.copy(), -2
    if any(how == "several" for _, how in got.values()):
        return record.copy(), -3
    # 7.
    out = record.copy()
    for L in F:
        for b in range(DATA_BITS):
            k = DATA_BITS * L + b
            bit = (got[L][0] >> (BLK_BITS - 1 - b)) & 1
            out["data"][k >> 3] = (int(out["data"][k >> 3]) & ~(0x80 >> (k & 7))) | (bit << (7 - (k & 7)))
    out["nerr"][0] += sum(dist(got[L][0], x[0][L]) for L in F)
    out["nerr"][1] = 0
    J = sum(1 for _, how in got.values() if how == "joint")
    out["flags"] |= FRAME_RESCUED | FRAME_COMBINED | (K << 8) | (min(J, 15) << 12)
    return out, K


def blocks_of(r, chips):
    """step 3 for one copy: its 12 received blocks from its own channel's chips, or None -- the chips are no longer held, or the number
    of blocks the first pass rejects among them is not the record's nerr[1]"""
    fc = chips(int(r["channel"]), int(r["bitpos"]), FRAME_CHIPS)
    if fc is None:
        return None
    blocks = ir.received_blocks(np.asarray(fc, dtype=np.uint8))
    if sum(1 for b in blocks if ir.first_pass_rejects(b)) != int(r["nerr"][1]):
        return None
    return blocks


new_div_state = dr.new_state


def diversity(records, groups, chips, offsets=None, window=WINDOW, state=None, **mut):
    """One submit: diversity_reference.diversity on is_frame, failed and STATUS above, with step 3 in front of combine.  groups:
    [[channel, ...], ...]; chips(channel, start, count) -> the channel's chips or None; offsets: {channel: offset in chips} or a
    sequence indexed by channel (None: zeros).  outcomes[i]: 'other' (not visited), 'good', 'no_partner', 'partner_good', 'left_out'
    (step 3: r's chips, or all partners', do not serve), 'combined', 'guard', 'none', 'several'."""
    def attempt(r, partners):
        # 3. blocks from chips
        mine = blocks_of(r, chips)
        theirs = [b for b in (blocks_of(p, chips) for p in partners) if b is not None]
        return None if mine is None or not theirs else combine(r, [mine] + theirs, **mut)

    return dr.diversity(records, groups, offsets, window, state, is_frame=is_frame, failed=failed, attempt=attempt, status=STATUS)


restart_div_group = dr.restart_group

# ---- the align step (SPEC 3.3k) with the predicates of SPEC 3.3n
new_state, restart_group = da.new_state, da.restart_group


def good(r):
    return is_frame(r) and int(r["nerr"][1]) == 0


def match(x, y):
    return int(x["len"]) == int(y["len"]) == LEN and bytes(x["data"][:LEN]) == bytes(y["data"][:LEN])


def align(records, groups, state, mode):
    """diversity_align_reference.align on `good` and `match` above"""
    return da.align(records, groups, state, mode, good=good, match=match)


def run(records, groups, chips, state, mode=LEARN | MARK, window=WINDOW, **mut):
    """One submit as the library runs it (diversity_align_reference.run): align, the pass over the locked members at the learned
    offsets, the carried records of the unlocked members.  Returns (records after both steps in the same order, outcomes, state)."""
    def div(out, locked_groups, off, window, state):
        return diversity(out, locked_groups, chips, off, window, state, **mut)

    return da.run(records, groups, state, mode, window, good=good, match=match, diversity=div, is_frame=is_frame)
