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
    """One submit.  groups: [[channel, ...], ...]; chips(channel, start, count) -> the channel's chips or None; offsets: {channel:
    offset in chips} or a sequence indexed by channel (None: zeros).  outcomes[i]: 'other' (not visited), 'good', 'no_partner',
    'partner_good', 'left_out' (step 3: r's chips, or all partners', do not serve), 'combined', 'guard', 'none', 'several'."""
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
            # 2. partners: the nearest candidate within the window, this submit's or the carried one
            partners = []
            for m, ch in enumerate(members):
                if m == m_r:
                    continue
                cands = [out[j] for j in idx[ch]]
                if ch in state["carried"]:
                    cands.append(state["carried"][ch])
                cands = [c for c in cands if int(c["len"]) == LEN and abs(int(c["bitpos"]) - off_of(ch) - t_r) <= window]
                if cands:
                    partners.append(min(cands, key=lambda c: (abs(int(c["bitpos"]) - off_of(ch) - t_r), int(c["bitpos"]))))
            if not partners:
                outcomes[i] = "no_partner"
                continue
            if any(not failed(p) for p in partners):
                outcomes[i] = "partner_good"
                continue
            # 3. blocks from chips
            mine = blocks_of(r, chips)
            theirs = [b for b in (blocks_of(p, chips) for p in partners) if b is not None]
            if mine is None or not theirs:
                outcomes[i] = "left_out"
                continue
            state["tried"][g] += 1
            rec, st = combine(r, [mine] + theirs, **mut)
            outcomes[i] = STATUS.get(st, "combined")
            if st > 0:
                out[i] = rec
                state["combined"][g] += 1
        # the carried records: each member's newest frame record of this submit, as the pass left it
        for ch in members:
            if idx[ch]:
                state["carried"][ch] = out[max(idx[ch], key=lambda i: int(out[i]["bitpos"]))].copy()
    return out, outcomes, state


restart_div_group = dr.restart_group

# ---- the align step (SPEC 3.3k) with the predicates of SPEC 3.3n
new_state, restart_group = da.new_state, da.restart_group


def good(r):
    return is_frame(r) and int(r["nerr"][1]) == 0


def match(x, y):
    return int(x["len"]) == int(y["len"]) == LEN and bytes(x["data"][:LEN]) == bytes(y["data"][:LEN])


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
                pb, pa = max(hits)
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


def run(records, groups, chips, state, mode=LEARN | MARK, window=WINDOW, **mut):
    """One submit as the library runs it: align, the pass over the locked members at the learned offsets, the carried records of the
    unlocked members.  Returns (records after both steps in the same order, outcomes, state)."""
    out = align(records, groups, state, mode)
    lk = state["locked"]
    locked_groups = [[ch for ch in members if lk[ch]] for members in groups]
    out, outcomes, state["div"] = diversity(out, locked_groups, chips, state["off"], window, state["div"], **mut)
    for members in groups:
        for ch in members:
            if not lk[ch]:
                idx = [i for i in range(len(out)) if int(out[i]["channel"]) == ch and is_frame(out[i])]
                if idx:
                    state["div"]["carried"][ch] = out[max(idx, key=lambda i: int(out[i]["bitpos"]))].copy()
    return out, outcomes, state
