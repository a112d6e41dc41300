"""A Python twin of sonde_batch_set_diversity for DFM groups (DESIGN SPEC 3.3m), written from the rule alone: plain Python, the word
decoder a search over the 16 encoded nibbles, nothing shared with csrc/dfm_diversity_kernel.hip.  Test infrastructure only.

    combine(copies, n)         steps 3 to 6 on caller-made records: copy 0 is the record to rewrite.  Returns (record, status):
                               status = the copies used, -1 (the pairing guard refuses), -2 (a word of F has no solution), -3 (none
                               has none, one has several).
    diversity(records, groups, offsets, window, state)
                               one submit: steps 1 and 2 are SPEC 3.3j's with the substitutions of SPEC 3.3m (the shape of
                               check_diversity_reference.diversity; the state -- carried records by channel, tried / combined per
                               group -- and restart_group are diversity_reference's).  Returns (records after the pass in the same
                               order, outcomes per record, state).
    align(records, groups, state, mode), run(records, groups, state, mode, window), new_state, restart_group
                               the align step of SPEC 3.3k with the two predicates of SPEC 3.3m, and one submit as the library runs
                               it; the state is diversity_align_reference's.

The Hamming primitives (the 16 codewords, the syndrome) are those of the SPEC 3.3g twin (dfm_rescue_reference.py), imported and not
changed."""
from __future__ import annotations

import diversity_align_reference as da
import diversity_reference as dr
import dfm_rescue_reference as dfr

DFM = dfr.DFM
WORDS = 33
FRAME_RESCUED, FRAME_COMBINED, FRAME_DUPLICATE = 2, 4, 8
LEARN, MARK = da.LEARN, da.MARK
MIN_AGREED, MAX_DIFFER = 17, 2
CODEWORDS = dfr.CODEWORDS
STATUS = {-1: "guard", -2: "none", -3: "several"}


def is_frame(r):
    return int(r["type"]) == DFM and int(r["len"]) == WORDS


def failed(r):
    return int(r["nerr"][1]) > 0


def is_codeword(b):
    return not any(dfr.syndrome(b))


def dist(a, b):
    return bin((int(a) ^ int(b)) & 0xFF).count("1")


def joint(flags):
    """SONDE_FRAME_JOINT"""
    return (int(flags) >> 12) & 0xF


def guard(x):
    """step 3: (|A|, |D|) of the copies' words x[j][i]"""
    A = [i for i in range(WORDS) if all(is_codeword(c[i]) for c in x)]
    D = [i for i in A if any(c[i] != x[0][i] for c in x)]
    return len(A), len(D)


def decode_word(words):
    """step 4 for one word of F: words[j] = the word in copy j (copy 0's is not a codeword).  Returns (value, how): how = 'taken' (a),
    'joint' (b), 'none' or 'several' (value None)."""
    held = [w for w in words[1:] if is_codeword(w)]
    lost = [w for w in words if not is_codeword(w)]
    if held:
        count = {v: held.count(v) for v in set(held)}
        top = max(count.values())
        tops = [v for v, n in count.items() if n == top]
        if len(tops) > 1:
            return None, "several"
        v = tops[0]
        return (v, "taken") if all(dist(w, v) == 2 for w in lost) else (None, "none")
    fits = [c for c in CODEWORDS if all(dist(w, c) == 2 for w in words)]
    if len(fits) == 1:
        return fits[0], "joint"
    return None, ("several" if fits else "none")


def combine(copies, n=None):
    K = len(copies) if n is None else int(n)
    copies = [copies[k] for k in range(K)]
    r = copies[0]
    x = [[int(b) for b in c["data"][:WORDS]] for c in copies]
    n_a, n_d = guard(x)
    if n_a < MIN_AGREED or n_d > MAX_DIFFER:
        return r.copy(), -1
    F = [i for i in range(WORDS) if not is_codeword(x[0][i])]
    got = {i: decode_word([c[i] for c in x]) for i in F}
    if any(how == "none" for _, how in got.values()):
        return r.copy(), -2
    if any(how == "several" for _, how in got.values()):
        return r.copy(), -3
    out = r.copy()
    for i in F:
        out["data"][i] = got[i][0]
    out["nerr"][0] += len(F)
    out["nerr"][1] = 0
    J = sum(1 for _, how in got.values() if how == "joint")
    out["flags"] |= FRAME_RESCUED | FRAME_COMBINED | (K << 8) | (min(J, 15) << 12)
    return out, K


new_div_state = dr.new_state


def diversity(records, groups, offsets=None, window=960, state=None):
    """One submit: diversity_reference.diversity on is_frame, failed, combine and STATUS above.  groups: [[channel, ...], ...]; offsets:
    {channel: offset_bits} or a sequence indexed by channel (None: zeros).  outcomes[i]: 'other' (not visited), 'good', 'no_partner',
    'partner_good', 'combined', 'guard', 'none', 'several'."""
    return dr.diversity(records, groups, offsets, window, state, is_frame=is_frame, failed=failed,
                        attempt=lambda r, partners: combine([r] + partners), status=STATUS)


restart_div_group = dr.restart_group

# ---- the align step (SPEC 3.3k) with the predicates of SPEC 3.3m
new_state, restart_group = da.new_state, da.restart_group


def good(r):
    return is_frame(r) and int(r["nerr"][1]) == 0


def match(x, y):
    return int(x["len"]) == int(y["len"]) == WORDS and bytes(x["data"][:WORDS]) == bytes(y["data"][:WORDS])


def align(records, groups, state, mode):
    """diversity_align_reference.align on `good` and `match` above"""
    return da.align(records, groups, state, mode, good=good, match=match)


def run(records, groups, state, mode=LEARN | MARK, window=960):
    """One submit as the library runs it (diversity_align_reference.run): align, the pass over the locked members at the learned
    offsets, the carried records of the unlocked members.  Returns (records after both steps in the same order, outcomes, state)."""
    return da.run(records, groups, state, mode, window, good=good, match=match, diversity=diversity, is_frame=is_frame)
