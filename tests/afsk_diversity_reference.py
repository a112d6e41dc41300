"""A Python twin of sonde_batch_set_diversity for iMet and SRS-C50 groups (DESIGN SPEC 3.3o), written from the rule alone: plain
Python, brute force -- apply a subset, recompute the whole check --, no column, no syndrome, for both types; nothing shared with
csrc/afsk_diversity_kernel.hip.  Test infrastructure only.

    combine(copies, n)         steps 3 to 6 on caller-made records: copy 0 is the record to rewrite.  Returns (record, status):
                               status = the copies used, -1 (not attempted: no unknown, more than 8, for iMet a bit of the type byte
                               or of XDATA's length byte in doubt), -2 (no subset fits), -3 (several fit).
    diversity(records, groups, offsets, window, state)
                               one submit: steps 1 and 2 are SPEC 3.3j's (diversity_reference.diversity, whose state and
                               restart_group serve here unchanged) with the substitutions of SPEC 3.3o.  window 0: 160 for an iMet
                               group, 40 for a C50 group -- a group's kind is its records' `type`.
    align(records, groups, state, mode), run(records, groups, state, mode, window), new_state, restart_group
                               the align step of SPEC 3.3k with the two predicates of SPEC 3.3o (iMet groups only), and one submit
                               as the library runs it; the state is diversity_align_reference's.

The check primitives are those of the SPEC 3.3i twin (afsk_rescue_reference.py), imported and not changed; the walk is
check_diversity_reference.py's (working_frame) and diversity_reference.py's."""
from __future__ import annotations

import numpy as np

import afsk_rescue_reference as ar
import check_diversity_reference as cr
import diversity_align_reference as da
import diversity_reference as dr

IMET4, C50 = ar.IMET4, ar.C50
FRAME_RESCUED, FRAME_COMBINED, FRAME_DUPLICATE = 2, 4, 8
LEARN, MARK = da.LEARN, da.MARK
CAP = 8
WINDOW = {IMET4: 160, C50: 40}
ALIGN_LENGTHS = (14, 18, 20)             # PTU, GPS, PTUX: they carry a packet counter or the time
STATUS = cr.STATUS
unknowns = cr.unknowns


def is_frame(r):
    return ar.eligible(int(r["type"]), int(r["len"]))


def failed(r):
    return int(r["nerr"][0]) < 0


def combine(copies, n=None):
    K = len(copies) if n is None else int(n)
    copies = [copies[k] for k in range(K)]
    r = copies[0]
    kind, ln = int(r["type"]), int(r["len"])
    w, V = cr.working_frame(copies)                               # step 3
    passes = lambda bits: bool(ar.check_passes(kind, np.packbits(bits)[None, :], ln)[0])      # noqa: E731
    if not (passes(w) and len(V) >= 1):                           # 4. majority alone
        # 5. solve
        if len(V) == 0 or len(V) > CAP:
            return r.copy(), -1
        if kind == IMET4 and (V[0] < 16 or (V[0] < 24 and int(np.packbits(w)[1]) == 3)):
            return r.copy(), -1
        # every non-empty subset of V applied to w, one trial packet per subset, and the whole check recomputed over each
        subsets = np.arange(1, 1 << len(V))
        trials = np.tile(w, (len(subsets), 1))
        for j, k in enumerate(V):
            trials[((subsets >> j) & 1) == 1, k] ^= 1
        sols = np.nonzero(ar.check_passes(kind, np.packbits(trials, axis=1), ln))[0]
        if len(sols) != 1:
            return r.copy(), (-3 if len(sols) else -2)
        w = trials[sols[0]]
    # 6. record
    out = r.copy()
    out["data"][:ln] = np.packbits(w)
    out["nerr"][0] = 0
    out["flags"] |= FRAME_RESCUED | FRAME_COMBINED | (K << 8) | (min(len(V), 15) << 12)
    return out, K


new_div_state = dr.new_state


def _kind_of(members, records, state):
    """the sonde type of a group: its records' (this submit's, or a carried one); None: it has none, and nothing happens to it"""
    for ch in members:
        hit = records[records["channel"] == ch]
        if len(hit):
            return int(hit[0]["type"])
        if state is not None and ch in state["carried"]:
            return int(state["carried"][ch]["type"])
    return None


def diversity(records, groups, offsets=None, window=0, state=None):
    """One submit: diversity_reference.diversity on is_frame, failed, combine and STATUS above, once per kind over that kind's groups
    (the other groups stand in the list without members, so the group numbers stay), each with its own default window."""
    state = dr.new_state(groups) if state is None else state
    out = records.copy()
    outcomes = ["other"] * len(out)
    kinds = [_kind_of(members, records, state) for members in groups]
    for kind in (IMET4, C50):
        mine = [members if k == kind else [] for members, k in zip(groups, kinds)]
        if not any(mine):
            continue
        new, oc, state = dr.diversity(out, mine, offsets, window or WINDOW[kind], state, is_frame=is_frame, failed=failed,
                                      attempt=lambda r, partners: combine([r] + partners), status=STATUS)
        chans = {ch for members in mine for ch in members}
        for i in range(len(out)):
            if int(out[i]["channel"]) in chans:
                out[i] = new[i]
                outcomes[i] = oc[i]
    return out, outcomes, state


restart_div_group = dr.restart_group

# ---- the align step (SPEC 3.3k) with the predicates of SPEC 3.3o: iMet only, and of its packets those that cannot repeat
new_state, restart_group = da.new_state, da.restart_group


def good(r):
    return int(r["type"]) == IMET4 and int(r["len"]) in ALIGN_LENGTHS and not failed(r)


match = cr.match


def align(records, groups, state, mode):
    """diversity_align_reference.align on `good` and `match` above"""
    return da.align(records, groups, state, mode, good=good, match=match)


def run(records, groups, state, mode=LEARN | MARK, window=0):
    """One submit as the library runs it (diversity_align_reference.run): align, the pass over the locked members at the learned
    offsets, the carried records of the unlocked members.  Returns (records after both steps in the same order, outcomes, state)."""
    return da.run(records, groups, state, mode, window, good=good, match=match, diversity=diversity, is_frame=is_frame)
