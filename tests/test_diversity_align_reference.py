"""The twin of the align step (tests/diversity_align_reference.py, DESIGN SPEC 3.3k) on the CPU: every designed caller-made case ends
as designed, and over the CPU oracle's records of the scenes of tests/diversity_align_scenes.py the learned offsets are the scene's
delays, one copy of every transmitted frame stays unmarked however the stream is cut, the cut changes which copy and not which frames,
and the groups that can never lock stay as they are.  No GPU."""
import copy
import functools

import numpy as np
import pytest

import diversity_align_reference as dar
import diversity_align_scenes as das
import diversity_reference as dr
import diversity_scenes as ds

DUP, COMBINED = dar.FRAME_DUPLICATE, dr.FRAME_COMBINED

# name -> (off of the case's members, locked, learned, duplicates, flags & DUPLICATE per member's records)
DESIGNED = {
    "pair_lock": ([0, 450], 3, 1, 1, [[0], [8]]),
    "pair_lock_initial_offset_kept": ([70, 520], 3, 1, 1, [[0], [8]]),
    # members 0 and 1 are never good together: 2 locks to 0 through frame X, then 1 joins through the frame it shares with 2
    "chain_of_three": ([0, 100, 5000], 7, 2, 2, [[0], [0, 0], [8, 8]]),
    "rebase_higher": ([0, 450], 3, 1, 1, [[0], [8]]),
    "agree_nothing_learned": ([0, 450], 3, 0, 1, [[0], [8]]),
    "lower_joins_locked_higher": ([50, 500], 3, 1, 1, [[0], [8]]),
    "carried_only": ([0, 480], 3, 1, 1, [[], [8]]),
    "carried_failed_is_no_candidate": ([0, 0], 0, 0, 0, [[], [0]]),
    "latest_in_b_wins": ([0, 520], 3, 1, 2, [[0, 0], [8, 8]]),
    "failed_copies_teach_nothing": ([0, 0], 0, 0, 0, [[0], [0]]),
    "two_sondes": ([0, 0], 0, 0, 0, [[0, 0], [0, 0]]),
    "same_bytes_other_len": ([0, 0], 0, 0, 0, [[0], [0]]),
    "header_differs": ([0, 450], 3, 1, 1, [[0], [8]]),
    "last_byte_differs": ([0, 0], 0, 0, 0, [[0], [0]]),
    "byte_8_differs": ([0, 0], 0, 0, 0, [[0], [0]]),
    "last_byte_differs_518": ([0, 0], 0, 0, 0, [[0], [0]]),
    "match_518": ([0, 451], 3, 1, 1, [[0], [8]]),
    "mode_0": ([0, 0, 0], 0, 0, 0, [[0, 0], [0], [0]]),
    "mode_1": ([0, 450, 5120], 7, 2, 0, [[0, 0], [0], [0]]),
    "mode_2": ([0, 0, 0], 0, 0, 3, [[0, 8], [8], [8]]),
    "four_copies": ([0, 40, 5000, -100], 15, 3, 3, [[0], [8], [8], [8]]),
}


def test_every_designed_case_ends_as_designed():
    cases = {c["name"]: c for c in das.unit_cases()}
    for name, (off, locked, learned, dups, flags) in DESIGNED.items():
        c = cases[name]
        per, o, lk, le, du = das.twin_case(c)
        assert (o[:len(off)], lk, le, du) == (off, locked, learned, dups), name
        assert [[int(r["flags"]) & DUP for r in p] for p in per] == flags, name
        for p, recs in zip(per, c["members"]):              # nothing else of a record changes
            for r, was in zip(p, recs):
                r = r.copy()
                r["flags"] &= ~np.uint32(DUP)
                r["channel"] = was["channel"]
                assert r.tobytes() == was.tobytes(), name


def test_every_pair_order_and_lock_state():
    """four members of which only (a, b) share a frame, at 1000 + 10 a in a and 4000 + 100 b in b; the initial offsets are 5, 60, 700, 8000"""
    init = [5, 60, 700, 8000]
    for c in das.unit_cases():
        if not c["name"].startswith("pair_") or "_locks_" not in c["name"]:
            continue
        a, b, lk = int(c["name"][5]), int(c["name"][6]), int(c["name"][-1])
        d = (4000 + 100 * b) - (1000 + 10 * a)
        _, off, locked, learned, dups = das.twin_case(c)
        want = list(init)
        if lk == 2:                                         # only the higher member is locked: the lower one joins it
            want[a] = init[b] - d
        else:
            want[b] = init[a] + d
        assert (off, locked, learned, dups) == (want, c["locked"] | (1 << a) | (1 << b), 1, 1), c["name"]


def test_unlocked_members_are_untouched_by_the_combining_steps():
    from sdrpp_radiosonde_amd import synth
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    tx = synth.rs41_build_frames(41, np.arange(1), np.arange(1) + 9, False)[0]
    da, db = ds.case_damage("disjoint_bursts", np.random.default_rng(3))
    recs = np.zeros(2, dtype=FRAME_DTYPE)
    recs[0], recs[1] = ds.make_record(tx, da, 0, 1000)[()], ds.make_record(tx, db, 1, 1300)[()]
    groups = [[0, 1]]
    st = dar.new_state(groups, None, dar.LEARN)              # nothing known: unlocked, and two failed copies teach nothing
    out, outcomes, st = dar.run(recs, groups, st, dar.LEARN)
    assert out.tobytes() == recs.tobytes() and outcomes == ["other", "other"] and st["div"]["tried"] == [0]
    assert not any(st["locked"].values()) and st["learned"] == [0]
    assert all(st["div"]["carried"][ch].tobytes() == recs[ch].tobytes() for ch in (0, 1))      # the carried records are kept all the same
    st = dar.new_state(groups, [0, 300], dar.LEARN)          # the same records in a locked group are combined
    out, outcomes, st = dar.run(recs, groups, st, dar.LEARN)
    assert outcomes[0] == "combined" and bytes(out[0]["data"][:320]) == bytes(tx) and int(out[0]["flags"]) & COMBINED


@functools.lru_cache(maxsize=None)
def _run(extended, cuts, mode=3, true_offsets=False):
    """[(records after the submit, a copy of the state after it)] over the oracle's records of the scene"""
    sc = das.scene(extended)
    st = dar.new_state(sc.groups, das.TRUE_OFFSETS if true_offsets else None, mode)
    res = []
    for sub in das.cut(das.oracle_frames(extended), sc, cuts):
        out, _, st = dar.run(sub.copy(), sc.groups, st, mode, sc.window)
        res.append((out, copy.deepcopy(st)))
    return res


def _is_good(r):
    return int(r["nerr"][0]) >= 0 and int(r["nerr"][1]) >= 0


EXT = pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
CUTS = pytest.mark.parametrize("cuts", [1, 4, 10])


@EXT
@CUTS
def test_the_learned_offsets_are_the_scenes_delays(extended, cuts):
    sc = das.scene(extended)
    res = _run(extended, cuts)
    st = res[-1][1]
    for ch, (_, delay) in enumerate(das.MEMBERS[:7]):
        want = delay + (das.JUMP_BITS if ch == 6 else 0)
        assert st["locked"][ch] and abs(st["off"][ch] - want) < 64, (ch, st["off"][ch])
    # group c: the first offset before the jump, the second within one frame of it
    pos_jump = [pos for pos, _, _, k in sc.tx[6] if k in (das.JUMP_FRAME[extended], das.JUMP_FRAME[extended] + 1)]
    nbits = sc.n // 10
    first = min(s for s, (_, t) in enumerate(res) if abs(t["off"][6] - das.JUMP_BITS) < 64)
    assert first <= min((pos_jump[1] + 8 * sc.flen) * cuts // nbits, cuts - 1)
    if cuts == 10:
        before = [t["off"][6] for s, (_, t) in enumerate(res) if t["locked"][6] and s < first]
        assert before and all(abs(v) < 64 for v in before)
        assert first >= (pos_jump[0] + 8 * sc.flen) * cuts // nbits


@EXT
@CUTS
def test_one_copy_of_every_transmitted_frame_stays_unmarked(extended, cuts):
    sc = das.scene(extended)
    per_frame = {}
    for out, _ in _run(extended, cuts):
        for r in out:
            if _is_good(r):
                stream, k = das.frame_of(sc, r)[:2]
                per_frame.setdefault((stream, k), []).append(int(r["flags"]) & DUP)
    assert len(per_frame) > 30
    for key, flags in per_frame.items():
        assert flags.count(0) == 1, (key, flags)
    # as many marks as the first pass left surplus good copies (a combined frame is the only good copy of its frame)
    first_pass = {}
    for r in das.oracle_frames(extended):
        if _is_good(r) and int(r["channel"]) < 11:
            key = das.frame_of(sc, r)[:2]
            first_pass[key] = first_pass.get(key, 0) + 1
    surplus = sum(v - 1 for v in first_pass.values())
    assert sum(len(f) - 1 for f in per_frame.values()) == sum(_run(extended, cuts)[-1][1]["duplicates"]) == surplus >= 6


@EXT
@CUTS
def test_the_cut_changes_which_copy_not_which_frames(extended, cuts):
    """groups a and b, whose delays do not change: from the submit in which all members of the group are locked onwards the distinct
    good frames are those of a run that was given the true offsets"""
    sc = das.scene(extended)
    learn, given = _run(extended, cuts), _run(extended, cuts, 0, True)
    for g in (0, 1):
        members = sc.groups[g]
        lock = min(s for s, (_, t) in enumerate(learn) if all(t["locked"][ch] for ch in members))
        sets = []
        for res in (learn, given):
            got = set()
            for out, _ in res[lock:]:
                got |= {das.frame_of(sc, r)[:2] for r in out if int(r["channel"]) in members and _is_good(r)}
            sets.append(got)
        assert sets[0] == sets[1] and len(sets[0]) >= 2, (g, sets)
        if lock == 0:
            assert learn[-1][1]["div"]["combined"][g] == given[-1][1]["div"]["combined"][g] >= 1


@EXT
def test_the_combined_frames_are_the_transmitted_ones(extended):
    sc = das.scene(extended)
    n = {g: 0 for g in range(3)}
    for out, _ in _run(extended, 4):
        for r in out:
            if int(r["flags"]) & COMBINED:
                tx = das.frame_of(sc, r)[2]
                assert bytes(r["data"][:len(tx)]) == bytes(tx)
                n[[int(r["channel"]) in g for g in sc.groups].index(True)] += 1
    assert all(v >= 1 for v in n.values()), n               # group b: copies 5000 bits apart


@EXT
@CUTS
def test_two_sondes_and_never_good_together_never_lock(extended, cuts):
    sc = das.scene(extended)
    res = _run(extended, cuts)
    for (out, st), sub in zip(res, das.cut(das.oracle_frames(extended), sc, cuts)):
        keep = np.isin(sub["channel"], [7, 8, 9, 10, 11])
        assert keep.sum() == 0 or out[keep].tobytes() == sub[keep].tobytes()
        assert not any(st["locked"][ch] for ch in (7, 8, 9, 10))
        assert st["learned"][3:] == [0, 0] and st["duplicates"][3:] == [0, 0] and st["div"]["tried"][3:] == [0, 0]
    assert np.isin(das.oracle_frames(extended)["channel"], [7, 8, 9, 10]).sum() >= 20


def test_a_restart_puts_the_group_back():
    groups = [[0, 1], [2, 3]]
    st = dar.new_state(groups, None, 3)
    st["off"][1], st["locked"][0], st["locked"][1], st["learned"][0], st["duplicates"][0] = 450, True, True, 1, 4
    st["locked"][2] = st["locked"][3] = True
    dar.restart_group(st, groups, 0)
    assert (st["off"][1], st["locked"][0], st["locked"][1], st["learned"], st["duplicates"]) == (0, False, False, [0, 0], [0, 0])
    assert st["locked"][2] and st["locked"][3]
    st = dar.new_state(groups, [0, 7, 0, 9], 3)
    st["off"][1] = 450
    dar.restart_group(st, groups, 0)
    assert st["off"][1] == 7 and st["locked"][1]
