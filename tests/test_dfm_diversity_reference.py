"""The twin of sonde_batch_set_diversity for DFM groups (tests/dfm_diversity_reference.py, DESIGN SPEC 3.3m) on the CPU oracle's records of
the designed scene (tests/dfm_diversity_scenes.py): every case ends as the scene plan says, every combined record is the transmitted
frame, the set of frames a group delivers does not depend on how the stream is cut, and a copy that arrives a submit late is combined
from the carried record; rule (b) of step 4 exhaustively for two copies; a group whose offset is wrong by one frame changes nothing.
Then the align twin for DFM: offsets are learned and followed, one copy per frame stays unmarked, and what the learn rule does with a
frame that is repeated (a sonde at rest)."""
import itertools

import numpy as np
import pytest

import dfm_diversity_reference as cr
import dfm_diversity_scenes as cs

NAME = {-1: "guard", -2: "none", -3: "several"}


def _by_frame(sc, records, outcomes):
    got = {}
    for f, o in zip(records, outcomes):
        w = cs.frame_of(sc, f)
        assert w is not None, (int(f["channel"]), int(f["bitpos"]))
        got.setdefault(w[:2], []).append((f, o, w[2]))
    return got


def test_every_case_ends_as_planned_and_combined_records_are_the_transmitted_frames():
    sc = cs.scene()
    base = cs.oracle_frames()
    out, outcomes, state = cr.diversity(base.copy(), sc.groups, sc.offsets, sc.window)
    got = _by_frame(sc, out, outcomes)
    n_combined, seen = 0, set()
    for key, (case, expect) in sc.plan.items():
        recs = got.get(key, [])
        if case is None:
            assert all(o in ("good", "other") for _, o, _ in recs), (key, [o for _, o, _ in recs])
            continue
        copies = sum(1 for s, _ in sc.sonde if s == key[0])
        assert len(recs) == copies, (key, case)                # a damaged frame lies inside the scene in every copy
        seen.add(case)
        oc = [o for _, o, _ in recs]
        assert oc.count("combined") == (1 if expect == "combined" else 0), (key, case, oc)
        status, J = cs.EXPECT[case][1:]
        if expect == "combined":
            n_combined += 1
            f, _, tx = next(r for r in recs if r[1] == "combined")
            assert bytes(f["data"][:33]) == bytes(tx) and int(f["nerr"][1]) == 0 and int(f["nerr"][0]) >= 1, (key, case)
            assert (int(f["flags"]) & 0xFF06) == (2 | 4 | (copies << 8) | (J << 12)), (key, case, hex(int(f["flags"])))
            assert cr.joint(f["flags"]) == J
            if case == "quad_tie":                              # copy 0 meets one against one; copy 1, visited next, is combined
                assert oc == ["several", "combined", "partner_good", "partner_good"], (key, oc)
            elif key[0] != cs.DELAYED_STREAM:                   # copy 0 is visited first and combined; the others then find it good
                assert oc == ["combined"] + ["partner_good"] * (copies - 1), (key, case, oc)
            else:
                assert sorted(oc) == ["combined", "partner_good"], (key, case, oc)
        elif case == "partner_good":
            assert sorted(oc) == ["good", "partner_good"], (key, oc)
        elif case == "lonely":
            assert set(oc) == {"other"}, (key, oc)
        else:
            assert set(oc) == {NAME[status]}, (key, case, oc)
    assert seen == set(cs.EXPECT) - {None}
    assert sum(state["combined"]) == n_combined == sum(1 for c, e in sc.plan.values() if e == "combined") >= 15
    # every visit that found failed partners only counts as tried, the guard's refusals included
    assert sum(state["tried"]) == sum(1 for o in outcomes if o in ("combined", "guard", "none", "several"))
    assert sum(1 for o in outcomes if o == "guard") >= 8
    untouched = [i for i, o in enumerate(outcomes) if o != "combined"]
    assert out[untouched].tobytes() == base[untouched].tobytes()


def test_the_delivered_frames_do_not_depend_on_the_cut_and_a_late_copy_is_combined_from_the_carried_record():
    sc = cs.scene()
    base = cs.oracle_frames()

    def delivered(parts):
        state, good, late = None, set(), 0
        for p in parts:
            before = {ch: r.copy() for ch, r in (state["carried"].items() if state else [])}
            out, outcomes, state = cr.diversity(p.copy(), sc.groups, sc.offsets, sc.window, state)
            for f, o in zip(out, outcomes):
                w = cs.frame_of(sc, f)
                if int(f["nerr"][1]) == 0:
                    good.add(w[:2])
                if o == "combined":
                    assert bytes(f["data"][:33]) == bytes(w[2])
                    here = sum(1 for q in p if cs.frame_of(sc, q)[:2] == w[:2])
                    if here < ((int(f["flags"]) >> 8) & 0xF) and any(cs.frame_of(sc, c)[:2] == w[:2] for c in before.values()):
                        late += 1                               # a copy it was made from came with an earlier submit
        return good, late, state

    whole, _, st1 = delivered([base])
    for cuts in (4, 10):
        good, _, st = delivered(cs.cut(base, sc, cuts))
        assert good == whole, cuts
        assert sum(st["combined"]) == sum(st1["combined"]), cuts
    # two submits cut between the two copies of a frame the plan combines
    first = cs.late_cut_tiles(sc)
    end = base["bitpos"].astype(np.int64) + sc.listed_after
    boundary = first * cs.TILE * (sc.nchips - 16) // sc.n
    good, late, _ = delivered([base[end <= boundary], base[end > boundary]])
    assert good == whole and late >= 1


def test_the_rule_alone_reaches_every_status_on_the_unit_cases():
    copies, n_copies, names, want = cs.unit_cases()
    seen = set()
    for i, name in enumerate(names):
        rec, st = cr.combine(copies[i], n_copies[i])
        if want[i] is not None:
            assert st == want[i], (name, st, want[i])
        seen.add(st)
        if st > 0:
            assert st == n_copies[i] and int(rec["nerr"][1]) == 0 and all(cr.is_codeword(b) for b in rec["data"][:33]), name
            assert rec["data"][33:].tobytes() == copies[i][0]["data"][33:].tobytes()
        else:
            assert rec.tobytes() == copies[i][0].tobytes(), name
    assert seen == {2, 3, 4, -1, -2, -3}


def test_rule_b_for_two_copies_exhaustively_the_truth_or_nothing():
    """every codeword with every two weight-2 error patterns (16 * 28 * 28): the word decodes to the codeword or not at all, and it
    decodes exactly when no weight-4 codeword's support holds both patterns (counted here without the decoder)"""
    pairs = [(0x80 >> a) | (0x80 >> b) for a, b in itertools.combinations(range(8), 2)]
    w4 = [c for c in cr.CODEWORDS if bin(c).count("1") == 4]
    assert len(pairs) == 28 and len(w4) == 14
    free = {(e1, e2) for e1 in pairs for e2 in pairs if not any(w & e1 == e1 and w & e2 == e2 for w in w4)}
    decoded = 0
    for c in cr.CODEWORDS:
        for e1 in pairs:
            for e2 in pairs:
                v, how = cr.decode_word([c ^ e1, c ^ e2])
                assert how in ("joint", "several") and (v == c if how == "joint" else v is None), (c, e1, e2, v, how)
                assert (how == "joint") == ((e1, e2) in free)
                decoded += how == "joint"
    assert decoded == 16 * len(free) and len(free) == 28 * 12      # per first pattern: itself, 12 that share a bit and 3 of the 15 disjoint ones are lost


def test_a_group_whose_offset_is_wrong_by_one_frame_changes_nothing():
    sc = cs.scene()
    base = cs.oracle_frames()
    out, outcomes, state = cr.diversity(base.copy(), sc.groups, cs.OFFSETS_WRONG, sc.window)
    mine = np.isin(base["channel"], sc.groups[0])
    assert out[mine].tobytes() == base[mine].tobytes()
    assert state["combined"][0] == 0 and state["tried"][0] >= 8
    # (the stream's last frame has no later neighbour and meets its own copy: the window takes the nearest record, 557 chips off)
    assert sum(1 for o, m in zip(outcomes, mine) if m and o == "guard") >= 8 and "combined" not in {o for o, m in zip(outcomes, mine) if m}
    assert state["combined"][1:] == cr.diversity(base.copy(), sc.groups, sc.offsets, sc.window)[2]["combined"][1:]


# ---- the align step for DFM groups
MODE = cr.LEARN | cr.MARK


def _align_run(records, cuts, sc):
    state = cr.new_state(sc.groups, None, MODE)
    outs = []
    for p in cs.cut(records, sc, cuts):
        out, _, state = cr.run(p.copy(), sc.groups, state, MODE, sc.window)
        outs.append(out)
    return np.concatenate(outs), state


@pytest.mark.parametrize("cuts", [1, 2, 4])
def test_align_learns_the_offsets_and_marks_all_but_one_copy_per_frame(cuts):
    """the triple's third receiver is 5000 chips, nine DFM frames, late: the two copies of a frame must be seen at once (SPEC 3.3k), so
    it locks only where a submit is long enough to hold a frame of both -- with four submits of 3200 chips it never does, and stays a
    member without records"""
    sc = cs.scene(clean=True, align=True)
    base = cs.oracle_frames(clean=True, align=True)
    out, state = _align_run(base, cuts, sc)
    if cuts == 4:
        assert not state["locked"][6] and all(state["locked"][ch] for members in sc.groups for ch in members if ch != 6)
        return
    for g, members in enumerate(sc.groups):
        assert all(state["locked"][ch] for ch in members), g
        for ch in members[1:]:       # the difference of the chip counts is the difference of the delays, to the chip
            assert abs(state["off"][ch] - state["off"][members[0]] - (sc.sonde[ch][1] - sc.sonde[members[0]][1])) <= 1, (g, ch)
        if g == 2:                   # a copy nine frame periods late goes unmarked (SPEC 3.3k: later than one frame period after the first)
            continue
        recs = [f for f in out if int(f["channel"]) in members]
        frames = {cs.frame_of(sc, f)[:2] for f in recs}
        unmarked =[cs.frame_of(sc, f)[:2] for f in recs if not int(f["flags"]) & cr.FRAME_DUPLICATE]
        assert sorted(unmarked) == sorted(frames), g
        assert state["duplicates"][g] == len(recs) - len(frames)


def test_align_on_the_damaged_scene_locks_and_every_combined_frame_is_the_transmitted_one():
    sc = cs.scene(align=True)
    out, state = _align_run(cs.oracle_frames(align=True), 2, sc)
    assert all(state["locked"][ch] for members in sc.groups for ch in members)
    comb = out[out["flags"] & cr.FRAME_COMBINED != 0]
    assert len(comb) == sum(state["div"]["combined"]) >= 15
    for f in comb:
        assert bytes(f["data"][:33]) == bytes(cs.frame_of(sc, f)[2])


def test_a_repeated_frame_the_latest_candidates_count_and_a_wrong_lock_is_corrected_by_the_next_frame():
    """a sonde at rest can send the same 33 words twice, 560 chips apart.  The learn rule takes the match that is latest in the higher
    member and, of several, latest in the lower: right whenever both members see both copies.  If the lower member's view holds
    only the earlier one, the group locks one frame off; nothing is combined across that offset (the pairing guard), and the next
    frame that is good in both and not repeated re-bases the higher member."""
    sc = cs.scene(clean=True)
    base = cs.oracle_frames(clean=True)
    recs = cs.sort_records(base[np.isin(base["channel"], [0, 1])].copy())
    a, b = recs[recs["channel"] == 0], recs[recs["channel"] == 1]
    assert len(a) == len(b) >= 8
    for r in (a, b):
        r["data"][3] = r["data"][2]                             # frame 3 repeats frame 2
    groups = [[0, 1]]
    true = int(b["bitpos"][0]) - int(a["bitpos"][0])
    # both members see both copies
    state = cr.new_state(groups, None, MODE)
    cr.run(np.concatenate([a[:4], b[:4]]), groups, state, MODE)
    assert state["off"][1] - state["off"][0] == true and state["learned"] == [1]
    # the lower member's view ends with the first copy, the higher's with the second: one frame off
    state = cr.new_state(groups, None, MODE)
    cr.run(np.concatenate([a[2:3], b[2:4]]), groups, state, MODE)
    assert state["off"][1] - state["off"][0] == true + cs.FRAME_CHIPS and state["learned"] == [1]
    # the next submit brings the second copy of the lower member and frame 4 of both: the latest match is frame 4, the offset is right again
    cr.run(np.concatenate([a[3:5], b[4:5]]), groups, state, MODE)
    assert state["off"][1] - state["off"][0] == true and state["learned"] == [2]


def test_a_failed_copy_beside_a_copy_the_dfm_rescue_completed_stays_as_recorded():
    """cs.rescued_partner_scene through the SPEC 3.3g twin and then this one, the order the library runs them in"""
    import dfm_rescue_reference as dfr
    import oracle_lib
    oracle_lib.build()
    sc = cs.rescued_partner_scene()
    recs, streams = [], []
    for c in range(sc.C):
        ch = oracle_lib.Channel(sc.type, c)
        ch.feed(sc.iq[c])
        recs.append(ch.frames())
        streams.append(ch.bits())
    first = cs.sort_records(np.concatenate(recs))
    rescued, how, _ = dfr.rescue(first, dfr.chips_of_streams(streams))
    out, outcomes, state = cr.diversity(rescued, sc.groups, None, sc.window)
    seen = {"rescued_partner": 0, "both_hidden": 0}
    for f, h, o, r in zip(rescued, how, outcomes, out):
        case = sc.plan[cs.frame_of(sc, f)[1]]
        if case is None:
            continue
        ch = int(f["channel"])
        seen[case] += ch == 0
        want = {("rescued_partner", 0): ("unsolved", "partner_good"), ("rescued_partner", 1): ("rescued", "good"),
                ("both_hidden", 0): ("unsolved", "combined"), ("both_hidden", 1): ("unsolved", "partner_good")}[(case, ch)]
        assert (h, o) == want, (case, ch, h, o)
        assert (r.tobytes() == f.tobytes()) == (o != "combined")
    assert seen["rescued_partner"] >= 3 and seen["both_hidden"] >= 3
    assert state["tried"] == state["combined"] == [seen["both_hidden"]]
