"""The twin of sonde_batch_set_diversity for M10 / M20 / MRZ-N1 groups (tests/check_diversity_reference.py, DESIGN SPEC 3.3l) on the CPU
oracle's records of the designed scenes (tests/check_diversity_scenes.py): every case ends as the scene plan says, every combined
record is the transmitted frame, the counts per kind are the plan's, the set of frames a group delivers does not depend on how the
stream is cut, and a copy that arrives a submit late is combined from the carried record.  Then the align twin for these types: the
offset is learned from the first pair of identical good frames, a jump is followed, all but one good copy of a frame are marked."""
import numpy as np
import pytest

import check_diversity_reference as cr
import check_diversity_scenes as cs

KINDS = list(cs.KINDS)
# what the first visited copy of a case ends as, for the cases the pass does not combine
NAME = {-1: "not_attempted", -2: "no_fit", -3: "several_fit"}


def _by_frame(sc, records, outcomes):
    got = {}
    for f, o in zip(records, outcomes):
        w = cs.frame_of(sc, f)
        assert w is not None, (int(f["channel"]), int(f["bitpos"]))
        got.setdefault(w[:2], []).append((f, o, w[2]))
    return got


@pytest.mark.parametrize("kind", KINDS)
def test_every_case_ends_as_planned_and_combined_records_are_the_transmitted_frames(kind):
    sc = cs.scene(kind)
    out, outcomes, state = cr.diversity(cs.oracle_frames(kind).copy(), sc.groups, sc.offsets, sc.window)
    got = _by_frame(sc, out, outcomes)
    n_combined, seen = 0, set()
    for key, (case, expect) in sc.plan.items():
        recs = got.get(key, [])
        if case is None:
            assert all(o in ("good", "other") for _, o, _ in recs), (key, [o for _, o, _ in recs])
            continue
        assert len(recs) == sum(1 for s, _ in sc.sonde if s == key[0]), (key, case)      # a damaged frame lies inside the scene in every copy
        seen.add(case)
        oc = [o for _, o, _ in recs]
        assert oc.count("combined") == (1 if expect == "combined" else 0), (key, case, oc)
        status = cs.EXPECT[case][1]
        if expect == "combined":
            n_combined += 1
            f, _, tx = next(r for r in recs if r[1] == "combined")
            assert bytes(f["data"][:sc.len]) == bytes(tx) and int(f["nerr"][0]) == 0, (key, case)
            assert (int(f["flags"]) & 0xF06) == (2 | 4 | (status << 8)), (key, case, hex(int(f["flags"])))
            want_v = {"triple_majority": 15, "triple_two_wrong": 5, "quad_tie": 5, "disjoint_3_3": 6, "one_vs_seven": 8, "in_check": 2}[case]
            assert cr.unknowns(f["flags"]) == want_v, (key, case)
            assert all(o == "partner_good" for o in oc if o != "combined"), (key, case, oc)      # the other copies find the combined one
        elif case == "partner_good":
            assert sorted(oc) == ["good", "partner_good"], (key, oc)
        elif case == "lonely":
            assert set(oc) <= {"no_partner", "other"}, (key, oc)
        else:
            assert set(oc) == {NAME[status]}, (key, case, oc)
    assert seen == set(cs.PAIR_CASES[kind]) | {"triple_majority", "triple_two_wrong", "quad_tie", "lonely"}
    # the counts of the plan: combined records per kind, and per group the counters
    assert sum(state["combined"]) == n_combined == sum(1 for c, e in sc.plan.values() if e == "combined")
    assert n_combined == {"m10": 33, "m20": 36, "mrz": 19}[kind]
    assert state["combined"][4] == state["tried"][4] == 0                  # the pair the window does not cover
    untouched = [i for i, o in enumerate(outcomes) if o != "combined"]
    assert out[untouched].tobytes() == cs.oracle_frames(kind)[untouched].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_the_delivered_frames_do_not_depend_on_the_cut_and_a_late_copy_is_combined_from_the_carried_record(kind):
    sc = cs.scene(kind)
    base = cs.oracle_frames(kind)

    def delivered(parts):
        state, good, late = None, set(), 0
        for p in parts:
            before = {ch: r.copy() for ch, r in (state["carried"].items() if state else [])}
            out, outcomes, state = cr.diversity(p.copy(), sc.groups, sc.offsets, sc.window, state)
            for f, o in zip(out, outcomes):
                w = cs.frame_of(sc, f)
                if int(f["nerr"][0]) >= 0:
                    good.add(w[:2])
                if o == "combined":
                    assert bytes(f["data"][:sc.len]) == bytes(w[2])
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
        seen.add(min(st, 0))
        if st > 0:
            assert int(rec["nerr"][0]) == 0 and cr.mr.syndrome(int(rec["type"]), rec["data"], int(rec["len"])) == 0, name
        else:
            assert rec.tobytes() == copies[i][0].tobytes(), name
    assert seen == {0, -1, -2, -3}


# ---- the align step for these types
def _align_run(kind, records, cuts, groups):
    sc = cs.scene(kind, clean=True)
    state = cr.new_state(groups, None, cr.LEARN | cr.MARK)
    outs = []
    for p in cs.cut(records, sc, cuts):
        out, _, state = cr.run(p.copy(), groups, state, cr.LEARN | cr.MARK, sc.window)
        outs.append(out)
    return np.concatenate(outs), state


@pytest.mark.parametrize("kind", KINDS)
def test_align_learns_the_offset_from_the_first_common_good_frame_and_marks_one_copy_per_frame(kind):
    sc = cs.scene(kind, clean=True)
    base = cs.oracle_frames(kind, clean=True)
    out, state = _align_run(kind, base, 4, sc.groups)
    for g, members in enumerate(sc.groups):
        assert all(state["locked"][ch] for ch in members), g
        for ch in members[1:]:       # the difference of the bit counts is the difference of the delays, to the chip
            assert abs(state["off"][ch] - state["off"][members[0]] - (sc.sonde[ch][1] - sc.sonde[members[0]][1])) <= 1, (g, ch)
        # one record per transmitted frame stays unmarked
        recs = [f for f in out if int(f["channel"]) in members]
        frames = {cs.frame_of(sc, f)[:2] for f in recs}
        unmarked = [cs.frame_of(sc, f)[:2] for f in recs if not int(f["flags"]) & cr.FRAME_DUPLICATE]
        assert sorted(unmarked) == sorted(frames), g
        assert state["duplicates"][g] == len(recs) - len(frames)
    # locking takes one pair of identical good frames: the first submit that holds a frame in two members
    first = cs.cut(base, sc, 4)[0]
    _, _, st = cr.run(first.copy(), sc.groups, cr.new_state(sc.groups, None, cr.LEARN | cr.MARK), cr.LEARN | cr.MARK, sc.window)
    assert all(st["locked"][ch] for ch in sc.groups[0]) and st["learned"][0] == 1


def test_align_follows_a_jump_and_failed_copies_teach_nothing():
    sc = cs.scene("m10", clean=True)
    base = cs.oracle_frames("m10", clean=True).copy()
    late = (base["channel"] == 3) & (base["bitpos"] > sc.nchips // 2)
    base["bitpos"][late] += 1500                                         # channel 3 idles for 1500 chips in mid-stream
    _, state = _align_run("m10", base, 10, sc.groups)
    assert abs(state["off"][3] - state["off"][2] - 1800) <= 1 and state["learned"][1] == 2
    failed = cs.oracle_frames("m10", clean=True).copy()
    failed["nerr"][failed["channel"] == 3, 0] = -1
    _, state = _align_run("m10", failed, 4, sc.groups)
    assert not state["locked"][3] and not state["locked"][2] and state["learned"][1] == 0


def test_a_failed_copy_beside_a_copy_the_manchester_rescue_corrected_stays_as_recorded():
    """cs.rescued_partner_scene through the SPEC 3.3f twin and then this one, the order the library runs them in"""
    import manchester_rescue_reference as mr
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
    rescued, how, _ = mr.rescue(first, mr.chips_of_streams(streams))
    out, outcomes, state = cr.diversity(rescued, sc.groups, None, sc.window)
    seen = {"rescued_partner": 0, "both_hidden": 0}
    for f, h, o, r in zip(rescued, how, outcomes, out):
        case = sc.plan[cs.frame_of(sc, f)[1]]
        if case is None:
            continue
        ch = int(f["channel"])
        seen[case] += ch == 0
        want = {("rescued_partner", 0): ("no_hint", "partner_good"), ("rescued_partner", 1): ("rescued", "good"),
                ("both_hidden", 0): ("no_hint", "combined"), ("both_hidden", 1): ("no_hint", "partner_good")}[(case, ch)]
        assert (h, o) == want, (case, ch, h, o)
        assert (r.tobytes() == f.tobytes()) == (o != "combined")
    assert seen["rescued_partner"] >= 3 and seen["both_hidden"] >= 3
    assert state["tried"] == state["combined"] == [seen["both_hidden"]]
