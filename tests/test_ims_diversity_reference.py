"""The twin of sonde_batch_set_diversity for iMS-100 groups (tests/ims_diversity_reference.py, DESIGN SPEC 3.3n) on the CPU oracle's records
and chips of the designed scene (tests/ims_diversity_scenes.py): every case ends as the scene plan says, every combined record is the
transmitted frame, each mutation of the rule's constants changes the case that is there to catch it, the set of frames a group
delivers does not depend on how the stream is cut, and a copy that arrives a submit late is combined from the carried record and the
chips at its position; a group whose offset is wrong by one frame changes nothing; a record whose nerr[1] is not what its chips say
is left out.  Then the align twin for iMS-100, and the pass behind the SPEC 3.3h twin."""
import numpy as np
import pytest

import ims_diversity_reference as cr
import ims_diversity_scenes as cs
import ims_rescue_reference as ir

NAME = {-1: "guard", -2: "none", -3: "several"}
TRIED = ("combined", "guard", "none", "several")


def _by_frame(sc, records, outcomes):
    got = {}
    for f, o in zip(records, outcomes):
        w = cs.frame_of(sc, f)
        assert w is not None, (int(f["channel"]), int(f["bitpos"]))
        got.setdefault(w[:2], []).append((f, o, w[2]))
    return got


def _twin(sc, **mut):
    base, streams = cs.oracle_run()
    return base, cr.diversity(base.copy(), sc.groups, ir.chips_of_streams(streams), sc.offsets, sc.window, **mut)


def test_every_case_ends_as_planned_and_combined_records_are_the_transmitted_frames():
    sc = cs.scene()
    base, (out, outcomes, state) = _twin(sc)
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
        status, J = cs.EXPECT[case][1:3]
        if case == "wrong_offset":                              # each copy meets a copy of the neighbouring frame, or nothing at the scene's ends
            assert set(oc) <= {"guard", "no_partner", "partner_good"}, (key, oc)
        elif expect == "combined":
            n_combined += 1
            assert oc.count("combined") == 1, (key, case, oc)
            f, _, tx = next(r for r in recs if r[1] == "combined")
            assert bytes(f["data"][:51]) == bytes(tx) and int(f["nerr"][1]) == 0 and int(f["nerr"][0]) >= 3, (key, case)
            assert (int(f["flags"]) & 0xFF06) == (2 | 4 | (copies << 8) | (J << 12)), (key, case, hex(int(f["flags"])))
            assert cr.joint(f["flags"]) == J and cr.copies_of(f["flags"]) == copies
            if key[0] != cs.DELAYED_STREAM:                     # copy 0 is visited first and combined; the others then find it good
                assert oc == ["combined"] + ["partner_good"] * (copies - 1), (key, case, oc)
            else:
                assert sorted(oc) == ["combined", "partner_good"], (key, case, oc)
        elif expect == "miscorrected":                          # dist6: copy 0 has no solution; copy 1 is completed around its miscorrection
            n_combined += 1
            assert oc == ["none", "combined"], (key, oc)
            f, _, tx = recs[1]
            assert bytes(f["data"][:51]) != bytes(tx) and int(f["nerr"][1]) == 0
        elif case == "partner_good":
            assert sorted(oc) == ["good", "partner_good"], (key, oc)
        elif case == "lonely":
            assert set(oc) == {"other"}, (key, oc)
        else:
            assert set(oc) == {NAME[status]}, (key, case, oc)
    assert seen == set(cs.EXPECT) - {None}
    assert sum(state["combined"]) == n_combined >= 25
    assert sum(state["tried"]) == sum(1 for o in outcomes if o in TRIED) and "left_out" not in outcomes
    untouched = [i for i, o in enumerate(outcomes) if o != "combined"]
    assert out[untouched].tobytes() == base[untouched].tobytes()
    assert state["combined"][cs.WRONG_GROUP] == 0 and state["tried"][cs.WRONG_GROUP] >= 16


@pytest.mark.parametrize("case", sorted(c for c, e in cs.EXPECT.items() if e[3] is not None))
def test_each_mutation_changes_the_case_it_is_there_to_catch(case):
    sc = cs.scene()
    _, (_, plain, _) = _twin(sc)
    base, (out, mutated, _) = _twin(sc, **cs.EXPECT[case][3])
    got_plain, got_mut = _by_frame(sc, base, plain), _by_frame(sc, out, mutated)
    keys = [k for k, (c, _) in sc.plan.items() if c == case]
    assert len(keys) >= 2
    changed = 0
    for key in keys:
        before, after = [o for _, o, _ in got_plain[key]], [o for _, o, _ in got_mut[key]]
        assert "combined" not in before[:1], (key, before)
        changed += "combined" in after and "combined" not in before[:1] and after[0] == "combined"
    assert changed >= (len(keys) if case != "wrong_offset" else len(keys) // 2), (case, changed, len(keys))


def test_the_delivered_frames_do_not_depend_on_the_cut_and_a_late_copy_is_combined_from_the_carried_record():
    sc = cs.scene()
    base, streams = cs.oracle_run()
    chips = ir.chips_of_streams(streams)

    def delivered(parts):
        state, good, late = None, set(), 0
        for p in parts:
            before = {ch: r.copy() for ch, r in (state["carried"].items() if state else [])}
            out, outcomes, state = cr.diversity(p.copy(), sc.groups, chips, sc.offsets, sc.window, state)
            for f, o in zip(out, outcomes):
                w = cs.frame_of(sc, f)
                if int(f["nerr"][1]) == 0:
                    good.add(w[:2])
                if o == "combined":
                    here = sum(1 for q in p if cs.frame_of(sc, q)[:2] == w[:2])
                    if here < cr.copies_of(f["flags"]) and any(cs.frame_of(sc, c)[:2] == w[:2] for c in before.values()):
                        late += 1                               # a copy it was made from came with an earlier submit
        return good, late, state

    whole, _, st1 = delivered([base])
    for cuts in (3, 5, 9):
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
    records, n_copies, blocks, names, want = cs.unit_cases()
    seen = set()
    for i, name in enumerate(names):
        rec, st = cs.twin_unit(records, n_copies, blocks, i)
        if want[i] is not None:
            assert st == want[i], (name, st, want[i])
        seen.add(st)
        if st > 0:
            assert st == n_copies[i] and int(rec["nerr"][1]) == 0 and int(rec["nerr"][0]) > int(records[i]["nerr"][0]), name
            assert rec["data"][51:].tobytes() == records[i]["data"][51:].tobytes()
            got = cs.tx_blocks(rec["data"])                     # the record now holds twelve codewords' data bits; those of F are decoded values
            assert all(ir.poly_mod(b) == 0 for b in got)
        else:
            assert rec.tobytes() == records[i].tobytes(), name
    assert seen == {2, 3, 4, 0, -1, -2, -3}


def test_the_constants_of_the_rule():
    assert (cr.MIN_AGREED, cr.MAX_DIFFER, cr.MAX_DIST, cr.CAP, cr.WINDOW) == (6, 1, 5, 6, 576)
    # |V| <= 4: two fitting subsets would differ by a codeword of weight <= 4, and the code's distance is 5
    assert min(bin(ir.encode(d)).count("1") for d in range(1, 1 << 12)) >= 5


def test_a_record_whose_count_is_not_what_its_chips_say_is_left_out():
    sc = cs.scene()
    base, streams = cs.oracle_run()
    chips = ir.chips_of_streams(streams)
    _, plain, _ = cr.diversity(base.copy(), sc.groups, chips, sc.offsets, sc.window)
    i = next(i for i, o in enumerate(plain) if o == "combined" and int(base[i]["channel"]) == 0)
    patched = base.copy()
    patched[i]["nerr"][1] += 1
    out, outcomes, state = cr.diversity(patched, sc.groups, chips, sc.offsets, sc.window)
    assert outcomes[i] == "left_out" and out[i].tobytes() == patched[i].tobytes()
    # its partner, visited next, finds it failed but no longer fit to serve: left out as well, and neither counts as tried
    j = next(j for j in range(len(base)) if int(base[j]["channel"]) == 1 and abs(int(base[j]["bitpos"]) - int(base[i]["bitpos"])) < 64)
    assert outcomes[j] == "left_out"
    whole = cr.diversity(base.copy(), sc.groups, chips, sc.offsets, sc.window)[2]
    assert state["tried"][0] == whole["tried"][0] - 1 and state["combined"][0] == whole["combined"][0] - 1
    # chips that are no longer held: the same
    gone = lambda ch, start, count: None if ch == 1 else chips(ch, start, count)      # noqa: E731
    _, oc, st = cr.diversity(base.copy(), sc.groups, gone, sc.offsets, sc.window)
    assert st["tried"][0] == 0 and {o for o, f in zip(oc, base) if int(f["channel"]) in (0, 1)} <= {"good", "left_out", "partner_good"}


# ---- the align step for iMS-100 groups
MODE = cr.LEARN | cr.MARK


def _align_run(records, streams, cuts, sc):
    state = cr.new_state(sc.groups, None, MODE)
    chips = ir.chips_of_streams(streams)
    outs = []
    for p in cs.cut(records, sc, cuts):
        out, _, state = cr.run(p.copy(), sc.groups, chips, state, MODE, sc.window)
        outs.append(out)
    return np.concatenate(outs), state


@pytest.mark.parametrize("cuts", [1, 2])
def test_align_learns_the_offsets_and_marks_all_but_one_copy_per_frame(cuts):
    sc = cs.scene(clean=True, align=True)
    base, streams = cs.oracle_run(clean=True, align=True)
    out, state = _align_run(base, streams, cuts, sc)
    for g, members in enumerate(sc.groups):
        assert all(state["locked"][ch] for ch in members), g
        for ch in members[1:]:       # the difference of the chip counts is the difference of the delays, to the chip
            assert abs(state["off"][ch] - state["off"][members[0]] - (sc.sonde[ch][1] - sc.sonde[members[0]][1])) <= 1, (g, ch)
        if g == 2:                   # a copy two frame periods late goes unmarked (SPEC 3.3k: later than one frame period after the first)
            continue
        recs = [f for f in out if int(f["channel"]) in members]
        frames = {cs.frame_of(sc, f)[:2] for f in recs}
        unmarked = [cs.frame_of(sc, f)[:2] for f in recs if not int(f["flags"]) & cr.FRAME_DUPLICATE]
        assert sorted(unmarked) == sorted(frames), g
        assert state["duplicates"][g] == len(recs) - len(frames)


def test_align_on_the_damaged_scene_locks_at_the_first_frame_and_every_combined_frame_is_right():
    sc = cs.scene(align=True)
    base, streams = cs.oracle_run(align=True)
    out, state = _align_run(base, streams, 2, sc)
    assert all(state["locked"][ch] for members in sc.groups for ch in members)
    # the learned offsets are the true ones, so the pair that set_diversity's given offset puts one frame off combines here
    comb = out[out["flags"] & cr.FRAME_COMBINED != 0]
    assert len(comb) == sum(state["div"]["combined"]) >= 25
    wrong = 0
    for f in comb:
        s, k, tx = cs.frame_of(sc, f)
        wrong += bytes(f["data"][:51]) != bytes(tx)
        assert bytes(f["data"][:51]) == bytes(tx) or sc.plan[(s, k)][0] == "dist6"
    assert wrong == sum(1 for c, _ in sc.plan.values() if c == "dist6")


def test_the_align_unit_cases_end_as_they_are_named():
    cases = {c["name"]: cs.twin_align_case(c) for c in cs.align_unit_cases()}
    for name in ("same_key_byte_0_differs", "same_key_byte_43_differs", "same_key_words_0_to_10_differ", "byte_44_differs", "byte_47_differs",
                 "byte_48_differs", "last_byte_differs", "same_bytes_other_len", "failed_copies_teach_nothing", "two_sondes"):
        assert cases[name][2:] == (0, 0, 0), name
    for name in ("byte_behind_the_frame_differs_and_matches", "bytes_behind_the_frame_differ_in_the_carried", "pair_lock"):
        assert cases[name][2:] == (3, 1, 1), name
    assert cases["a_jump_is_followed"][1][:2] == [0, 467] and cases["rebase_higher"][1][:2] == [0, 450]
    assert cases["four_copies"][2:] == (15, 3, 3)


def test_a_failed_copy_beside_a_copy_the_ims_rescue_completed_stays_as_recorded():
    """cs.rescued_partner_scene through the SPEC 3.3h twin and then this one, the order the library runs them in"""
    sc = cs.rescued_partner_scene()
    first, streams = cs.rescued_partner_oracle()
    chips = ir.chips_of_streams(streams)
    rescued, how, _ = ir.rescue(first, chips)
    out, outcomes, state = cr.diversity(rescued, sc.groups, chips, None, sc.window)
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
        if o == "combined":
            assert bytes(r["data"][:51]) == bytes(cs.frame_of(sc, f)[2])
    assert seen["rescued_partner"] >= 3 and seen["both_hidden"] >= 3
    assert state["tried"] == state["combined"] == [seen["both_hidden"]]
