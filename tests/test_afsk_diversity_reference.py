"""The twin of sonde_batch_set_diversity for iMet and SRS-C50 groups (tests/afsk_diversity_reference.py, DESIGN SPEC 3.3o) over the
CPU oracle's records of the designed scenes (tests/afsk_diversity_scenes.py): every planned case has its outcome, every combined record
is the transmitted packet, and the result does not depend on the cut into submits.  No GPU."""
import numpy as np
import pytest

import afsk_diversity_reference as ad
import afsk_diversity_scenes as ds

KINDS = ["imet", "c50"]
COMBINED = ad.FRAME_COMBINED


def run_twin(sc, records, cuts=1):
    state = ad.new_div_state(sc.groups)
    outs = []
    for part in ds.cut(records, sc, cuts):
        out, _, state = ad.diversity(part, sc.groups, sc.offsets, 0, state)
        outs.append(out)
    return ds.sort_records(np.concatenate(outs)), state


@pytest.fixture(scope="module", params=KINDS)
def ran(request):
    kind = request.param
    sc = ds.scene(kind)
    fr = ds.oracle_frames(kind)
    out, state = run_twin(sc, fr.copy())
    return kind, sc, fr, out, state


def by_packet(sc, records):
    got = {}
    for f in records:
        hit = ds.frame_of(sc, f)
        if hit:
            got.setdefault(hit[:2], []).append(f)
    return got


def received_as_planned(sc, s, k, recs):
    """every receiver's first pass recorded packet k of stream s once, with exactly the planned damage (the demodulators lose a
    packet now and then, most of them while a channel settles: such an occurrence of a case shows nothing)"""
    tx = sc.stream_frames[s][k][1]
    chans = [ch for ch, (t, _) in enumerate(sc.sonde) if t == s]
    dmg = sc.damage[(s, k)]
    for no, ch in enumerate(chans):
        mine = [f for f in recs if int(f["channel"]) == ch]
        d = dmg[no] if no < len(dmg) else []
        if sc.plan[(s, k)][0] == "xdata_len_byte" and d and d[0] < 24:      # the framer took another length: nothing of the packet's own
            if any(int(f["len"]) == len(tx) for f in mine):
                return False
            continue
        want = ds.make_record(sc.kind, tx, d)
        if len(mine) != 1 or int(mine[0]["len"]) != len(tx) or bytes(mine[0]["data"][:len(tx)]) != bytes(want["data"][:len(tx)]):
            return False
    return True


def test_every_planned_case_has_its_outcome(ran):
    kind, sc, fr, out, _ = ran
    got, first = by_packet(sc, out), by_packet(sc, fr)
    seen = {}
    grouped = {ch for g in sc.groups for ch in g}
    for (s, k), (case, expect) in sc.plan.items():
        if not received_as_planned(sc, s, k, first.get((s, k), [])):
            continue
        recs = got[(s, k)]
        n_comb = sum(1 for f in recs if int(f["flags"]) & COMBINED)
        if expect == "combined":
            tx = sc.stream_frames[s][k][1]
            assert n_comb == 1, (s, k, case)
            f = next(f for f in recs if int(f["flags"]) & COMBINED)
            assert int(f["channel"]) in grouped and int(f["nerr"][0]) == 0 and bytes(f["data"][:len(tx)]) == bytes(tx)
            assert (int(f["flags"]) >> 8) & 0xF == ds.EXPECT[case][1]
            # one good copy per transmitted packet, and the other copies stay failed as recorded
            assert sum(1 for f in recs if int(f["nerr"][0]) >= 0) == 1
        else:
            assert n_comb == 0, (s, k, case)
        seen[case] = seen.get(case, 0) + 1
    for case in ds.PAIR_CASES[kind] + ds.TRIPLE_CASES + ds.QUAD_CASES + ["lonely"]:
        assert seen.get(case, 0) >= 2, (case, seen)
    # the packet the late cut falls into is among them
    late = (ds.DELAYED_STREAM, sc.late_cut_packet)
    assert received_as_planned(sc, *late, first.get(late, []))


def test_every_combined_record_is_the_transmitted_packet_and_there_are_enough(ran):
    kind, sc, fr, out, state = ran
    comb = out[(out["flags"] & COMBINED) != 0]
    assert len(comb) >= 12 and sum(state["combined"]) == len(comb)
    pairs = set()
    for f in comb:
        hit = ds.frame_of(sc, f)
        assert hit is not None
        tx = hit[2]
        assert int(f["len"]) == len(tx) and bytes(f["data"][:len(tx)]) == bytes(tx)
        pairs.add(((int(f["flags"]) >> 8) & 0xF, ad.unknowns(f["flags"])))
    assert {c for c, _ in pairs} == {2, 3, 4}
    # nothing but the combined records changed
    same = (out["flags"] & COMBINED) == 0
    assert out[same].tobytes() == fr[same].tobytes()
    if kind == "imet":
        assert {int(f["len"]) for f in comb} >= {14, 18, 13}


@pytest.mark.parametrize("cuts", [4, 8])
def test_the_cut_into_submits_changes_only_which_copy_is_rewritten(ran, cuts):
    kind, sc, fr, out, state = ran
    out2, state2 = run_twin(sc, fr.copy(), cuts)
    # iMet's delayed pair is left out: its second copy comes 300 symbols late, behind the stream's next packet, so where a cut falls
    # between the two the first copy is no longer its member's carried record (SPEC 3.3o "Limits"): a cut can only lose such a packet
    skip = {1} if kind == "imet" else set()
    for g in range(len(sc.groups)):
        if g in skip:
            assert state2["combined"][g] <= state["combined"][g]
        else:
            assert state2["combined"][g] == state["combined"][g] and state2["tried"][g] == state["tried"][g]
    chans = {ch for g, m in enumerate(sc.groups) if g not in skip for ch in m}
    good = lambda o: sorted((ds.frame_of(sc, f)[:2], bytes(f["data"][:int(f["len"])])) for f in o      # noqa: E731
                            if int(f["flags"]) & COMBINED and int(f["channel"]) in chans)
    assert good(out2) == good(out)


def test_clean_scene_is_unchanged():
    for kind in KINDS:
        sc = ds.scene(kind, clean=True)
        fr = ds.oracle_frames(kind, clean=True)
        out, state = run_twin(sc, fr.copy())
        assert out.tobytes() == fr.tobytes() and not any(state["tried"]) and not any(state["combined"])


def test_unit_cases_have_their_status():
    copies, n_copies, names, want = ds.unit_cases()
    seen = set()
    for row, K, name, st in zip(copies, n_copies, names, want):
        out, got = ad.combine(row, int(K))
        seen.add(got)
        if st is not None:
            assert got == st, (name, got, st)
        if got > 0:
            assert int(out["nerr"][0]) == 0 and int(out["flags"]) & COMBINED and (int(out["flags"]) >> 8) & 0xF == K
        else:
            assert out.tobytes() == row[0].tobytes()
    assert seen == {2, 3, 4, -1, -2, -3}


def test_align_twin_locks_marks_ptu_and_gps_and_no_xdata():
    sc = ds.scene("imet", align=True)
    fr = ds.oracle_frames("imet", align=True)
    state = ad.new_state(sc.groups, None, ad.LEARN | ad.MARK)
    out, _, state = ad.run(fr.copy(), sc.groups, state, ad.LEARN | ad.MARK, 0)
    assert all(state["locked"].values())
    d = [state["off"][ch] - state["off"][6] for ch in (7, 8)]
    assert abs(d[0] - 300) <= 7 and abs(d[1] - 5000) <= 7      # the demodulators' delays lie 6..13 symbols: two differ by at most 7
    dup = (out["flags"] & ad.FRAME_DUPLICATE) != 0
    assert not (dup & (out["len"] == 13)).any() and not (dup & (out["nerr"][:, 0] < 0)).any()
    # of the good PTU / GPS copies of one transmitted packet all but one are marked
    grouped = {ch for g in sc.groups for ch in g}
    checked = 0
    for (s, k), recs in by_packet(sc, out).items():
        ok = [f for f in recs if int(f["channel"]) in grouped and int(f["nerr"][0]) >= 0 and int(f["len"]) in (14, 18)]
        if len(ok) >= 2:
            assert sum(1 for f in ok if not int(f["flags"]) & ad.FRAME_DUPLICATE) == 1, (s, k)
            checked += 1
    assert checked >= 20 and sum(state["duplicates"]) >= checked
    # and the pass behind the step combines at the learned offsets
    assert sum(state["div"]["combined"]) >= 12
