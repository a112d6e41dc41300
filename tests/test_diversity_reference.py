"""The twin of sonde_batch_set_diversity (tests/diversity_reference.py, DESIGN SPEC 3.3j) on the CPU oracle's records of the designed
scenes (tests/diversity_scenes.py): every case ends as designed, every combined record is the transmitted frame, untouched records
stay byte for byte, the counters are what the plan says, and however the stream is cut into submits a group delivers the same set
of distinct good frames with exactly one record rewritten per cluster of failed copies."""
import numpy as np
import pytest

import diversity_reference as dr
import diversity_scenes as ds

FAILED = {"too_many", "undecodable", "rejected"}


def _clusters(sc, records, outcomes):
    """{(stream, frame k): [(record index, outcome)]} over the records of grouped channels"""
    grouped = {ch for g in sc.groups for ch in g}
    cl = {}
    for i, f in enumerate(records):
        if int(f["channel"]) in grouped:
            stream, k, _ = ds.frame_of(sc, f)
            cl.setdefault((stream, k), []).append((i, outcomes[i]))
    return cl


def _good(f):
    return int(f["nerr"][0]) >= 0 and int(f["nerr"][1]) >= 0


@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
def test_every_case_ends_as_designed(extended):
    sc, fr = ds.scene(extended), ds.oracle_frames(extended)
    out, outcomes, st = dr.diversity(fr, sc.groups, sc.offsets, sc.window)
    seen, tried, combined = set(), [0] * len(sc.groups), [0] * len(sc.groups)
    group_of = {ch: g for g, m in enumerate(sc.groups) for ch in m}
    for (stream, k), members in _clusters(sc, fr, outcomes).items():
        case, expect = sc.plan[(stream, k)]
        ocs = [oc for _, oc in members]
        g = group_of[int(fr[members[0][0]]["channel"])]
        seen.add(case)
        if expect == "combined":
            assert ocs.count("combined") == 1 and all(oc in ("combined", "partner_good") for oc in ocs), (case, stream, k, ocs)
            tried[g] += 1
            combined[g] += 1
        elif expect in FAILED:
            assert all(oc == expect for oc in ocs), (case, stream, k, ocs)
            tried[g] += len(ocs)
        else:
            assert all(oc in ("good", "partner_good", "no_partner") for oc in ocs), (case, stream, k, ocs)
        for i, oc in members:
            tx = ds.frame_of(sc, fr[i])[2]
            if oc == "combined":
                K = len(members)
                assert bytes(out[i]["data"][:len(tx)]) == bytes(tx)
                assert int(out[i]["flags"]) == int(fr[i]["flags"]) | dr.FRAME_RESCUED | dr.FRAME_COMBINED | (K << 8)
                assert _good(out[i]) and not _good(fr[i])
                for c in (0, 1):        # a codeword that had failed: the bytes that changed; one that had not: untouched
                    diff = sum(1 for o in range(8, len(tx)) if ds.cw_of(o) == c and out[i]["data"][o] != fr[i]["data"][o])
                    assert int(out[i]["nerr"][c]) == (diff if int(fr[i]["nerr"][c]) < 0 else int(fr[i]["nerr"][c]))
                    assert diff == 0 or int(fr[i]["nerr"][c]) < 0
                for name in ("channel", "type", "len", "bitpos"):
                    assert out[i][name] == fr[i][name]
            else:
                assert out[i].tobytes() == fr[i].tobytes(), (case, stream, k, oc)
    want = set(ds.EXT_CASES if extended else ds.STD_CASES + ["triple", "triple_middle_clean", "lonely"])
    assert want <= seen, want - seen
    assert (st["tried"], st["combined"]) == (tried, combined)
    # channels in no group, and the pairs that can find no partner (too far apart; lengths differ)
    for i, f in enumerate(fr):
        if outcomes[i] in ("other", "no_partner", "good"):
            assert out[i].tobytes() == f.tobytes()
    if not extended:
        assert st["tried"][3:] == [0, 0] and outcomes.count("no_partner") >= 10 and outcomes.count("other") >= 5


@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
def test_the_cut_into_submits_changes_which_copy_not_which_frames(extended):
    sc, fr = ds.scene(extended), ds.oracle_frames(extended)
    delivered, counters = {}, {}
    for cuts in (1, 4, 10):
        state, parts, ocs = None, [], []
        for sub in ds.cut(fr, sc, cuts):
            o, oc, state = dr.diversity(sub, sc.groups, sc.offsets, sc.window, state)
            parts.append(o)
            ocs += oc
        out = np.concatenate(parts)
        assert len(out) == len(fr)
        cl = _clusters(sc, out, ocs)
        for (stream, k), members in cl.items():
            recs = [out[i] for i, _ in members]
            n_rewritten = sum(1 for r in recs if int(r["flags"]) & dr.FRAME_COMBINED)
            if sc.plan[(stream, k)][1] == "combined" and len(members) == len([1 for s, _ in sc.sonde if s == stream]):
                assert n_rewritten == 1, (cuts, stream, k, [oc for _, oc in members])
            else:
                assert n_rewritten == 0 or sc.plan[(stream, k)][1] == "combined"
        delivered[cuts] = {(stream, k) for (stream, k), members in cl.items() if any(_good(out[i]) for i, _ in members)}
        for (stream, k), members in cl.items():
            for i, _ in members:
                if _good(out[i]):
                    tx = ds.frame_of(sc, out[i])[2]
                    assert bytes(out[i]["data"][:len(tx)]) == bytes(tx)
        counters[cuts] = state["combined"]
    assert delivered[1] == delivered[4] == delivered[10] and len(delivered[1]) >= 8
    assert counters[1] == counters[4] == counters[10]


def test_combine_on_the_caller_made_cases():
    copies, n_copies, names = ds.unit_cases()
    assert len(copies) >= 180 and {2, 3, 4} <= set(n_copies.tolist())
    want = {"combined": None, "too_many": -1, "undecodable": -2}
    seen = set()
    for cp, K, name in zip(copies, n_copies, names):
        out, st = dr.combine(cp, K)
        seen.add(st if st < 0 else 0)
        base = name.replace("_swapped", "").rsplit("_", 1)[0]
        if base in ds.CASES and base != "partner_good":
            w = want[ds.CASES[base][2]]
            assert st == (int(K) if w is None else w), (name, st)
        if name == "triple_outer_two":
            assert st == -1
        if name in ("triple", "triple_reversed"):
            assert st == 3
        if name == "e24_and_a_common_error":
            assert st == -3
        if st < 0:
            assert out.tobytes() == cp[0].tobytes()
        else:
            assert st == int(K) and int(out["flags"]) == dr.FRAME_RESCUED | dr.FRAME_COMBINED | (int(K) << 8) and _good(out)
    assert seen == {0, -1, -2, -3}


def test_a_restarted_group_forgets_its_carried_records():
    sc, fr = ds.scene(), ds.oracle_frames()
    subs = ds.cut(fr, sc, 10)
    state = None
    for s, sub in enumerate(subs):
        if s == 5:
            for g in range(len(sc.groups)):
                dr.restart_group(state, sc.groups, g)
            assert not state["carried"] and not any(state["tried"])
        _, _, state = dr.diversity(sub, sc.groups, sc.offsets, sc.window, state)
    assert state["carried"]
