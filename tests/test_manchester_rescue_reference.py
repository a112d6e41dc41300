"""CPU: the twin of SONDE_FLAG_MANCHESTER_RESCUE (tests/manchester_rescue_reference.py, DESIGN SPEC 3.3f) on the designed scenes of
tests/manchester_rescue_scenes.py, over the CPU oracle's records and chips (Channel.bits()): every case of the table gives the
outcome the SPEC says, every rescued frame is the transmitted one, the result does not depend on how the records are cut, a noisy
M10 scene gains frames and none of them is wrong, and the scenes tell seven mutations of the rule from the rule."""
import numpy as np
import pytest

import manchester_rescue_reference as mr
import manchester_rescue_scenes as ms

KINDS = ["m10", "m20", "mrz"]


def _twin(kind, **mut):
    fr, streams = ms.oracle_run(kind)
    return mr.rescue(fr, mr.chips_of_streams(streams), **mut)


def table_mismatches(kind, **mut):
    """records of the scene whose outcome, flip count or bytes are not what the table of cases says, under the (mutated) twin"""
    sc = ms.scene(kind)
    fr, _ = ms.oracle_run(kind)
    out, outcomes, _ = _twin(kind, **mut)
    bad, seen = [], {}
    for f0, f, oc in zip(fr, out, outcomes):
        pos, tx = ms.tx_of(sc, f)
        case = sc.plan[(int(f["channel"]), pos)]
        want, flips = ms.EXPECT[case]
        seen[case] = seen.get(case, 0) + 1
        ok = oc == want and mr.FRAME_RESCUED * (want == "rescued") == int(f["flags"]) & mr.FRAME_RESCUED and ((int(f["flags"]) >> 8) & 0xF) == flips
        if want in ("rescued", "clean"):
            ok = ok and int(f["nerr"][0]) == 0 and np.array_equal(f["data"][:sc.len], tx[:sc.len])
        else:
            ok = ok and f.tobytes() == f0.tobytes()
        if case == "second1":
            ok = ok and int(f["nerr"][1]) == 1
        if not ok:
            bad.append((int(f["channel"]), pos, case, oc))
    return bad, seen


@pytest.mark.parametrize("kind", KINDS)
def test_every_case_of_the_table(kind):
    sc = ms.scene(kind)
    fr, streams = ms.oracle_run(kind)
    assert len(fr) == sum(len(v) for v in sc.frames) and set(fr["type"]) == {sc.type} and set(fr["len"]) == {sc.len}
    bad, seen = table_mismatches(kind)
    assert not bad, bad
    for case in ms.CASES[kind]:
        assert seen.get(case, 0) >= 2, (case, seen)
    # |V| is the recorded nerr[1] (SPEC step 1), and only the named fields of a rescued record change
    out, outcomes, state = _twin(kind)
    get = mr.chips_of_streams(streams)
    for f0, f, oc in zip(fr, out, outcomes):
        assert len(mr.violations(sc.type, sc.len, int(f0["bitpos"]), get, int(f0["channel"]))) == int(f0["nerr"][1])
        assert all(f[k] == f0[k] for k in ("channel", "type", "len", "bitpos")) and f["nerr"][1] == f0["nerr"][1] and (f["flags"] ^ f0["flags"]) & 1 == 0
        assert not f["data"][sc.len:].any()
    for c in range(sc.C):
        mine = [oc for f, oc in zip(fr, outcomes) if int(f["channel"]) == c]
        st = state.get(c, mr.new_state())
        assert st == {"tried": sum(oc in ("unsolved", "ambiguous", "rescued") for oc in mine), "rescued": mine.count("rescued")}


def test_columns_are_the_change_of_the_syndrome():
    rng = np.random.default_rng(5)
    for kind, ln in ((mr.M10, 101), (mr.M10, 70), (mr.MRZN1, 45)):
        d = rng.integers(0, 256, size=ln, dtype=np.uint8)
        s = mr.syndrome(kind, d, ln)
        for k in list(range(0, 24)) + [int(v) for v in rng.integers(0, 8 * ln, size=40)] + list(range(8 * ln - 16, 8 * ln)):
            e = d.copy()
            e[k // 8] ^= 0x80 >> (k % 8)
            assert mr.syndrome(kind, e, ln) ^ s == mr.column(kind, ln, k), (kind, ln, k)


def test_dependent_four_is_dependent():
    for kind, (typ, _, _, _, ln, _, _) in ms.KINDS.items():
        (a, b), (c, d) = ms.dependent_four(kind)
        assert len({a, b, c, d}) == 4 and min(a, b, c, d) >= 8
        assert mr.column(typ, ln, a) ^ mr.column(typ, ln, b) ^ mr.column(typ, ln, c) ^ mr.column(typ, ln, d) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_cut_invariance_of_the_twin(kind):
    fr, streams = ms.oracle_run(kind)
    get = mr.chips_of_streams(streams)
    whole, oc_whole, st_whole = mr.rescue(fr, get)
    order = np.lexsort((fr["channel"], fr["bitpos"]))              # time order: what successive submits deliver
    parts, state = [], {}
    for piece in np.array_split(order, 3):
        out, _, state = mr.rescue(fr[np.sort(piece)], get, state)
        parts.append(out)
    got = np.concatenate(parts)
    got = got[np.lexsort((got["bitpos"], got["channel"]))]
    assert got.tobytes() == whole.tobytes() and state == st_whole


def test_noisy_m10_scene_gains_frames_and_none_is_wrong():
    sc = ms.noisy_scene()
    fr, streams = ms.oracle_run("noisy")
    out, outcomes, _ = mr.rescue(fr, mr.chips_of_streams(streams))
    n_res = wrong = 0
    for f, oc in zip(out, outcomes):
        if oc != "rescued":
            continue
        n_res += 1
        hit = ms.tx_of(sc, f)
        wrong += hit is None or not np.array_equal(f["data"][:101], hit[1])
    print("noisy scene: records", len(fr), "clean", int((fr["nerr"][:, 0] == 0).sum()), "rescued", n_res, "wrong", wrong)
    assert n_res >= 30 and wrong == 0


MUTATIONS = {"cap_7": dict(cap=7), "cap_9": dict(cap=9), "first_solution": dict(first_solution=True), "no_check_columns": dict(check_cols=False),
             "m20_rows_as_m10": dict(m20_rows_as_m10=True), "mrz_columns_from_ffff": dict(mrz_col_start=0xFFFF), "no_byte0_rule": dict(byte0_rule=False)}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_scenes_reject_a_mutated_rule(name):
    bad = {kind: table_mismatches(kind, **MUTATIONS[name])[0] for kind in KINDS}
    assert any(bad.values()), name
    # and each where it must: the MRZ-N1 mutation on MRZ-N1, the M20 one on M20, the length-byte one on M10 / M20
    must = {"m20_rows_as_m10": ["m20"], "mrz_columns_from_ffff": ["mrz"], "no_byte0_rule": ["m10", "m20"]}.get(name, KINDS)
    for kind in must:
        assert bad[kind], (name, kind)
