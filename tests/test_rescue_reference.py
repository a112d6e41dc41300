"""The twin of SONDE_FLAG_RS41_RESCUE (tests/rescue_reference.py, DESIGN SPEC 3.3c) proved on the CPU before a GPU sees it: the
oracle's frame records of 40 dB signals with byte errors injected into the on-air bits go through the twin, and every record is
checked against what was transmitted and what was injected."""
import numpy as np
import pytest

import rescue_reference as rr
import rescue_scenes as rs


def _check_scene(extended):
    sc = rs.scene(extended)
    ref = rs.oracle_frames(extended)
    out, outcomes, state = rr.rescue(ref)
    assert len(out) == len(ref) > 0
    seen = {}
    for f0, f1, oc in zip(ref, out, outcomes):
        c = int(f0["channel"])
        pos, tx = rs.tx_of(sc, f0)
        case, cnt = sc.plan[(c, pos)]
        key = (case, (c, pos) in sc.early)
        seen.setdefault(key, []).append(oc)
        failed = [int(v) < 0 for v in f0["nerr"]]
        if oc == "rescued":
            assert any(failed) and case is not None
            assert np.array_equal(f1["data"][8:sc.flen], tx[8:]), (c, pos, case)
            assert not f1["data"][sc.flen:].any()
            for cw in (0, 1):
                if failed[cw]:
                    assert f1["nerr"][cw] == cnt[cw], (c, pos, case, cw, f1["nerr"], cnt)
                else:
                    assert f1["nerr"][cw] == f0["nerr"][cw]
            assert f1["flags"] == f0["flags"] | rr.FRAME_RESCUED
            assert (f1["len"], f1["bitpos"], f1["channel"], f1["type"]) == (f0["len"], f0["bitpos"], f0["channel"], f0["type"])
        else:
            assert f1.tobytes() == f0.tobytes(), (c, pos, case, oc)
        if oc == "clean":
            assert not any(failed)
        # the case decides the outcome
        if case is None:
            assert oc == "clean", (c, pos, oc)
        elif (c, pos) in sc.early:
            assert oc == "no_layout", (c, pos, case, oc)
        else:
            assert oc == rs.EXPECT[case], (c, pos, case, oc, f0["nerr"])
    return seen, state, outcomes


def test_standard_frames_every_case_of_the_table():
    seen, state, outcomes = _check_scene(False)
    for case in rs.STD_CASES:
        assert len(seen.get((case, False), [])) >= 2, (case, {k: len(v) for k, v in seen.items()})
    assert len(seen.get(("meas_burst40", True), [])) >= 2                 # damaged before the first clean frame: not rescued ...
    for oc in ("clean", "no_layout", "too_many", "undecodable", "rescued"):
        assert outcomes.count(oc) >= 2, (oc, outcomes)
    # ... and the same damage in a later frame of the same channels is
    sc = rs.scene(False)
    for c in (sc.C - 2, sc.C - 1):
        assert state[c]["rescued"] >= 1 and state[c]["tried"] == state[c]["rescued"]
        assert state[c]["lay"][320] == [(o, t, ln) for o, (t, ln) in zip(rs.STD_OFFSETS, rs.synth.RS41_SUBFRAMES_STD)]
        assert state[c]["lay"][518] == []
    assert sum(st["tried"] for st in state.values()) == sum(oc in ("too_many", "undecodable", "rejected", "rescued") for oc in outcomes)


def test_extended_frames():
    seen, state, outcomes = _check_scene(True)
    assert len(seen.get(("gpspos_whole", False), [])) >= 2 and set(seen[("gpspos_whole", False)]) == {"rescued"}
    assert len(seen.get(("xdata_burst30", False), [])) >= 2 and set(seen[("xdata_burst30", False)]) == {"too_many"}
    assert outcomes.count("no_layout") >= 2
    assert all(len(st["lay"][518]) == 7 and st["lay"][320] == [] for st in state.values())


def test_result_does_not_depend_on_how_the_records_are_cut():
    ref = rs.oracle_frames(False)
    whole, _, st_whole = rr.rescue(ref)
    # per channel in three pieces by time, the state carried
    state, parts = {}, []
    order = np.argsort(ref["bitpos"], kind="stable")
    for piece in np.array_split(order, 3):
        sub = ref[np.sort(piece)]                      # (channel, time) order inside the piece
        out, _, state = rr.rescue(sub, state)
        parts.append(out)
    got = np.concatenate(parts)
    got = got[np.lexsort((got["bitpos"], got["channel"]))]
    assert got.tobytes() == whole.tobytes()
    assert state == st_whole


@pytest.mark.parametrize("n", [156, 255])
def test_decoder_at_and_beyond_the_bound(n):
    rng = np.random.default_rng(n)
    for e, v, ok in [(0, 12, True), (0, 13, False), (1, 11, True), (12, 6, True), (12, 7, False), (23, 0, True), (23, 1, False), (24, 0, True), (25, 0, False)]:
        cw = rr.rs_encode(rng.integers(0, 256, size=n - 24))
        assert not any(rr.syndromes(cw))
        pos = rng.choice(n, size=e + v, replace=False)
        er = np.zeros(n, dtype=np.uint8)
        er[pos[:e]] = 1
        r = list(cw)
        for k in pos:
            r[k] ^= int(rng.integers(1, 256))
        if e:
            r[pos[0]] = cw[pos[0]]                     # an erased byte that happens to be right
        st, w = rr.rs_decode_ee(r, er)
        if ok:
            assert st == e + v - (1 if e else 0) and w == cw, (e, v, st)
        else:
            assert st == -1 and w == r, (e, v, st)
