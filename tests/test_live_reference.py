"""The live receiver's host halves on the CPU (DESIGN SPEC 3.12): sonde_live_match against its Python twin, LivePolicy under scripts
(no GPU: candidates and detections in, actions and events out), and the scene gate of synth.make_wideband_scene."""
from __future__ import annotations

import numpy as np
import pytest

import live_reference as LR
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd import live
from sdrpp_radiosonde_amd.batch import SondeError

FS = 1_000_000
RS41, DFM, M10 = 0, 1, 3


# ---------------------------------------------------------------- the matching rule
# (vfos, candidates, match_hz, cand_of_vfo, vfo_of_cand)
MATCH_TABLE = [
    ([100_000], [100_000], 0, [0], [0]),                                   # an exact hit
    ([100_000], [110_000], 0, [0], [0]),                                   # just inside match_hz (the default, 10000)
    ([100_000], [110_001], 0, [-1], [-1]),                                 # just outside
    ([100_000], [89_999, 90_000], 0, [1], [-1, 0]),
    ([0], [2_500], 2_500, [0], [0]),
    ([0], [-2_501], 2_500, [-1], [-1]),
    ([100_000], [97_000, 102_000], 0, [1], [-1, 0]),                       # two candidates near one VFO: the nearer one
    ([100_000], [98_000, 102_000], 0, [0], [0, -1]),                       # ... a tie: the lower candidate index
    ([100_000, 108_000], [103_000], 0, [0, -1], [0]),                      # two VFOs near one candidate: the nearer one
    ([100_000, 106_000], [103_000], 0, [0, -1], [0]),                      # ... a tie: the lower VFO index
    ([106_000, 100_000], [103_000], 0, [0, -1], [0]),
    ([100_000, 104_000], [101_000, 103_500, 300_000], 0, [0, 1], [0, 1, -1]),
    ([], [1, 2], 0, [], [-1, -1]),                                         # empty lists
    ([5, 6], [], 0, [-1, -1], []),
    ([], [], 0, [], []),
    ([-499_000], [499_000], 0, [-1], [-1]),
]


def test_match_equals_the_twin_on_a_table():
    for v, c, hz, cv, vc in MATCH_TABLE:
        assert LR.match_ref(v, c, hz) == (cv, vc), (v, c, hz)
        a, b = live.match(v, c, hz)
        assert (a.tolist(), b.tolist()) == (cv, vc), (v, c, hz)


def test_match_equals_the_twin_on_random_lists():
    rng = np.random.default_rng(12)
    hits = 0
    for _ in range(1500):
        nv, nc = int(rng.integers(0, 9)), int(rng.integers(0, 12))
        step = int(rng.choice([1, 500, 5000]))                             # coarse grids make ties
        v = (rng.integers(-40, 40, nv) * step).tolist()
        c = (rng.integers(-40, 40, nc) * step).tolist()
        hz = int(rng.choice([0, 1, 2500, 10000, 40000]))
        a, b = live.match(v, c, hz)
        assert (a.tolist(), b.tolist()) == LR.match_ref(v, c, hz), (v, c, hz)
        hits += int((a >= 0).sum())
        for k, i in enumerate(a.tolist()):                                  # the two tables agree with each other
            assert i < 0 or b[i] == k
    assert hits > 1000


def test_match_needs_its_outputs():
    L = _lib.load()
    v = np.zeros(1, np.int32)
    assert L.sonde_live_match(v.ctypes.data, 1, v.ctypes.data, 1, 0, None, None) < 0
    assert b"sonde_live_match" in L.sonde_last_error()


# ---------------------------------------------------------------- the policy under scripts
S, P = 1_000_000, 2_000_000                    # one scan period and the probe time, in input samples


def _policy(cap=None, probes=2, **kw):
    return live.LivePolicy(FS, cap or {RS41: 2, DFM: 1, M10: 1}, probes, probe_samples=P, **kw)


def _kinds(pol):
    return [e[0] for e in pol.events]


def test_a_sonde_appears_is_probed_and_typed():
    pol = _policy()
    assert pol.slot_type == [RS41, RS41, DFM, M10] and pol.scan(S, []) == []
    assert pol.scan(2 * S, [123_400], [51.0]) == [("probe", 0, 123_400)]
    assert pol.scan(3 * S, [123_450], [52.0]) == [] and pol.probes_due(3 * S) == []          # being probed: not probed twice
    assert pol.probes_due(2 * S + P) == [0]
    # the decode slot goes where the candidate was seen last (a drifting carrier has moved on since the probe began)
    assert pol.probe_result(2 * S + P, 0, DFM) == [("release", 0), ("decode", 2, 123_450, DFM)]
    assert pol.events[-1] == ("found", 2 * S + P, 0, 123_450, DFM) and pol.probes == {} and pol.known == []
    assert pol.vfos[2]["id"] == 0 and not pol.hold(2)
    assert pol.vfos[2]["cn0"] == 52.0
    assert pol.scan(5 * S, [123_900], [50.0]) == [] and pol.vfos[2]["cn0"] == 50.0   # its own carrier: no new probe
    # a carrier whose 40 kHz probe VFO would not lie inside the band is left alone
    assert pol.scan(6 * S, [123_900, 485_000]) == []


def test_missed_scans_hold_then_the_sonde_returns_with_its_id():
    pol = _policy(lose_after=3)
    pol.add_initial(-200_000, RS41)
    pol.scan(S, [-200_100])
    assert not pol.hold(0)
    for k in (2, 3):                                                      # lose_after - 1 misses
        assert pol.scan(k * S, []) == [] and pol.hold(0)
    assert pol.scan(4 * S, [-199_000]) == [] and not pol.hold(0)
    assert pol.vfos[0]["id"] == 0 and pol.vfos[0]["misses"] == 0 and _kinds(pol) == ["found"]


def test_lost_after_lose_after_scans_and_the_slot_is_reused_with_a_new_id():
    pol = _policy(lose_after=3)
    assert pol.add_initial(300_000, M10) == ("decode", 3, 300_000, M10)
    pol.scan(S, [300_000])
    assert pol.scan(2 * S, []) == [] and pol.scan(3 * S, []) == []
    assert pol.scan(4 * S, []) == [("clear", 3)]
    assert pol.events[-1] == ("lost", 4 * S, 0, 300_000, M10) and pol.vfos == {} and pol.free[M10] == [3]
    assert pol.scan(5 * S, [-100_000]) == [("probe", 0, -100_000)]
    assert pol.probe_result(5 * S + P, 0, M10) == [("release", 0), ("decode", 3, -100_000, M10)]
    assert pol.vfos[3]["id"] == 1 and pol.events[-1] == ("found", 5 * S + P, 1, -100_000, M10)


def test_a_full_pool_is_logged_once_and_served_when_a_slot_frees():
    pol = _policy(lose_after=1)
    pol.add_initial(0, DFM)
    assert pol.scan(S, [0, 200_000]) == [("probe", 0, 200_000)]
    assert pol.probe_result(S + P, 0, DFM) == [("release", 0)]
    assert pol.events[-1] == ("full", S + P, -1, 200_000, DFM)
    for k in (4, 5):                                                      # typed already: neither probed nor logged again
        assert pol.scan(k * S, [0, 200_010]) == []
    assert _kinds(pol).count("full") == 1 and _kinds(pol).count("probe") == 1
    # the first DFM vanishes: its slot goes to the one that waited, at once
    assert pol.scan(6 * S, [200_020]) == [("clear", 2), ("decode", 2, 200_020, DFM)]
    assert [e[:3] for e in pol.events[-2:]] == [("lost", 6 * S, 0), ("found", 6 * S, 1)]


def test_undecided_max_probes_times_then_ignored_until_absent_once():
    pol = _policy(max_probes=3)
    n = S
    for k in range(3):
        assert pol.scan(n, [50_000]) == [("probe", 0, 50_000)], k
        assert pol.scan(n + S, [50_020]) == []
        n += P
        assert pol.probe_result(n, 0, -1) == [("release", 0)]
        n += S
    assert pol.events[-1][0] == "ignored" and _kinds(pol).count("probe") == 3
    for _ in range(4):
        assert pol.scan(n, [50_000]) == [] and pol.probes == {}
        n += S
    assert pol.scan(n, []) == [] and pol.known == []                     # absent from one scan
    assert pol.scan(n + S, [50_000]) == [("probe", 0, 50_000)]
    assert pol.vfos == {} and "found" not in _kinds(pol)


def test_candidates_wait_for_a_probe_slot_in_ascending_offset_order():
    pol = _policy(probes=2)
    cands = [300_000, -100_000, 100_000, -300_000]
    assert pol.scan(S, cands) == [("probe", 0, -300_000), ("probe", 1, -100_000)]
    assert pol.scan(2 * S, cands) == []                                   # none free
    assert pol.probe_result(S + P, 1, RS41) == [("release", 1), ("decode", 0, -100_000, RS41)]
    assert pol.scan(4 * S, cands) == [("probe", 1, 100_000)]
    assert pol.probe_result(S + P, 0, -1) == [("release", 0)]
    assert pol.scan(5 * S, cands) == [("probe", 0, -300_000)]             # tried once, not yet ignored: its turn comes before 300 000's
    assert sorted(q["offset"] for q in pol.probes.values()) == [-300_000, 100_000]


def test_capacity_forms_and_refusals():
    assert live.LivePolicy(FS, 2, 1, probe_samples=P).n_slots == 14
    with pytest.raises(SondeError):
        live.LivePolicy(FS, {}, 1, probe_samples=P)
    with pytest.raises(SondeError):
        live.LivePolicy(FS, {9: 1}, 1, probe_samples=P)
    with pytest.raises(SondeError):
        live.LivePolicy(FS, 1, 0, probe_samples=P)
    pol = _policy()
    pol.add_initial(0, DFM)
    with pytest.raises(SondeError, match="no free slot"):
        pol.add_initial(50_000, DFM)
    import sdrpp_radiosonde_amd as pkg
    assert pkg.LiveReceiver is live.LiveReceiver and pkg.LivePolicy is live.LivePolicy


def test_frame_ok_follows_the_parsers_rules():
    f = np.zeros(9, _lib.FRAME_DTYPE)
    f["type"] = [0, 0, 0, 1, 1, 2, 3, 3, 6]
    f["nerr"] = [[0, 2], [-1, 0], [3, -1], [3, 0], [0, 1], [1, 0], [0, 5], [-1, 0], [-1, 0]]
    assert live.frame_ok(f).tolist() == [True, False, False, True, False, True, True, False, False]
    assert live.frame_ok(f[:0]).shape == (0,)


# ---------------------------------------------------------------- the scene gate
def test_the_scene_gate_defaults_to_the_existing_scene():
    sondes = [(-300_000, 0), (100_000, 1)]
    n = 128_000
    a = synth.make_wideband_scene(sondes, n, fs=FS, seed=4)[0]
    b = synth.make_wideband_scene(sondes, n, fs=FS, seed=4, active=None)[0]
    c = synth.make_wideband_scene(sondes, n, fs=FS, seed=4, active=[None, None])[0]
    assert a.numpy().tobytes() == b.numpy().tobytes() == c.numpy().tobytes()
    g, frames, symbols = synth.make_wideband_scene(sondes, n, fs=FS, seed=4, active=[None, (40_000, 90_000)])
    only0 = synth.make_wideband_scene(sondes[:1], n, fs=FS, seed=4)
    assert frames[0] == only0[1][0] or all(np.array_equal(x[1], y[1]) for x, y in zip(frames[0], only0[1][0]))
    d = (g - a).numpy()
    assert not d[40_000:90_000].any() and d[:40_000].any() and d[90_000:].any()      # the second carrier is off the air outside its span
    e = (g - only0[0]).numpy()
    assert not e[:40_000].any() and not e[90_000:].any() and e[40_000:90_000].any()  # and nothing else is there (one noise floor, the same)
