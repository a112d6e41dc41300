"""-m gpu: SONDE_FLAG_RS41_RESCUE (DESIGN SPEC 3.3c) against its twin (tests/rescue_reference.py) on the scenes of
tests/test_rescue_reference.py: with the flag the records are the twin's over the oracle's, whole records byte for byte, and
rescue_info reports the twin's layouts and counters; without it they are the oracle's; a clean scene does not change; the result
does not depend on how the stream is cut into submits, on time slices, on where the RS stage runs or on the completion mode; in
a mixed batch only RS41 records change; a restarted channel starts without a layout; poll() delivers the rescued block."""
import functools

import numpy as np
import pytest
import torch

import rescue_reference as rr
import rescue_scenes as rs
from rescue_gpu_harness import run, sorted_frames as _sorted
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCUE = _lib.FLAG_RS41_RESCUE
_dev_cache = {}
_run = functools.partial(run, tile=rs.TILE)


def _iq(extended=False, clean=False):
    key = (extended, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(rs.scene(extended, clean).iq).to(DEV)
    return _dev_cache[key]


def _layouts(st):
    return {flen: [tuple(int(v) for v in e) for e in st["lay"][flen]] for flen in (320, 518)}


@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
def test_flag_on_records_are_the_twins(extended):
    sc = rs.scene(extended)
    want, outcomes, state = rr.rescue(rs.oracle_frames(extended))
    assert outcomes.count("rescued") >= 2
    got, b = _run(_iq(extended), RESCUE, keep=True)
    assert len(got) == len(want)
    for g, w, oc in zip(got, want, outcomes):
        assert g.tobytes() == w.tobytes(), (int(w["channel"]), int(w["bitpos"]), oc, g["nerr"], w["nerr"], int(g["flags"]))
    assert (got["flags"] & _lib.FRAME_RESCUED != 0).sum() == outcomes.count("rescued")
    for c in range(sc.C):
        info = b.rescue_info(c)
        st = state.get(c, rr.new_state())
        assert info["layouts"] == _layouts(st), c
        assert (info["tried"], info["rescued"]) == (st["tried"], st["rescued"]), c
    b.close()


def test_flag_off_is_the_oracle_and_knows_nothing_of_the_rescue():
    got, b = _run(_iq(), 0, keep=True)
    assert got.tobytes() == rs.oracle_frames().tobytes()
    with pytest.raises(SondeError):
        b.rescue_info(0)
    b.close()


def test_clean_scene_is_unchanged_by_the_flag():
    off = _run(_iq(clean=True), 0)
    on, b = _run(_iq(clean=True), RESCUE, keep=True)
    assert len(off) > 20 and on.tobytes() == off.tobytes()
    assert off.tobytes() == rs.oracle_frames(clean=True).tobytes()
    info = b.rescue_info(0)
    assert len(info["layouts"][320]) == 6 and (info["tried"], info["rescued"]) == (0, 0)
    b.close()


@pytest.mark.parametrize("variant", ["4_submits", "10_submits", "time_slices_3", "split_fec", "late_join_frames_of", "pipeline_frames_of"])
def test_cut_invariance(variant):
    want, _, state = rr.rescue(rs.oracle_frames())
    kw = {"4_submits": dict(cuts=4), "10_submits": dict(cuts=10), "time_slices_3": dict(time_slices=3),
          "split_fec": dict(flags=RESCUE | _lib.FLAG_SPLIT_FEC, cuts=2),
          "late_join_frames_of": dict(flags=RESCUE | _lib.FLAG_LATE_JOIN, cuts=4, via_ticket=True),
          "pipeline_frames_of": dict(flags=RESCUE | _lib.FLAG_PIPELINE, cuts=4, via_ticket=True)}[variant]
    kw.setdefault("flags", RESCUE)
    got, b = _run(_iq(), keep=True, **kw)
    assert got.tobytes() == want.tobytes()
    for c in range(rs.scene().C):
        info = b.rescue_info(c)
        assert info["layouts"] == _layouts(state[c]) and (info["tried"], info["rescued"]) == (state[c]["tried"], state[c]["rescued"]), c
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LATE_JOIN, _lib.FLAG_SPLIT_FEC], ids=["one_launch", "late_join_units", "split_fec_units"])
def test_mixed_batch_only_rs41_records_change(flags):
    sc = rs.scene()
    types = np.array([0, 1, 3, 0, 3, 0, 1, 0], dtype=np.uint8)
    src = [0, None, None, 3, None, 7, None, 8]              # RS41 rows: channels of the scene (7 and 8 start damaged)
    rows = []
    for c, (t, s) in enumerate(zip(types, src)):
        rows.append(_iq()[s] if s is not None else synth.make_batch(int(t), 1, sc.n, seed=60 + c, ebn0_db=25.0, first_channel=c).iq[0].to(DEV))
    iq = torch.stack(rows).contiguous()
    off = _run(iq, flags, cuts=2, via_ticket=bool(flags & _lib.FLAG_LATE_JOIN), types=types)
    on, b = _run(iq, flags | RESCUE, cuts=2, via_ticket=bool(flags & _lib.FLAG_LATE_JOIN), types=types, keep=True)
    want, outcomes, state = rr.rescue(off)
    assert outcomes.count("rescued") >= 4 and outcomes.count("other") >= 8
    assert on.tobytes() == want.tobytes()
    other = off["type"] != 0
    assert on[other].tobytes() == off[other].tobytes()
    assert b.rescue_info(5)["rescued"] == state[5]["rescued"] >= 1
    with pytest.raises(SondeError):
        b.rescue_info(1)                                    # not an RS41 channel
    b.close()


def test_restart_channels_forget_their_layout():
    iq, restart, cuts = _iq(), [0, 4], 4       # channels whose frames 3, 4 and 5 are all damaged in the scene's plan
    step = iq.shape[1] // cuts

    def feed(flags):
        b = SondeBatch(iq.shape[0], step, flags=flags)
        parts = []
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            if k == 1:
                b.restart_channels(restart)
            parts.append(b.frames().copy())
        return parts, b

    off, b0 = feed(0)
    on, b1 = feed(RESCUE)
    state, firsts = {}, {}
    for k in range(cuts):
        if k == 2:
            for c in restart:
                state.pop(c, None)
        want, outcomes, state = rr.rescue(off[k], state)
        assert on[k].tobytes() == want.tobytes(), k
        if k >= 2:
            for f, oc in zip(off[k], outcomes):
                firsts.setdefault(int(f["channel"]), (oc, int(f["nerr"][0]), int(f["nerr"][1])))
    # the first frame after the restart is damaged (the scene's plan) and stays so; the channel learns again and rescues later
    for c in restart:
        assert firsts[c][0] == "no_layout" and min(firsts[c][1:]) == -1, (c, firsts[c])
    for c in range(iq.shape[0]):
        info = b1.rescue_info(c)
        assert info["layouts"] == _layouts(state[c]) and (info["tried"], info["rescued"]) == (state[c]["tried"], state[c]["rescued"]), c
    whole, _, st_whole = rr.rescue(rs.oracle_frames())
    others = [c for c in range(iq.shape[0]) if c not in restart]
    got = _sorted(on)
    assert got[np.isin(got["channel"], others)].tobytes() == whole[np.isin(whole["channel"], others)].tobytes()
    assert all(state[c] == st_whole[c] for c in others)
    b0.close()
    b1.close()


def test_poll_delivers_the_rescued_measurement_block():
    iq, n, seq = rs.ptu_stream()
    x = torch.from_numpy(iq).to(DEV)
    ptu = {}
    for flags in (0, RESCUE):
        b = SondeBatch(1, n, flags=flags)
        b.submit(x)
        fr = b.frames()
        frags = b.poll()
        ptu[flags] = [(d.temp, d.rh) for _, d in frags if d.fields & _lib.DATA_PTU]
        bad = fr[(fr["nerr"] < 0).any(axis=1)]
        res = fr[fr["flags"] & _lib.FRAME_RESCUED != 0]
        assert (len(bad), len(res)) == ((1, 0) if flags == 0 else (0, 1)), (flags, fr["nerr"])
        if flags:
            assert int(res[0]["data"][59]) | (int(res[0]["data"][60]) << 8) == seq          # the wiped frame's number
        b.close()
    assert len(ptu[RESCUE]) == len(ptu[0]) + 1 >= 2
    T, RH = synth.rs41_true_ptu(np.array([0]), np.array([seq - 1000]))
    extra = [v for v in ptu[RESCUE] if v not in ptu[0]]
    assert len(extra) == 1 and abs(extra[0][0] - float(T[0])) < 0.1 and abs(extra[0][1] - float(RH[0])) < 1.0, (extra, T, RH)


def test_receivers_pass_the_flag_to_their_batch():
    from sdrpp_radiosonde_amd.live import LiveReceiver
    from sdrpp_radiosonde_amd.tuner import WidebandReceiver
    fs = 2_400_000
    for rescue in (True, False):
        for rx in (WidebandReceiver(fs, [(100_000, 0)], chain="iq48", rescue=rescue), LiveReceiver(fs, {0: 2}, probes=2, rescue=rescue)):
            assert bool(rx.batch.flags & RESCUE) == rescue
            if rescue:
                assert rx.batch.rescue_info(0) == {"layouts": {320: [], 518: []}, "tried": 0, "rescued": 0}
            else:
                with pytest.raises(SondeError):
                    rx.batch.rescue_info(0)
