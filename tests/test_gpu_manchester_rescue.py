"""-m gpu: SONDE_FLAG_MANCHESTER_RESCUE (DESIGN SPEC 3.3f) against its twin (tests/manchester_rescue_reference.py) on the scenes of
tests/manchester_rescue_scenes.py.  With the flag the records are the twin's over the records of a flag-off run and the chips
sonde_batch_read_bits returns, whole records byte for byte, and they are the twin's over the CPU oracle; manchester_rescue_info reports
the twin's counters.  Without the flag the records are the oracle's and the entry point refuses.  The result does not depend on how
the stream is cut into submits, on time slices, on where the frame decoders run or on the completion mode; in a mixed batch only
M10 / M20 / MRZ-N1 records change, and the RS41 pass works beside it; a restarted channel counts from zero; poll() delivers a rescued
frame's fragments."""
import functools

import numpy as np
import pytest
import torch

import manchester_rescue_reference as mr
import manchester_rescue_scenes as ms
from rescue_gpu_harness import check_info, gpu_chips as _gpu_chips, run
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCUE = _lib.FLAG_MANCHESTER_RESCUE
KINDS = ["m10", "m20", "mrz"]
_dev_cache = {}
_run = functools.partial(run, tile=ms.TILE)
_check_info = functools.partial(check_info, method="manchester_rescue_info", new_state=mr.new_state)


def _iq(kind, clean=False):
    key = (kind, clean)
    if key not in _dev_cache:
        sc = ms.noisy_scene() if kind == "noisy" else ms.scene(kind, clean)
        _dev_cache[key] = torch.from_numpy(sc.iq).to(DEV)
    return _dev_cache[key]


def _oracle_twin(kind):
    fr, streams = ms.oracle_run(kind)
    return mr.rescue(fr, mr.chips_of_streams(streams))


def _types(kind):
    return np.full(ms.scene(kind).C if kind != "noisy" else ms.noisy_scene().C, ms.KINDS[kind][0] if kind != "noisy" else ms.M10, dtype=np.uint8)


@pytest.mark.parametrize("kind", KINDS)
def test_flag_on_records_are_the_twins(kind):
    sc = ms.scene(kind)
    off, b0 = _run(_iq(kind), 0, types=_types(kind), keep=True)
    want, outcomes, state = mr.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 6 and {"too_many", "unsolved", "ambiguous"} <= set(outcomes)
    got, b = _run(_iq(kind), RESCUE, types=_types(kind), keep=True)
    assert len(got) == len(want)
    for g, w, oc in zip(got, want, outcomes):
        assert g.tobytes() == w.tobytes(), (int(w["channel"]), int(w["bitpos"]), oc, g["nerr"], w["nerr"], int(g["flags"]), int(w["flags"]))
    assert got.tobytes() == _oracle_twin(kind)[0].tobytes()
    res = got[got["flags"] & _lib.FRAME_RESCUED != 0]
    assert len(res) == outcomes.count("rescued") and (res["nerr"][:, 0] == 0).all()
    assert sorted(set(int(v) for v in _lib.frame_flips(res["flags"]))) == [1, 4]
    for f in res:
        assert np.array_equal(f["data"][:sc.len], ms.tx_of(sc, f)[1][:sc.len])
    _check_info(b, state, range(sc.C))
    b.close()


def test_flag_off_is_the_oracle_and_knows_nothing_of_the_rescue():
    got, b = _run(_iq("m10"), 0, types=_types("m10"), keep=True)
    assert got.tobytes() == ms.oracle_run("m10")[0].tobytes()
    with pytest.raises(SondeError):
        b.manchester_rescue_info(0)
    b.close()


@pytest.mark.parametrize("kind", ["m10", "mrz"])
def test_clean_scene_is_unchanged_by_the_flag(kind):
    off = _run(_iq(kind, clean=True), 0, types=_types(kind))
    on, b = _run(_iq(kind, clean=True), RESCUE, types=_types(kind), keep=True)
    assert len(off) >= 15 and (off["nerr"] == 0).all() and on.tobytes() == off.tobytes()
    assert off.tobytes() == ms.oracle_run(kind, True)[0].tobytes()
    _check_info(b, {}, range(ms.scene(kind).C))
    b.close()


@pytest.mark.parametrize("variant", ["4_submits", "time_slices_3", "split_fec", "late_join_frames_of", "pipeline_frames_of"])
def test_cut_invariance(variant):
    want, _, state = _oracle_twin("m10")
    kw = {"4_submits": dict(cuts=4), "time_slices_3": dict(time_slices=3),
          "split_fec": dict(flags=RESCUE | _lib.FLAG_SPLIT_FEC, cuts=2),
          "late_join_frames_of": dict(flags=RESCUE | _lib.FLAG_LATE_JOIN, cuts=4, via_ticket=True),
          "pipeline_frames_of": dict(flags=RESCUE | _lib.FLAG_PIPELINE, cuts=4, via_ticket=True)}[variant]
    kw.setdefault("flags", RESCUE)
    got, b = _run(_iq("m10"), keep=True, types=_types("m10"), **kw)
    assert got.tobytes() == want.tobytes()
    _check_info(b, state, range(ms.scene("m10").C))
    b.close()


def test_cut_invariance_tile_sized_submits():
    want, _, state = _oracle_twin("m10")
    c = 1
    got, b = _run(_iq("m10")[c:c + 1].contiguous(), RESCUE, cuts=ms.KINDS["m10"][3], keep=True, types=np.array([ms.M10], dtype=np.uint8))
    w = want[want["channel"] == c].copy()
    w["channel"] = 0
    assert (w["flags"] & _lib.FRAME_RESCUED != 0).sum() >= 2 and got.tobytes() == w.tobytes()
    assert b.manchester_rescue_info(0) == state[c]
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LATE_JOIN, _lib.FLAG_SPLIT_FEC], ids=["one_launch", "late_join_units", "split_fec_units"])
def test_mixed_batch_only_manchester_records_change(flags):
    import rescue_reference as rr
    import rescue_scenes as rs
    n = ms.TILE * 100
    rs41 = torch.from_numpy(rs.scene().iq).to(DEV)
    assert rs41.shape[1] == n
    dfm = synth.make_batch(1, 1, n, seed=61, ebn0_db=25.0, first_channel=1).iq.to(DEV)
    rows = [rs41[0], dfm[0], _iq("m10")[0], _iq("m20")[0], _iq("mrz")[0, :n], rs41[7], _iq("m10")[3], _iq("mrz")[1, :n], _iq("m20")[1]]
    types = np.array([0, 1, 3, 3, 6, 0, 3, 6, 3], dtype=np.uint8)
    iq = torch.stack(rows).contiguous()
    via = bool(flags & _lib.FLAG_LATE_JOIN)
    off, b0 = _run(iq, flags, types=types, keep=True)
    want, outcomes, state = mr.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 8 and outcomes.count("other") >= 20
    for extra in (0, _lib.FLAG_RS41_RESCUE):
        on, b = _run(iq, flags | RESCUE | extra, cuts=2, via_ticket=via, types=types, keep=True)
        w = rr.rescue(want)[0] if extra else want
        assert on.tobytes() == w.tobytes()
        other = ~np.isin(off["type"], [ms.M10, ms.MRZN1])
        if not extra:
            assert on[other].tobytes() == off[other].tobytes()
        else:
            assert ((on["flags"] & _lib.FRAME_RESCUED != 0) & (on["type"] == 0)).sum() >= 2
        _check_info(b, state, [c for c in range(len(types)) if types[c] in (ms.M10, ms.MRZN1)])
        with pytest.raises(SondeError):
            b.manchester_rescue_info(1)                     # a DFM channel
        b.close()


def test_wide_auto_rows_follow_the_twin_on_their_own_chips():
    n = ms.TILE * 100
    iq = torch.stack([_iq("m10")[0], _iq("mrz")[0, :n], _iq("m10")[2], _iq("m20")[0]]).contiguous()
    types = np.array([3, 6, 3, 3], dtype=np.uint8)
    off, b0 = _run(iq, _lib.FLAG_WIDE_AUTO, types=types, keep=True)
    want, outcomes, state = mr.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 4
    on, b = _run(iq, _lib.FLAG_WIDE_AUTO | RESCUE, types=types, keep=True)
    assert on.tobytes() == want.tobytes()
    _check_info(b, state, range(4))
    b.close()


def test_restarted_channels_count_from_zero():
    iq, restart, cuts = _iq("m10"), [0, 2], 4
    step = iq.shape[1] // cuts

    def feed(flags):
        b = SondeBatch(iq.shape[0], step, flags=flags, types=_types("m10"))
        parts, before = [], None
        state = {}
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            fr = b.frames().copy()
            if flags == 0:
                # the twin over this submit's records and the chips still in the ring
                if k == 2:
                    for c in restart:
                        state.pop(c, None)
                fr, _, state = mr.rescue(fr, _gpu_chips(b), state)
            elif k == 1:
                before = {c: b.manchester_rescue_info(c) for c in restart}
            if k == 1:
                b.restart_channels(restart)
            parts.append(fr)
        return parts, b, state, before

    want, b0, state, _ = feed(0)
    on, b1, _, before = feed(RESCUE)
    b0.close()
    for k in range(cuts):
        assert on[k].tobytes() == want[k].tobytes(), k
    assert all(before[c]["tried"] >= 1 for c in restart)
    whole = _oracle_twin("m10")[2]
    for c in range(iq.shape[0]):
        info = b1.manchester_rescue_info(c)
        assert info == state.get(c, mr.new_state()), c
        assert (info != whole[c]) == (c in restart), c
    b1.close()


def test_poll_delivers_the_rescued_frames_fragments():
    sc = ms.scene("m10")
    c = 0
    want, outcomes, _ = _oracle_twin("m10")
    fr0, _ = ms.oracle_run("m10")
    # the frame numbers (index in the channel's stream) of the rescued frames of channel c, and of those clean as recorded
    num = {pos: k for k, (pos, _) in enumerate(sc.frames[c])}
    rescued = sorted(num[ms.tx_of(sc, f)[0]] for f, oc in zip(fr0, outcomes) if int(f["channel"]) == c and oc == "rescued")
    clean = sorted(num[ms.tx_of(sc, f)[0]] for f, oc in zip(fr0, outcomes) if int(f["channel"]) == c and oc == "clean")
    assert len(rescued) >= 2 and len(clean) >= 2
    t_of = lambda k: 315964800 + 2200 * 604800 + (k * 1000 + 123456000) // 1000 - 18      # noqa: E731  (parse.cpp feed_m10 on synth.m10_build_frames)
    x = _iq("m10")[c:c + 1].contiguous()
    times = {}
    for flags in (0, RESCUE):
        b = SondeBatch(1, x.shape[1], flags=flags, types=np.array([ms.M10], dtype=np.uint8))
        b.submit(x)
        times[flags] = sorted(int(d.time) for _, d in b.poll() if d.fields & _lib.DATA_TIME)
        b.close()
    assert times[0] == [t_of(k) for k in clean]
    assert times[RESCUE] == [t_of(k) for k in sorted(clean + rescued)]


def test_noisy_scene_follows_the_twin_and_every_rescued_frame_was_sent():
    sc = ms.noisy_scene()
    types = np.full(sc.C, ms.M10, dtype=np.uint8)
    off, b0 = _run(_iq("noisy"), 0, types=types, keep=True)
    want, outcomes, state = mr.rescue(off, _gpu_chips(b0))
    b0.close()
    on, b = _run(_iq("noisy"), RESCUE, types=types, keep=True)
    assert on.tobytes() == want.tobytes() and on.tobytes() == _oracle_twin("noisy")[0].tobytes()
    res = on[on["flags"] & _lib.FRAME_RESCUED != 0]
    print("noisy scene on the GPU: records", len(on), "clean without the flag", int((off["nerr"][:, 0] == 0).sum()), "rescued", len(res))
    assert len(res) >= 30
    for f in res:
        hit = ms.tx_of(sc, f)
        assert hit is not None and np.array_equal(f["data"][:101], hit[1]), (int(f["channel"]), int(f["bitpos"]))
    _check_info(b, state, range(sc.C))
    b.close()


def test_the_batch_behind_a_channelizer_has_no_rescue():
    """sonde_chan_create takes no flags, so its embedded batch never has the pass (sd_batch_submit_bins refuses one that had): the
    entry point says so"""
    from sdrpp_radiosonde_amd.batch import SondeChannelizer
    ch = SondeChannelizer()
    with pytest.raises(SondeError):
        ch.batch.manchester_rescue_info(0)
    ch.close()


def test_receivers_pass_the_flag_to_their_batch():
    from sdrpp_radiosonde_amd.live import LiveReceiver
    from sdrpp_radiosonde_amd.tuner import WidebandReceiver
    fs = 2_400_000
    for on in (True, False):
        for rx in (WidebandReceiver(fs, [(100_000, 3)], chain="iq48", manchester_rescue=on, rescue=not on),
                   LiveReceiver(fs, {3: 2}, probes=2, manchester_rescue=on, rescue=not on)):
            assert bool(rx.batch.flags & RESCUE) == on and bool(rx.batch.flags & _lib.FLAG_RS41_RESCUE) == (not on)
            if on:
                assert rx.batch.manchester_rescue_info(0) == {"tried": 0, "rescued": 0}
            else:
                with pytest.raises(SondeError):
                    rx.batch.manchester_rescue_info(0)
