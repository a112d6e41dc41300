"""-m gpu: SONDE_FLAG_AFSK_RESCUE (DESIGN SPEC 3.3i) against its twin (tests/afsk_rescue_reference.py) on the scenes of
tests/afsk_rescue_scenes.py.  With the flag the records are the twin's over the records of a flag-off run, whole records byte for
byte, and they are the twin's over the CPU oracle; afsk_rescue_info reports the twin's counters.  Without the flag the records are the
oracle's and the entry point refuses.  The result does not depend on how the stream is cut into submits, on where the frame decoders
run or on the completion mode; in a mixed batch with all five rescue flags only iMet / C50 records differ from the four-flag run; a
restarted channel counts from zero; poll() delivers a rescued packet's fields."""
import functools

import numpy as np
import pytest
import torch

import afsk_rescue_reference as ar
import afsk_rescue_scenes as sc
from rescue_gpu_harness import check_info, run
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCUE = _lib.FLAG_AFSK_RESCUE
KINDS = ["imet", "c50"]
AFSK_MIN = 16384             # the shortest submit of a batch with iMet or C50 channels
_dev_cache = {}
_run = functools.partial(run, tile=AFSK_MIN)
_check_info = functools.partial(check_info, method="afsk_rescue_info", new_state=ar.new_state)


def _iq(kind, clean=False):
    key = (kind, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(sc.scene_of(kind, clean).iq).to(DEV)
    return _dev_cache[key]


def _types(kind):
    s = sc.scene_of(kind)
    return np.full(s.C, s.type, dtype=np.uint8)


def _oracle_twin(kind):
    return ar.rescue(sc.oracle_run(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_flag_on_records_are_the_twins(kind):
    s = sc.scene(kind)
    off = _run(_iq(kind), 0, types=_types(kind))
    want, outcomes, state = ar.rescue(off)
    assert outcomes.count("rescued") >= 30 and "unsolved" in outcomes and ("ambiguous" in outcomes) == (kind == "c50")
    got, b = _run(_iq(kind), RESCUE, types=_types(kind), keep=True)
    assert len(got) == len(want)
    for g, w, oc in zip(got, want, outcomes):
        assert g.tobytes() == w.tobytes(), (int(w["channel"]), int(w["bitpos"]), oc, g["nerr"], w["nerr"], int(g["flags"]), int(w["flags"]))
    assert got.tobytes() == _oracle_twin(kind)[0].tobytes()
    res = got[got["flags"] & _lib.FRAME_RESCUED != 0]
    assert len(res) == outcomes.count("rescued") and (res["nerr"] == 0).all()
    assert sorted(set(int(v) for v in _lib.frame_flips(res["flags"]))) == [1, 2]
    for f in res:
        tx = sc.tx_of(s, f)[1]
        assert int(f["len"]) == len(tx) and np.array_equal(f["data"][:len(tx)], tx) and not f["data"][len(tx):].any()
    _check_info(b, state, range(s.C))
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_flag_off_is_the_oracle_and_knows_nothing_of_the_rescue(kind):
    got, b = _run(_iq(kind), 0, types=_types(kind), keep=True)
    assert got.tobytes() == sc.oracle_run(kind).tobytes()
    assert not (got["flags"] & _lib.FRAME_RESCUED).any() and (got["nerr"][:, 0] == -1).sum() >= 30
    with pytest.raises(SondeError):
        b.afsk_rescue_info(0)
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_clean_scene_is_unchanged_by_the_flag(kind):
    off = _run(_iq(kind, clean=True), 0, types=_types(kind))
    on, b = _run(_iq(kind, clean=True), RESCUE, types=_types(kind), keep=True)
    assert len(off) >= 70 and (off["nerr"] == 0).all() and on.tobytes() == off.tobytes()
    assert off.tobytes() == sc.oracle_run(kind, True).tobytes()
    _check_info(b, {}, range(sc.scene(kind).C))
    b.close()


@pytest.mark.parametrize("kind,variant", [("imet", "4_submits"), ("c50", "4_submits"), ("imet", "split_fec"), ("c50", "split_fec"),
                                          ("imet", "late_join_frames_of"), ("c50", "pipeline_frames_of"), ("imet", "pipeline_frames_of")])
def test_cut_invariance(kind, variant):
    want, _, state = _oracle_twin(kind)
    kw = {"4_submits": dict(cuts=4), "split_fec": dict(flags=RESCUE | _lib.FLAG_SPLIT_FEC, cuts=2),
          "late_join_frames_of": dict(flags=RESCUE | _lib.FLAG_LATE_JOIN, cuts=4, via_ticket=True),
          "pipeline_frames_of": dict(flags=RESCUE | _lib.FLAG_PIPELINE, cuts=4, via_ticket=True)}[variant]
    kw.setdefault("flags", RESCUE)
    got, b = _run(_iq(kind), keep=True, types=_types(kind), **kw)
    assert got.tobytes() == want.tobytes()
    _check_info(b, state, range(sc.scene(kind).C))
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_cut_invariance_shortest_submits(kind):
    want, _, state = _oracle_twin(kind)
    c = 1
    x = _iq(kind)[c:c + 1].contiguous()
    got, b = _run(x, RESCUE, cuts=x.shape[1] // AFSK_MIN, keep=True, types=_types(kind)[:1])
    w = want[want["channel"] == c].copy()
    w["channel"] = 0
    assert (w["flags"] & _lib.FRAME_RESCUED != 0).sum() >= 8 and got.tobytes() == w.tobytes()
    assert b.afsk_rescue_info(0) == state[c]
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LATE_JOIN, _lib.FLAG_SPLIT_FEC], ids=["default_units", "late_join_units", "split_fec_units"])
def test_mixed_batch_only_afsk_records_change(flags):
    import dfm_rescue_scenes as ds
    import ims_rescue_scenes as ims
    import manchester_rescue_scenes as ms
    import rescue_scenes as rs
    n = sc.TILE * 96
    rs41 = torch.from_numpy(rs.scene().iq).to(DEV)[:, :n]
    m10 = torch.from_numpy(ms.scene("m10").iq).to(DEV)[:, :n]
    dfm = torch.from_numpy(ds.scene().iq).to(DEV)[:, :n]
    im = torch.from_numpy(ims.scene_of("designed").iq).to(DEV)[:, :n]
    assert all(x.shape[1] == n for x in (rs41, m10, dfm, im, _iq("imet"), _iq("c50")))
    rows = [rs41[0], _iq("imet")[0], m10[0], dfm[0], _iq("c50")[0], im[0], _iq("imet")[2], rs41[7], _iq("c50")[1], dfm[3], m10[3], im[3]]
    types = np.array([0, 4, 3, 1, 5, 2, 4, 0, 5, 1, 3, 2], dtype=np.uint8)
    iq = torch.stack(rows).contiguous()
    via = bool(flags & _lib.FLAG_LATE_JOIN)
    four = _lib.FLAG_RS41_RESCUE | _lib.FLAG_MANCHESTER_RESCUE | _lib.FLAG_DFM_RESCUE | _lib.FLAG_IMS_RESCUE
    off = _run(iq, flags | four, types=types)
    want, outcomes, state = ar.rescue(off)
    assert outcomes.count("rescued") >= 40 and outcomes.count("other") >= 40
    for t in (0, 1, 2, 3):
        assert ((off["flags"] & _lib.FRAME_RESCUED != 0) & (off["type"] == t)).sum() >= 2, t
    on, b = _run(iq, flags | four | RESCUE, cuts=2, via_ticket=via, types=types, keep=True)
    assert on.tobytes() == want.tobytes()
    afsk = np.isin(off["type"], [sc.IMET4, sc.C50])
    assert on[~afsk].tobytes() == off[~afsk].tobytes() and on[afsk].tobytes() != off[afsk].tobytes()
    _check_info(b, state, [c for c in range(len(types)) if types[c] in (sc.IMET4, sc.C50)])
    with pytest.raises(SondeError):
        b.afsk_rescue_info(3)                               # a DFM channel
    assert b.manchester_rescue_info(2)["rescued"] >= 1 and b.rescue_info(0)["rescued"] >= 1 and b.dfm_rescue_info(3)["rescued"] >= 1
    assert b.ims_rescue_info(5)["rescued"] >= 1
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_restarted_channels_count_from_zero(kind):
    iq, restart, cuts = _iq(kind), [0, 2], 4
    step = iq.shape[1] // cuts

    def feed(flags):
        b = SondeBatch(iq.shape[0], step, flags=flags, types=_types(kind))
        parts, before = [], None
        state = {}
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            fr = b.frames().copy()
            if flags == 0:
                if k == 2:
                    for c in restart:
                        state.pop(c, None)
                fr, _, state = ar.rescue(fr, state)           # the twin over this submit's records
            elif k == 1:
                before = {c: b.afsk_rescue_info(c) for c in restart}
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
    whole = _oracle_twin(kind)[2]
    for c in range(iq.shape[0]):
        info = b1.afsk_rescue_info(c)
        assert info == state.get(c, ar.new_state()), c
        assert (info != whole[c]) == (c in restart), c
    b1.close()


def test_poll_delivers_the_rescued_packets_fields():
    s = sc.scene("imet")
    c = 0
    _, outcomes, _ = _oracle_twin("imet")
    fr0 = sc.oracle_run("imet")
    # the PTU packets (01 01 <packet number, u16> ...) of channel c: parse.cpp reports the number as SondeData.seq.  Those clean as
    # recorded, and those the pass rescued (what it repaired may be the number itself: taken from the transmitted packet)
    seq = {"clean": [], "rescued": []}
    for f, oc in zip(fr0, outcomes):
        tx = sc.tx_of(s, f)[1]
        if int(f["channel"]) == c and int(tx[1]) == 1 and oc in seq:
            seq[oc].append(int(tx[2]) | (int(tx[3]) << 8))
    assert len(seq["clean"]) >= 2 and len(seq["rescued"]) >= 2
    x = _iq("imet")[c:c + 1].contiguous()
    got = {}
    for flags in (0, RESCUE):
        b = SondeBatch(1, x.shape[1], flags=flags, types=np.array([sc.IMET4], dtype=np.uint8))
        b.submit(x)
        got[flags] = sorted(int(d.seq) for _, d in b.poll() if d.fields & _lib.DATA_PTU)
        b.close()
    assert got[0] == sorted(seq["clean"])
    assert got[RESCUE] == sorted(seq["clean"] + seq["rescued"])


def test_noisy_imet_scene_follows_the_twin_and_every_rescued_packet_was_sent():
    s = sc.noisy_scene("noisy_imet")
    off = _run(_iq("noisy_imet"), 0, types=_types("noisy_imet"))
    want, outcomes, state = ar.rescue(off)
    on, b = _run(_iq("noisy_imet"), RESCUE, types=_types("noisy_imet"), keep=True)
    assert on.tobytes() == want.tobytes() and on.tobytes() == _oracle_twin("noisy_imet")[0].tobytes()
    res = on[on["flags"] & _lib.FRAME_RESCUED != 0]
    print("noisy iMet scene on the GPU: records", len(on), "clean without the flag", int((off["nerr"][:, 0] == 0).sum()), "rescued", len(res))
    assert len(res) >= 150
    for f in res:
        hit = sc.tx_of(s, f)
        assert hit is not None and int(f["len"]) == len(hit[1]) and np.array_equal(f["data"][:len(hit[1])], hit[1]), (int(f["channel"]), int(f["bitpos"]))
    _check_info(b, state, range(s.C))
    b.close()


def test_noisy_c50_scene_follows_the_twin():
    s = sc.noisy_scene("noisy_c50")
    off = _run(_iq("noisy_c50"), 0, types=_types("noisy_c50"))
    want, outcomes, state = ar.rescue(off)
    assert outcomes.count("rescued") >= 20 and "ambiguous" in outcomes and "unsolved" in outcomes
    on, b = _run(_iq("noisy_c50"), RESCUE, types=_types("noisy_c50"), keep=True)
    assert on.tobytes() == want.tobytes() and on.tobytes() == _oracle_twin("noisy_c50")[0].tobytes()
    _check_info(b, state, range(s.C))
    b.close()


def test_the_batch_behind_a_channelizer_has_no_rescue():
    """sonde_chan_create takes no flags, so its embedded batch never has the pass (sd_batch_submit_bins refuses one that had): the
    entry point says so"""
    from sdrpp_radiosonde_amd.batch import SondeChannelizer
    ch = SondeChannelizer()
    with pytest.raises(SondeError):
        ch.batch.afsk_rescue_info(0)
    ch.close()


def test_receivers_pass_the_flag_to_their_batch():
    from sdrpp_radiosonde_amd.live import LiveReceiver
    from sdrpp_radiosonde_amd.tuner import WidebandReceiver
    fs = 2_400_000
    for on in (True, False):
        for rx in (WidebandReceiver(fs, [(100_000, 4), (-200_000, 5)], chain="iq48", afsk_rescue=on, ims_rescue=not on),
                   LiveReceiver(fs, {4: 1, 5: 1}, probes=2, afsk_rescue=on, ims_rescue=not on)):
            assert bool(rx.batch.flags & RESCUE) == on and bool(rx.batch.flags & _lib.FLAG_IMS_RESCUE) == (not on)
            assert rx.batch.n_channels == 2
            for k in range(2):                              # an iMet and a C50 channel, in either order
                if on:
                    assert rx.batch.afsk_rescue_info(k) == {"tried": 0, "rescued": 0}
                else:
                    with pytest.raises(SondeError):
                        rx.batch.afsk_rescue_info(k)
