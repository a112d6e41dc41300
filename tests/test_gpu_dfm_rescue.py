"""-m gpu: SONDE_FLAG_DFM_RESCUE (DESIGN SPEC 3.3g) against its twin (tests/dfm_rescue_reference.py) on the scenes of
tests/dfm_rescue_scenes.py.  The word decoder alone on all 65 536 (word, mask) pairs.  With the flag the records are the twin's over
the records of a flag-off run and the chips sonde_batch_read_bits returns, whole records byte for byte, and dfm_rescue_info reports
the twin's counters.  Without the flag the records are the oracle's and the entry point refuses.  The result does not depend on how
the stream is cut into submits, on time slices, on where the frame decoders run, on the completion mode or (given that run's own
chips) on SONDE_FLAG_WIDE; in a mixed batch only DFM records change, and the other two passes work beside it; a restarted channel
counts from zero; poll() delivers a rescued frame's fragments."""
import functools

import numpy as np
import pytest
import torch

import dfm_rescue_reference as dr
import dfm_rescue_scenes as ds
from rescue_gpu_harness import check_info, gpu_chips as _gpu_chips, run
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCUE = _lib.FLAG_DFM_RESCUE
_dev_cache = {}
_run = functools.partial(run, tile=ds.TILE, default_type=ds.DFM)
_check_info = functools.partial(check_info, method="dfm_rescue_info", new_state=dr.new_state)


def _iq(name="designed", clean=False):
    key = (name, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(ds.scene_of(name, clean).iq).to(DEV)
    return _dev_cache[key]


def _oracle_twin(name):
    fr, streams = ds.oracle_run(name)
    return dr.rescue(fr, dr.chips_of_streams(streams))


def test_word_decoder_on_every_word_and_mask():
    words = np.repeat(np.arange(256, dtype=np.uint8), 256)
    masks = np.tile(np.arange(256, dtype=np.uint8), 256)
    b = SondeBatch(1, ds.TILE)
    got, status = b.test_hamming84_erasures(words, masks)
    b.close()
    for w, E, g, st in zip(words.tolist(), masks.tolist(), got.tolist(), status.tolist()):
        want = dr.decode_word(w, E)
        if want is None:
            assert st == -1 and g == w, (w, E, g, st)
        else:
            assert g == want and st == bin(w ^ want).count("1"), (w, E, g, st)
    assert (status >= 0).sum() > 1000 and (status == -1).sum() > 1000


@pytest.mark.parametrize("name", ["designed", "long"])
def test_flag_on_records_are_the_twins(name):
    sc = ds.scene(name)
    off, b0 = _run(_iq(name), 0, keep=True)
    want, outcomes, state = dr.rescue(off, _gpu_chips(b0))
    b0.close()
    if name == "designed":
        assert outcomes.count("rescued") >= 16 and {"too_many", "unsolved", "clean"} <= set(outcomes)
    else:
        assert len(off) > 70 and outcomes[60:71] == ["rescued", "unsolved"] * 5 + ["rescued"]
    got, b = _run(_iq(name), RESCUE, keep=True)
    assert len(got) == len(want)
    for g, w, oc in zip(got, want, outcomes):
        assert g.tobytes() == w.tobytes(), (int(w["channel"]), int(w["bitpos"]), oc, g["nerr"], w["nerr"], int(g["flags"]), int(w["flags"]))
    assert got.tobytes() == _oracle_twin(name)[0].tobytes()
    res = got[got["flags"] & _lib.FRAME_RESCUED != 0]
    assert len(res) == outcomes.count("rescued") and (res["nerr"][:, 1] == 0).all()
    assert sorted(set(int(v) for v in _lib.frame_words(res["flags"]))) == ([1, 2] if name == "designed" else [1])
    for f in res:
        assert np.array_equal(f["data"][:33], ds.tx_of(sc, f)[1])
    if name == "designed":
        assert set(int(f["flags"]) & 1 for f in res) == {0, 1}              # the channel with inverted polarity is rescued like the others
    _check_info(b, state, range(sc.C))
    b.close()


def test_flag_off_is_the_oracle_and_knows_nothing_of_the_rescue():
    got, b = _run(_iq(), 0, keep=True)
    assert got.tobytes() == ds.oracle_run("designed")[0].tobytes()
    with pytest.raises(SondeError):
        b.dfm_rescue_info(0)
    b.close()


def test_clean_scene_is_unchanged_by_the_flag():
    off = _run(_iq("designed", clean=True), 0)
    on, b = _run(_iq("designed", clean=True), RESCUE, keep=True)
    assert len(off) >= 100 and (off["nerr"] == 0).all() and on.tobytes() == off.tobytes()
    assert off.tobytes() == ds.oracle_run("designed", True)[0].tobytes()
    _check_info(b, {}, range(ds.scene().C))
    b.close()


@pytest.mark.parametrize("variant", ["4_submits", "time_slices_3", "split_fec", "late_join_frames_of", "pipeline_frames_of"])
def test_cut_invariance(variant):
    want, _, state = _oracle_twin("designed")
    kw = {"4_submits": dict(cuts=4), "time_slices_3": dict(time_slices=3),
          "split_fec": dict(flags=RESCUE | _lib.FLAG_SPLIT_FEC, cuts=2),
          "late_join_frames_of": dict(flags=RESCUE | _lib.FLAG_LATE_JOIN, cuts=4, via_ticket=True),
          "pipeline_frames_of": dict(flags=RESCUE | _lib.FLAG_PIPELINE, cuts=4, via_ticket=True)}[variant]
    kw.setdefault("flags", RESCUE)
    got, b = _run(_iq(), keep=True, **kw)
    assert got.tobytes() == want.tobytes()
    _check_info(b, state, range(ds.scene().C))
    b.close()


def test_cut_invariance_tile_sized_submits():
    want, _, state = _oracle_twin("designed")
    c = 3                                                   # the channel with inverted polarity
    got, b = _run(_iq()[c:c + 1].contiguous(), RESCUE, cuts=ds.DESIGNED["tiles"], keep=True)
    w = want[want["channel"] == c].copy()
    w["channel"] = 0
    assert (w["flags"] & _lib.FRAME_RESCUED != 0).sum() >= 4 and got.tobytes() == w.tobytes()
    assert b.dfm_rescue_info(0) == state[c]
    b.close()


def test_wide_rows_follow_the_twin_on_their_own_chips():
    off, b0 = _run(_iq(), _lib.FLAG_WIDE, keep=True)
    want, outcomes, state = dr.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 16
    on, b = _run(_iq(), _lib.FLAG_WIDE | RESCUE, keep=True)
    assert on.tobytes() == want.tobytes()
    _check_info(b, state, range(ds.scene().C))
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LATE_JOIN, _lib.FLAG_SPLIT_FEC], ids=["one_launch", "late_join_units", "split_fec_units"])
def test_mixed_batch_only_dfm_records_change(flags):
    import manchester_rescue_scenes as ms
    import rescue_scenes as rs
    n = ds.TILE * 100
    rs41 = torch.from_numpy(rs.scene().iq).to(DEV)
    m10 = torch.from_numpy(ms.scene("m10").iq).to(DEV)
    assert rs41.shape[1] == n and m10.shape[1] == n
    rows = [rs41[0], _iq()[0], m10[0], _iq()[3], rs41[7], m10[3], _iq()[1]]
    types = np.array([0, 1, 3, 1, 0, 3, 1], dtype=np.uint8)
    iq = torch.stack(rows).contiguous()
    via = bool(flags & _lib.FLAG_LATE_JOIN)
    both = _lib.FLAG_RS41_RESCUE | _lib.FLAG_MANCHESTER_RESCUE
    off, b0 = _run(iq, flags | both, types=types, keep=True)
    want, outcomes, state = dr.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 12 and outcomes.count("other") >= 20
    assert ((off["flags"] & _lib.FRAME_RESCUED != 0) & (off["type"] == 0)).sum() >= 2 and ((off["flags"] & _lib.FRAME_RESCUED != 0) & (off["type"] == 3)).sum() >= 2
    on, b = _run(iq, flags | both | RESCUE, cuts=2, via_ticket=via, types=types, keep=True)
    assert on.tobytes() == want.tobytes()
    other = off["type"] != ds.DFM
    assert on[other].tobytes() == off[other].tobytes() and on[~other].tobytes() != off[~other].tobytes()
    _check_info(b, state, [c for c in range(len(types)) if types[c] == ds.DFM])
    with pytest.raises(SondeError):
        b.dfm_rescue_info(2)                                # an M10 channel
    assert b.manchester_rescue_info(2)["rescued"] >= 1 and b.rescue_info(0)["rescued"] >= 1
    b.close()


def test_restarted_channels_count_from_zero():
    iq, restart, cuts = _iq(), [0, 3], 4
    step = iq.shape[1] // cuts
    types = np.full(iq.shape[0], ds.DFM, dtype=np.uint8)

    def feed(flags):
        b = SondeBatch(iq.shape[0], step, flags=flags, types=types)
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
                fr, _, state = dr.rescue(fr, _gpu_chips(b), state)
            elif k == 1:
                before = {c: b.dfm_rescue_info(c) for c in restart}
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
    whole = _oracle_twin("designed")[2]
    for c in range(iq.shape[0]):
        info = b1.dfm_rescue_info(c)
        assert info == state.get(c, dr.new_state()), c
        assert (info != whole[c]) == (c in restart), c
    b1.close()


def _seqs(records):
    """what parse.cpp's feed_dfm makes of the frame counters (sub-packet id 0) of the records it takes (nerr[1] == 0), in order"""
    out = []
    for f in records:
        if int(f["nerr"][1]) != 0:
            continue
        for blk in range(2):
            cw = f["data"][7 + 13 * blk:7 + 13 * blk + 13]
            if cw[12] >> 4 == 0:
                out.append(int((cw[6] >> 4) << 4 | (cw[7] >> 4)))
    return out


def test_poll_delivers_the_rescued_frames_fragments():
    c = 0
    want, outcomes, _ = _oracle_twin("designed")
    fr0, _ = ds.oracle_run("designed")
    mine = fr0["channel"] == c
    seq_off, seq_on = _seqs(fr0[mine]), _seqs(want[mine])
    assert len(seq_on) >= len(seq_off) + 2
    x = _iq()[c:c + 1].contiguous()
    got = {}
    for flags in (0, RESCUE):
        b = SondeBatch(1, x.shape[1], flags=flags, types=np.array([ds.DFM], dtype=np.uint8))
        b.submit(x)
        got[flags] = [int(d.seq) for _, d in b.poll() if d.fields & _lib.DATA_SEQ]
        b.close()
    assert got[0] == seq_off and got[RESCUE] == seq_on


@pytest.mark.parametrize("name", ["noisy", "noisy_negq"])
def test_noisy_scene_follows_the_twin_and_every_rescued_frame_was_sent(name):
    sc = ds.scene_of(name)
    off, b0 = _run(_iq(name), 0, keep=True)
    want, outcomes, state = dr.rescue(off, _gpu_chips(b0))
    b0.close()
    on, b = _run(_iq(name), RESCUE, keep=True)
    assert on.tobytes() == want.tobytes()
    res = on[on["flags"] & _lib.FRAME_RESCUED != 0]
    print(name, "on the GPU: records", len(on), "valid without the flag", int((off["nerr"][:, 1] == 0).sum()), "failed", int((off["nerr"][:, 1] != 0).sum()),
          "rescued", len(res), "equal to the reference's twin", on.tobytes() == _oracle_twin(name)[0].tobytes())
    assert len(res) >= 20
    for f in res:
        hit = ds.tx_of(sc, f)
        assert hit is not None and np.array_equal(f["data"][:33], hit[1]), (int(f["channel"]), int(f["bitpos"]))
    _check_info(b, state, range(sc.C))
    b.close()


def test_the_batch_behind_a_channelizer_has_no_rescue():
    """sonde_chan_create takes no flags, so its embedded batch never has the pass (sd_batch_submit_bins refuses one that had): the
    entry point says so"""
    from sdrpp_radiosonde_amd.batch import SondeChannelizer
    ch = SondeChannelizer()
    with pytest.raises(SondeError):
        ch.batch.dfm_rescue_info(0)
    ch.close()


def test_receivers_pass_the_flag_to_their_batch():
    from sdrpp_radiosonde_amd.live import LiveReceiver
    from sdrpp_radiosonde_amd.tuner import WidebandReceiver
    fs = 2_400_000
    for on in (True, False):
        for rx in (WidebandReceiver(fs, [(100_000, 1)], chain="iq48", dfm_rescue=on, manchester_rescue=not on),
                   LiveReceiver(fs, {1: 2}, probes=2, dfm_rescue=on, manchester_rescue=not on)):
            assert bool(rx.batch.flags & RESCUE) == on and bool(rx.batch.flags & _lib.FLAG_MANCHESTER_RESCUE) == (not on)
            if on:
                assert rx.batch.dfm_rescue_info(0) == {"tried": 0, "rescued": 0}
            else:
                with pytest.raises(SondeError):
                    rx.batch.dfm_rescue_info(0)
