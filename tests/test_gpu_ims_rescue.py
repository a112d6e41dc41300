"""-m gpu: SONDE_FLAG_IMS_RESCUE (DESIGN SPEC 3.3h) against its twin (tests/ims_rescue_reference.py) on the scenes of
tests/ims_rescue_scenes.py.  The block decoder alone on about 20 000 (block, mask) pairs.  With the flag the records are the twin's
over the records of a flag-off run and the chips sonde_batch_read_bits returns, whole records byte for byte, and ims_rescue_info
reports the twin's counters.  Without the flag the records are the oracle's and the entry point refuses.  The result does not depend
on how the stream is cut into submits, on time slices, on where the frame decoders run, on the completion mode or (given that run's
own chips) on SONDE_FLAG_WIDE; in a mixed batch with all four rescue flags only iMS-100 records differ from the three-flag run; a
restarted channel counts from zero; poll() delivers a rescued frame's fragments and LiveReceiver's validity rule takes it."""
import functools

import numpy as np
import pytest
import torch

import ims_rescue_reference as ir
import ims_rescue_scenes as ims
from rescue_gpu_harness import check_info, gpu_chips as _gpu_chips, run
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCUE = _lib.FLAG_IMS_RESCUE
_dev_cache = {}
_run = functools.partial(run, tile=ims.TILE, default_type=ims.IMS)
_check_info = functools.partial(check_info, method="ims_rescue_info", new_state=ir.new_state)


def _iq(name="designed", clean=False):
    key = (name, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(ims.scene_of(name, clean).iq).to(DEV)
    return _dev_cache[key]


def _oracle_twin(name):
    fr, streams = ims.oracle_run(name)
    return ir.rescue(fr, ir.chips_of_streams(streams))


def test_block_decoder_on_designed_random_and_ambiguous_pairs():
    blocks, viols, first_amb = ims.block_pairs()
    want_blk, want_st = ims.block_pairs_decoded()
    b = SondeBatch(1, ims.TILE)
    got, status = b.test_ims_block(blocks, viols)
    b.close()
    assert len(blocks) >= 19000
    bad = np.flatnonzero((got != want_blk) | (status != want_st))
    assert len(bad) == 0, [(int(i), hex(int(blocks[i])), hex(int(viols[i])), int(status[i]), int(want_st[i])) for i in bad[:5]]
    assert (status >= 0).sum() >= 1000 and (status == -1).sum() >= 1000
    assert (status[first_amb:] == -1).all() and (got[first_amb:] == blocks[first_amb:]).all()
    assert (got[status == -1] == blocks[status == -1]).all()


def test_flag_on_records_are_the_twins():
    sc = ims.scene()
    off, b0 = _run(_iq(), 0, keep=True)
    want, outcomes, state = ir.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 20 and {"unsolved", "clean"} <= set(outcomes) and "mismatch" not in outcomes
    got, b = _run(_iq(), RESCUE, keep=True)
    assert len(got) == len(want)
    for g, w, oc in zip(got, want, outcomes):
        assert g.tobytes() == w.tobytes(), (int(w["channel"]), int(w["bitpos"]), oc, g["nerr"], w["nerr"], int(g["flags"]), int(w["flags"]))
    assert got.tobytes() == _oracle_twin("designed")[0].tobytes()
    res = got[got["flags"] & _lib.FRAME_RESCUED != 0]
    assert len(res) == outcomes.count("rescued") and (res["nerr"][:, 1] == 0).all()
    assert sorted(set(int(v) for v in _lib.frame_blocks(res["flags"]))) == [1, 2]
    for f in res:                                                # rescued records carry the transmitted data bits
        assert np.array_equal(f["data"][:51], ims.tx_of(sc, f)[1])
    for f in got:                                                # and every record what the table of cases says
        case, _ = sc.plan[(int(f["channel"]), ims.tx_of(sc, f)[0])]
        want_oc, blocks, is_tx = ims.EXPECT[case]
        assert (bool(f["flags"] & _lib.FRAME_RESCUED), int(_lib.frame_blocks(f["flags"])), bool(np.array_equal(f["data"][:51], ims.tx_of(sc, f)[1]))) == \
            (want_oc == "rescued", blocks, is_tx), case
    _check_info(b, state, range(sc.C))
    b.close()


def test_flag_off_is_the_oracle_and_knows_nothing_of_the_rescue():
    got, b = _run(_iq(), 0, keep=True)
    assert got.tobytes() == ims.oracle_run("designed")[0].tobytes()
    with pytest.raises(SondeError):
        b.ims_rescue_info(0)
    b.close()


def test_clean_scene_is_unchanged_by_the_flag():
    off = _run(_iq("designed", clean=True), 0)
    on, b = _run(_iq("designed", clean=True), RESCUE, keep=True)
    assert len(off) >= 60 and (off["nerr"] == 0).all() and on.tobytes() == off.tobytes()
    assert off.tobytes() == ims.oracle_run("designed", True)[0].tobytes()
    _check_info(b, {}, range(ims.scene().C))
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
    _check_info(b, state, range(ims.scene().C))
    b.close()


def test_cut_invariance_tile_sized_submits():
    want, _, state = _oracle_twin("designed")
    c = 1
    got, b = _run(_iq()[c:c + 1].contiguous(), RESCUE, cuts=ims.DESIGNED["tiles"], keep=True)
    w = want[want["channel"] == c].copy()
    w["channel"] = 0
    assert (w["flags"] & _lib.FRAME_RESCUED != 0).sum() >= 4 and got.tobytes() == w.tobytes()
    assert b.ims_rescue_info(0) == state[c]
    b.close()


def test_wide_rows_follow_the_twin_on_their_own_chips():
    off, b0 = _run(_iq(), _lib.FLAG_WIDE, keep=True)
    want, outcomes, state = ir.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 20
    on, b = _run(_iq(), _lib.FLAG_WIDE | RESCUE, keep=True)
    assert on.tobytes() == want.tobytes()
    _check_info(b, state, range(ims.scene().C))
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LATE_JOIN, _lib.FLAG_SPLIT_FEC], ids=["one_launch", "late_join_units", "split_fec_units"])
def test_mixed_batch_only_ims_records_change(flags):
    import dfm_rescue_scenes as ds
    import manchester_rescue_scenes as ms
    import rescue_scenes as rs
    n = ims.TILE * 100
    rs41 = torch.from_numpy(rs.scene().iq).to(DEV)
    m10 = torch.from_numpy(ms.scene("m10").iq).to(DEV)
    dfm = torch.from_numpy(ds.scene().iq).to(DEV)
    assert rs41.shape[1] == n and m10.shape[1] == n and dfm.shape[1] == n
    rows = [rs41[0], _iq()[0], m10[0], dfm[0], _iq()[3], rs41[7], _iq()[1], dfm[3], m10[3]]
    types = np.array([0, 2, 3, 1, 2, 0, 2, 1, 3], dtype=np.uint8)
    iq = torch.stack(rows).contiguous()
    via = bool(flags & _lib.FLAG_LATE_JOIN)
    three = _lib.FLAG_RS41_RESCUE | _lib.FLAG_MANCHESTER_RESCUE | _lib.FLAG_DFM_RESCUE
    off, b0 = _run(iq, flags | three, types=types, keep=True)
    want, outcomes, state = ir.rescue(off, _gpu_chips(b0))
    b0.close()
    assert outcomes.count("rescued") >= 12 and outcomes.count("other") >= 20
    for t in (0, 1, 3):
        assert ((off["flags"] & _lib.FRAME_RESCUED != 0) & (off["type"] == t)).sum() >= 2, t
    on, b = _run(iq, flags | three | RESCUE, cuts=2, via_ticket=via, types=types, keep=True)
    assert on.tobytes() == want.tobytes()
    other = off["type"] != ims.IMS
    assert on[other].tobytes() == off[other].tobytes() and on[~other].tobytes() != off[~other].tobytes()
    _check_info(b, state, [c for c in range(len(types)) if types[c] == ims.IMS])
    with pytest.raises(SondeError):
        b.ims_rescue_info(3)                                # a DFM channel
    assert b.manchester_rescue_info(2)["rescued"] >= 1 and b.rescue_info(0)["rescued"] >= 1 and b.dfm_rescue_info(3)["rescued"] >= 1
    b.close()


def test_restarted_channels_count_from_zero():
    iq, restart, cuts = _iq(), [0, 3], 4
    step = iq.shape[1] // cuts
    types = np.full(iq.shape[0], ims.IMS, dtype=np.uint8)

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
                fr, _, state = ir.rescue(fr, _gpu_chips(b), state)
            elif k == 1:
                before = {c: b.ims_rescue_info(c) for c in restart}
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
        info = b1.ims_rescue_info(c)
        assert info == state.get(c, ir.new_state()), c
        assert (info != whole[c]) == (c in restart), c
    b1.close()


def _seqs(records):
    """what parse.cpp's feed_ims100 makes of the frame counters of the records it takes (nerr[1] == 0, word 0 with odd parity), in order"""
    out = []
    for f in records:
        v = int(f["data"][0]) << 9 | int(f["data"][1]) << 1 | int(f["data"][2]) >> 7
        if int(f["nerr"][1]) == 0 and bin(v).count("1") & 1:
            out.append(v >> 1)
    return out


def test_poll_and_the_live_validity_rule_deliver_the_rescued_frames():
    from sdrpp_radiosonde_amd.live import frame_ok
    c = 0
    want, outcomes, _ = _oracle_twin("designed")
    fr0, _ = ims.oracle_run("designed")
    mine = fr0["channel"] == c
    seq_off, seq_on = _seqs(fr0[mine]), _seqs(want[mine])
    assert len(seq_on) >= len(seq_off) + 4
    x = _iq()[c:c + 1].contiguous()
    got, valid = {}, {}
    for flags in (0, RESCUE):
        b = SondeBatch(1, x.shape[1], flags=flags, types=np.array([ims.IMS], dtype=np.uint8))
        b.submit(x)
        fr = b.frames().copy()
        got[flags] = [int(d.seq) for _, d in b.poll() if d.fields & _lib.DATA_SEQ]
        valid[flags] = fr[frame_ok(fr)]            # what LiveReceiver.frames() keeps
        b.close()
    assert got[0] == seq_off and got[RESCUE] == seq_on
    assert (valid[0]["flags"] & _lib.FRAME_RESCUED == 0).all() and (valid[RESCUE]["flags"] & _lib.FRAME_RESCUED != 0).sum() == len(valid[RESCUE]) - len(valid[0]) >= 4


def test_noisy_scene_follows_the_twin_and_gives_the_recorded_counts():
    sc = ims.scene_of("noisy")
    off, b0 = _run(_iq("noisy"), 0, keep=True)
    want, outcomes, state = ir.rescue(off, _gpu_chips(b0))
    b0.close()
    on, b = _run(_iq("noisy"), RESCUE, keep=True)
    assert on.tobytes() == want.tobytes()
    res = on[on["flags"] & _lib.FRAME_RESCUED != 0]
    equal = sum(ims.tx_of(sc, f) is not None and np.array_equal(f["data"][:51], ims.tx_of(sc, f)[1]) for f in res)
    same = on.tobytes() == _oracle_twin("noisy")[0].tobytes()
    print("noisy on the GPU: records", len(on), "failed without the flag", int((off["nerr"][:, 1] != 0).sum()), "rescued", len(res),
          "equal to the transmitted frame", equal, "equal to the reference's twin", same)
    assert off.tobytes() == ims.oracle_run("noisy")[0].tobytes() and same
    assert dict(records=len(on), failed=int((off["nerr"][:, 1] != 0).sum()), by_blocks=np.bincount(off["nerr"][:, 1][off["nerr"][:, 1] != 0]).tolist(),
                rescued=len(res), rescued_equal_tx=equal) == ims.NOISY_COUNTS
    _check_info(b, state, range(sc.C))
    b.close()


def test_the_batch_behind_a_channelizer_has_no_rescue():
    """sonde_chan_create takes no flags, so its embedded batch never has the pass (sd_batch_submit_bins refuses one that had): the
    entry point says so"""
    from sdrpp_radiosonde_amd.batch import SondeChannelizer
    ch = SondeChannelizer()
    with pytest.raises(SondeError):
        ch.batch.ims_rescue_info(0)
    ch.close()


def test_receivers_pass_the_flag_to_their_batch():
    from sdrpp_radiosonde_amd.live import LiveReceiver
    from sdrpp_radiosonde_amd.tuner import WidebandReceiver
    fs = 2_400_000
    for on in (True, False):
        for rx in (WidebandReceiver(fs, [(100_000, 2)], chain="iq48", ims_rescue=on, dfm_rescue=not on),
                   LiveReceiver(fs, {2: 2}, probes=2, ims_rescue=on, dfm_rescue=not on)):
            assert bool(rx.batch.flags & RESCUE) == on and bool(rx.batch.flags & _lib.FLAG_DFM_RESCUE) == (not on)
            if on:
                assert rx.batch.ims_rescue_info(0) == {"tried": 0, "rescued": 0}
            else:
                with pytest.raises(SondeError):
                    rx.batch.ims_rescue_info(0)
