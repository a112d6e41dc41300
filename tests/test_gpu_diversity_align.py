"""-m gpu: sonde_batch_set_diversity_auto (DESIGN SPEC 3.3k) against its twin (tests/diversity_align_reference.py) on the scenes of
tests/diversity_align_scenes.py.  No offset is given: with learn and mark_duplicates the records of every submit are the twin's over
the same batch's records without groups, whole records byte for byte, however the stream is cut and with time slices, and
diversity_offsets / diversity_info report the twin's state; mode 0 is set_diversity; the align step alone equals the twin on
caller-made cases; the groups that cannot lock stay as they are; the copies 5000 bits apart are combined into the transmitted frame;
a restarted group unlocks and locks again; the refusals hold; poll() leaves out the duplicates; DiversityReceiver takes two antennas'
wideband streams, one five granules late and each with fades of its own, to every transmitted frame exactly once."""
import collections

import numpy as np
import pytest
import torch

import diversity_align_reference as dar
import diversity_align_scenes as das
import diversity_scenes as ds
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DUP = _lib.FRAME_DUPLICATE
_dev_cache, _base_cache = {}, {}
VARIANTS = {"1_submit": (1, {}), "4_submits": (4, {}), "10_submits": (10, {}), "time_slices_3": (2, dict(time_slices=3))}


def _iq(extended=False):
    if extended not in _dev_cache:
        _dev_cache[extended] = torch.from_numpy(das.scene(extended).iq).to(DEV)
    return _dev_cache[extended]


def _sorted(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


def _run(iq, cuts=1, groups=None, keep=False, restart_at=None, learn=True, mark=True, offsets=None, probe=None, **kw):
    """the records of each submit, [(channel, bitpos)-sorted arrays]; probe(b, k) is called behind submit k's restart"""
    n = iq.shape[1]
    assert (n // das.TILE) % cuts == 0
    step = n // cuts
    b = SondeBatch(iq.shape[0], step, **kw)
    if groups is not None:
        b.set_diversity(groups, offsets, das.WINDOW, learn=learn, mark_duplicates=mark)
    parts = []
    for k in range(cuts):
        if restart_at is not None and k == restart_at[0]:
            b.restart_channels(restart_at[1])
            if probe:
                probe(b, k)
        b.submit(iq[:, k * step:(k + 1) * step])
        parts.append(_sorted(b.frames()))
    if keep:
        return parts, b
    b.close()
    return parts


def _base(extended, cuts, **kw):
    key = (extended, cuts, tuple(sorted(kw.items())))
    if key not in _base_cache:
        _base_cache[key] = _run(_iq(extended), cuts, **kw)
    return _base_cache[key]


def _twin(parts, groups, mode=3, restart_at=None, offsets=None):
    st, want = dar.new_state(groups, offsets, mode), []
    for k, sub in enumerate(parts):
        if restart_at is not None and k == restart_at[0]:
            for g, members in enumerate(groups):
                if set(members) <= set(restart_at[1]):
                    dar.restart_group(st, groups, g)
        w, _, st = dar.run(sub, groups, st, mode, das.WINDOW)
        want.append(w)
    return want, st


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        for a, e in zip(g, w):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))


def _same_state(b, st, groups):
    for g, members in enumerate(groups):
        got = b.diversity_offsets(g)
        assert got["offsets"][:len(members)] == [st["off"][ch] for ch in members], (g, got)
        assert got["locked"] == sum(int(st["locked"][ch]) << m for m, ch in enumerate(members)), (g, got)
        assert (got["learned"], got["duplicates"]) == (st["learned"][g], st["duplicates"][g]), (g, got)
        assert b.diversity_info(g) == {"tried": st["div"]["tried"][g], "combined": st["div"]["combined"][g]}, g


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
def test_learning_and_marking_the_records_are_the_twins(extended, variant):
    sc = das.scene(extended)
    cuts, kw = VARIANTS[variant]
    off = _base(extended, cuts, **kw)
    want, st = _twin(off, sc.groups)
    got, b = _run(_iq(extended), cuts, sc.groups, keep=True, **kw)
    _same(got, want)
    _same_state(b, st, sc.groups)
    b.close()
    assert all(st["locked"][ch] for ch in range(7)) and not any(st["locked"][ch] for ch in range(7, 11))
    assert sum(st["duplicates"]) >= 6 and sum(st["div"]["combined"]) >= 3
    # the two sondes and the never-good-together group: the records of a run without groups
    for g, o in zip(got, off):
        keep = np.isin(o["channel"], [7, 8, 9, 10, 11])
        assert g[keep].tobytes() == o[keep].tobytes()


def test_one_submit_is_the_oracles_and_the_copies_5000_bits_apart_are_combined():
    """on the parent nothing says where channel 4 stands, and 5000 bits are beyond any window_bits it takes"""
    sc = das.scene()
    off = _base(False, 1)
    assert off[0].tobytes() == das.oracle_frames().tobytes()
    got, b = _run(_iq(), 1, sc.groups, keep=True)
    assert abs(b.diversity_offsets(1)["offsets"][2] - 5000) < 64 and b.diversity_offsets(1)["locked"] == 7
    b.close()
    comb = [f for f in got[0] if int(f["flags"]) & _lib.FRAME_COMBINED and int(f["channel"]) in (2, 3, 4)]
    assert len(comb) >= 1 and any(_lib.frame_copies(int(f["flags"])) == 3 for f in comb)
    for f in comb:
        tx = das.frame_of(sc, f)[2]
        assert bytes(f["data"][:len(tx)]) == bytes(tx)


@pytest.mark.parametrize("cuts", [1, 4])
def test_mode_0_is_set_diversity(cuts):
    sc = ds.scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    n = iq.shape[1]
    step = n // cuts
    parts = {}
    for auto in (False, True):
        b = SondeBatch(sc.C, step)
        gid = np.full(sc.C, -1, dtype=np.int32)
        for g, members in enumerate(sc.groups):
            gid[members] = g
        off = np.array(sc.offsets, dtype=np.int64)
        if auto:
            b._chk(b.L.sonde_batch_set_diversity_auto(b.h, gid.ctypes.data, off.ctypes.data, sc.window, 0))
        else:
            b._chk(b.L.sonde_batch_set_diversity(b.h, gid.ctypes.data, off.ctypes.data, sc.window))
        parts[auto] = []
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            parts[auto].append(b.frames())
        info = [b.diversity_info(g) for g in range(len(sc.groups))]
        for g, members in enumerate(sc.groups):             # the host's offsets, every member locked, for good
            assert b.diversity_offsets(g) == {"offsets": [sc.offsets[ch] for ch in members] + [0] * (4 - len(members)),
                                              "locked": (1 << len(members)) - 1, "learned": 0, "duplicates": 0}
        parts[auto].append(info)
        b.close()
    assert sum(i["combined"] for i in parts[True][-1]) >= 6 and parts[True][-1] == parts[False][-1]
    for x, y in zip(parts[True][:-1], parts[False][:-1]):
        assert x.tobytes() == y.tobytes() and not (x["flags"] & DUP).any()


def test_the_align_step_alone_equals_the_twin():
    cases = das.unit_cases()
    records, counts, nm, carried, off, locked, mode = das.pack_cases(cases)
    assert records.shape[2] == 70 and set(nm.tolist()) == {2, 3, 4} and set(mode.tolist()) == {0, 1, 2, 3}
    b = SondeBatch(1, das.TILE)
    rec, o, lk, learned, dups = b.test_diversity_align(records, counts, nm, carried, off, locked, mode)
    for bad in (dict(nm=np.where(np.arange(len(nm)) == 0, 5, nm)), dict(mode=np.where(np.arange(len(nm)) == 0, 4, mode)),
                dict(counts=np.where(np.arange(len(nm))[:, None] == 0, 71, counts))):
        with pytest.raises(SondeError):
            b.test_diversity_align(records, bad.get("counts", counts), bad.get("nm", nm), carried, off, locked, bad.get("mode", mode))
    b.close()
    for k, c in enumerate(cases):
        per, woff, wlk, wle, wdu = das.twin_case(c)
        assert ([int(v) for v in o[k]], int(lk[k]), int(learned[k]), int(dups[k])) == (woff, wlk, wle, wdu), c["name"]
        for m, p in enumerate(per):
            assert rec[k, m, :len(p)].tobytes() == p.tobytes(), (c["name"], m)
    assert int(dups.sum()) > 50 and int(learned.sum()) > 50


def test_a_restarted_learning_group_unlocks_and_locks_again():
    sc = das.scene()
    restart = (5, [0, 1, 5, 6, 11])                         # groups a and c behind the fifth of ten submits, and the ungrouped channel
    seen = {}

    def probe(b, k):
        seen["after"] = [b.diversity_offsets(g) for g in range(3)]

    off = _run(_iq(), 10, restart_at=restart)
    want, st = _twin(off, sc.groups, restart_at=restart)
    got, b = _run(_iq(), 10, sc.groups, keep=True, restart_at=restart, probe=probe)
    _same(got, want)
    _same_state(b, st, sc.groups)
    b.close()
    zero = {"offsets": [0, 0, 0, 0], "locked": 0, "learned": 0, "duplicates": 0}
    assert seen["after"][0] == zero and seen["after"][2] == zero and seen["after"][1]["locked"] == 7
    assert all(st["locked"][ch] for ch in range(7)) and st["learned"][0] == 1 and st["learned"][2] == 1
    assert abs(st["off"][6] - das.JUMP_BITS) < 64           # both bit counts start over together: the jump is still between them
    whole = _twin(_base(False, 10), sc.groups)[1]
    assert st["duplicates"][0] < whole["duplicates"][0] and st["duplicates"][1] == whole["duplicates"][1]
    # a group that was given offsets goes back to them, locked
    b = SondeBatch(sc.C, sc.n // 10)
    b.set_diversity([[0, 1]], [0, 250] + [0] * 10, das.WINDOW, learn=True)
    for k in range(4):
        b.submit(_iq()[:, k * (sc.n // 10):(k + 1) * (sc.n // 10)])
    assert b.diversity_offsets(0)["offsets"][:2] == [0, 300] and b.diversity_offsets(0)["learned"] == 1
    b.restart_channels([0, 1])
    assert b.diversity_offsets(0) == {"offsets": [0, 250, 0, 0], "locked": 3, "learned": 0, "duplicates": 0}
    b.close()


def test_the_refusals():
    types = np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)
    gid = np.array([0, 0, -1, -1, -1, -1, -1], dtype=np.int32)

    def batch(**kw):
        return SondeBatch(7, das.TILE * 8, types=types, **kw)

    b = batch()
    for mode in (4, 8, 7, 1 << 31):                         # unknown mode bits
        assert b.L.sonde_batch_set_diversity_auto(b.h, gid.ctypes.data, None, 0, mode) < 0
    with pytest.raises(SondeError):
        b.diversity_offsets(0)                               # no groups yet
    b.close()
    for kw in (dict(flags=_lib.FLAG_LATE_JOIN), dict(flags=_lib.FLAG_PIPELINE)):
        b = batch(**kw)
        with pytest.raises(SondeError):
            b.set_diversity([[0, 1]], learn=True, mark_duplicates=True)
        b.close()
    for groups, window in (([[0, 2]], 0), ([[0]], 0), ([[0, 1, 3, 4, 5]], 0), ([[0, 1]], 1201), ([[0, 1], [], [3, 4]], 0)):
        b = batch()
        with pytest.raises(SondeError):
            b.set_diversity(groups, None, window, learn=True)
        b.close()
    b = batch()
    gap = np.array([0, 0, -1, 2, 2, -1, -1], dtype=np.int32)
    assert b.L.sonde_batch_set_diversity_auto(b.h, gap.ctypes.data, None, 0, 3) < 0
    b.set_diversity([[0, 1], [3, 4, 5, 6]], None, 1200, learn=True, mark_duplicates=True)
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]], learn=True)                # a second call
    with pytest.raises(SondeError):
        b.diversity_offsets(2)
    b.close()
    b = batch()
    b.submit(torch.zeros((7, das.TILE * 8, 2), dtype=torch.float32, device=DEV))
    b.sync()
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]], mark_duplicates=True)      # after a submit
    b.close()


def test_poll_leaves_out_the_duplicates_and_only_them():
    from sdrpp_radiosonde_amd.live import frame_ok
    sc = das.scene()
    polled, frames = {}, {}
    for mark in (False, True):
        b = SondeBatch(sc.C, sc.n)
        b.set_diversity(sc.groups, None, das.WINDOW, learn=True, mark_duplicates=mark)
        b.submit(_iq())
        frames[mark] = _sorted(b.frames())
        polled[mark] = collections.Counter((ch, d.seq) for ch, d in b.poll() if d.fields & _lib.DATA_SEQ)
        b.close()
    fr = frames[True]
    assert not (frames[False]["flags"] & DUP).any() and frame_ok(frames[False]).sum() == ((fr["nerr"][:, 0] >= 0) & (fr["nerr"][:, 1] >= 0)).sum()
    marked = fr[fr["flags"] & DUP != 0]
    assert len(marked) >= 6 and frames[True].tobytes() != frames[False].tobytes()
    # without the mode every record is delivered; with it exactly the marked records' fragments are missing
    gone = collections.Counter((int(f["channel"]), 1000 + das.frame_of(sc, f)[1]) for f in marked)
    assert polled[False] - polled[True] == gone and not polled[True] - polled[False]
    # one fragment set per transmitted frame from the good records of the marking groups, and frame_ok leaves out the same records
    ok = fr[frame_ok(fr)]
    assert len(ok) == frame_ok(frames[False]).sum() - len(marked)
    per_frame = collections.Counter(das.frame_of(sc, f)[:2] for f in ok if int(f["channel"]) < 11)
    assert len(per_frame) >= 20 and set(per_frame.values()) == {1}
    for f in ok:
        assert polled[True][(int(f["channel"]), 1000 + das.frame_of(sc, f)[1])] >= 1


def test_diversity_receiver_two_antennas():
    """two RS41 sondes in one wideband stream, heard on two antennas: antenna 1 gets the same block five granules (1024 bits) late, and
    each antenna is silent for 60 ms of every frame period at a place of its own (das.fade_plan)"""
    from sdrpp_radiosonde_amd import synth
    from sdrpp_radiosonde_amd.diversity import DiversityReceiver
    from sdrpp_radiosonde_amd.tuner import WidebandReceiver
    fs, sondes = 2_400_000, [(200_000, 0), (-350_000, 0)]
    for bad in (dict(sondes=[(200_000, 0), (0, 1)]), dict(antennas=1), dict(antennas=5), dict(track=True), dict(chain="reference")):
        with pytest.raises(SondeError):
            DiversityReceiver(fs, bad.pop("sondes", sondes), **bad)
    rx = DiversityReceiver(fs, sondes, antennas=2, max_in=20 * 102_400)
    assert rx.granule == 102_400
    n, delay = 80 * rx.granule, 5 * rx.granule
    spb = fs // 4800                                         # samples per bit
    iq, frames, symbols = synth.make_wideband_scene(sondes, n, fs=fs, ebn0_db=20.0, seed=4, device=DEV)
    fades0, fades1, faded = das.fade_plan(frames, n // spb, delay // spb)
    assert len(faded) >= 3
    ant0, ant1 = iq.clone(), iq.clone()
    for c in fades0:
        ant0[c * spb:(c + das.FADE_BITS) * spb] = 0
    for c in fades1:
        ant1[c * spb:(c + das.FADE_BITS) * spb] = 0
    ant1 = torch.cat([torch.zeros_like(ant1[:delay]), ant1[:n - delay]]).contiguous()
    got, ants, frags = [], [], []
    for a in range(0, n, rx.max_in):
        rx.submit([ant0[a:a + rx.max_in], ant1[a:a + rx.max_in]])
        f, ant = rx.frames()
        got.append(f)
        ants.append(ant)
        frags += rx.poll()
    got, ants = np.concatenate(got), np.concatenate(ants)
    for i in range(2):
        o = rx.offsets(i)
        assert o["locked"] == 3 and abs(o["offsets"][1] - o["offsets"][0] - delay // spb) <= 2 and o["learned"] >= 1, o
    with pytest.raises(SondeError):
        rx.offsets(2)
    rx.close()
    assert not (got["flags"] & DUP).any() and set(ants.tolist()) == {0, 1}
    good = got[(got["nerr"][:, 0] >= 0) & (got["nerr"][:, 1] >= 0)]
    sent = 0
    for i in range(2):
        for p, tx in frames[i]:
            if p + 8 * len(tx) + 64 > symbols[i]:
                continue
            sent += 1
            hits = [f for f in good if int(f["channel"]) == i and bytes(f["data"][:len(tx)]) == bytes(tx)]
            assert len(hits) == 1, (i, p, len(hits))         # every transmitted frame, exactly once
            seq = int(tx[59]) | (int(tx[60]) << 8)
            assert sum(1 for c, d in frags if c == i and d.fields & _lib.DATA_SEQ and d.seq == seq) >= 1
    assert sent >= 8 and len(good) == sent and (good["flags"] & _lib.FRAME_COMBINED != 0).sum() >= 2
    alone = []
    for block in (ant0, ant1):                               # either antenna alone delivers fewer good frames
        wb = WidebandReceiver(fs, sondes, chain="iq48", max_in=20 * 102_400)
        cnt = 0
        for a in range(0, n, wb.max_in):
            wb.submit(block[a:a + wb.max_in])
            f = wb.frames()
            cnt += int(((f["nerr"][:, 0] >= 0) & (f["nerr"][:, 1] >= 0)).sum())
        wb.close()
        alone.append(cnt)
    assert max(alone) < sent, (alone, sent)
