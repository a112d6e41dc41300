"""-m gpu: sonde_batch_set_diversity (DESIGN SPEC 3.3j) against its twin (tests/diversity_reference.py) on the scenes of
tests/diversity_scenes.py: with groups set the records of every submit are the twin's over the same batch's records without groups,
whole records byte for byte, however the stream is cut and with time slices, and diversity_info reports the twin's counters; the
combining rule alone equals the twin on caller-made copies; without the call the records are the oracle's; a clean scene does not
change; in a mixed batch only RS41 records of grouped channels change; the refusals hold; a restarted group starts over; poll()
delivers the blocks of a combined frame."""
import numpy as np
import pytest
import torch

import diversity_reference as dr
import diversity_scenes as ds
from rescue_reference import block_ok
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_dev_cache, _base_cache = {}, {}


def _iq(extended=False, clean=False):
    key = (extended, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(ds.scene(extended, clean).iq).to(DEV)
    return _dev_cache[key]


def _sorted(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


def _run(iq, cuts=1, groups=None, offsets=None, window=0, keep=False, restart_at=None, **kw):
    """the records of each submit, [(channel, bitpos)-sorted arrays]"""
    C_, n = iq.shape[0], iq.shape[1]
    assert (n // ds.TILE) % cuts == 0
    step = n // cuts
    b = SondeBatch(C_, step, **kw)
    if groups is not None:
        b.set_diversity(groups, offsets, window)
    parts = []
    for k in range(cuts):
        if restart_at is not None and k == restart_at[0]:
            b.restart_channels(restart_at[1])
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


def _twin(parts, sc, restart_at=None):
    state, want = None, []
    for k, sub in enumerate(parts):
        if restart_at is not None and k == restart_at[0] and state is not None:
            for g, members in enumerate(sc.groups):
                if set(members) <= set(restart_at[1]):
                    dr.restart_group(state, sc.groups, g)
        w, _, state = dr.diversity(sub, sc.groups, sc.offsets, sc.window, state)
        want.append(w)
    return want, state


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        for a, e in zip(g, w):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))


@pytest.mark.parametrize("variant", ["1_submit", "4_submits", "10_submits", "time_slices_3"])
@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
def test_with_groups_the_records_are_the_twins(extended, variant):
    sc = ds.scene(extended)
    cuts, kw = {"1_submit": (1, {}), "4_submits": (4, {}), "10_submits": (10, {}), "time_slices_3": (2, dict(time_slices=3))}[variant]
    off = _base(extended, cuts, **kw)
    want, state = _twin(off, sc)
    got, b = _run(_iq(extended), cuts, sc.groups, sc.offsets, sc.window, keep=True, **kw)
    _same(got, want)
    assert sum(state["combined"]) >= 6
    assert sum(int((g["flags"] & _lib.FRAME_COMBINED != 0).sum()) for g in got) == sum(state["combined"])
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()


def test_one_submit_equals_the_oracle_and_delivers_the_transmitted_frames():
    sc = ds.scene()
    off = _base(False, 1)
    assert off[0].tobytes() == ds.oracle_frames().tobytes()
    got = _run(_iq(), 1, sc.groups, sc.offsets, sc.window)[0]
    comb = got[got["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) >= 6
    for f in comb:
        tx = ds.frame_of(sc, f)[2]
        assert bytes(f["data"][:len(tx)]) == bytes(tx) and _lib.frame_copies(int(f["flags"])) in (2, 3) and int(f["flags"]) & _lib.FRAME_RESCUED


def test_the_combining_rule_alone_equals_the_twin():
    copies, n_copies, names = ds.unit_cases()
    b = SondeBatch(1, ds.TILE)
    out, status = b.test_rs41_combine(copies, n_copies)
    b.close()
    seen = set()
    for i, name in enumerate(names):
        w, st = dr.combine(copies[i], n_copies[i])
        assert int(status[i]) == st, (i, name, int(status[i]), st)
        assert out[i].tobytes() == w.tobytes(), (i, name, st)
        seen.add(min(st, 0))
    assert seen == {0, -1, -2, -3}


def test_the_combining_rule_refuses_what_it_cannot_take():
    copies, n_copies, _ = ds.unit_cases()
    b = SondeBatch(1, ds.TILE)
    for bad in (1, 5):
        with pytest.raises(SondeError):
            b.test_rs41_combine(copies[:1], np.array([bad]))
    good_first = copies[:1].copy()
    good_first[0, 0]["nerr"] = 0
    with pytest.raises(SondeError):
        b.test_rs41_combine(good_first, n_copies[:1])
    b.close()


def test_without_the_call_nothing_changes_and_info_raises():
    got, b = _run(_iq(), 1, keep=True)
    assert got[0].tobytes() == ds.oracle_frames().tobytes()
    with pytest.raises(SondeError):
        b.diversity_info(0)
    b.close()


def test_a_clean_scene_is_unchanged():
    sc = ds.scene(clean=True)
    off = _run(_iq(clean=True), 2)
    on, b = _run(_iq(clean=True), 2, sc.groups, sc.offsets, sc.window, keep=True)
    assert sum(len(p) for p in off) > 50
    _same(on, off)
    assert np.concatenate(off).tobytes() != b"" and _sorted(np.concatenate(off)).tobytes() == ds.oracle_frames(clean=True).tobytes()
    assert all(b.diversity_info(g) == {"tried": 0, "combined": 0} for g in range(len(sc.groups)))
    with pytest.raises(SondeError):
        b.diversity_info(len(sc.groups))
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_SPLIT_FEC, _lib.FLAG_RS41_RESCUE], ids=["one_launch", "split_fec_units", "with_rs41_rescue"])
def test_mixed_batch_only_grouped_rs41_records_change(flags):
    sc = ds.scene()
    types = np.array([0, 0, 1, 3, 0, 0, 0], dtype=np.uint8)
    src = [0, 1, None, None, 2, 3, 7]                        # RS41 rows: two pairs of the scene and its ungrouped channel
    groups, offsets = [[0, 1], [4, 5]], [0, 0, 0, 0, 0, 300, 0]
    rows = []
    for c, (t, s) in enumerate(zip(types, src)):
        rows.append(_iq()[s] if s is not None else synth.make_batch(int(t), 1, sc.n, seed=70 + c, ebn0_db=25.0, first_channel=c).iq[0].to(DEV))
    iq = torch.stack(rows).contiguous()
    off = _run(iq, 2, types=types, flags=flags)
    on, b = _run(iq, 2, groups, offsets, 0, keep=True, types=types, flags=flags)
    state, want = None, []
    for sub in off:
        w, _, state = dr.diversity(sub, groups, offsets, 960, state)
        want.append(w)
    _same(on, want)
    a, o = np.concatenate(on), np.concatenate(off)
    changed = np.array([x.tobytes() != y.tobytes() for x, y in zip(a, o)])
    assert changed.sum() == sum(state["combined"]) >= 4
    assert set(a["channel"][changed].tolist()) <= {0, 1, 4, 5} and (a["type"][changed] == 0).all()
    assert (o["type"] != 0).sum() >= 8
    if flags & _lib.FLAG_RS41_RESCUE:       # what SPEC 3.3c rescued is a good copy: it is never combined, and its partners stay
        both = (a["flags"] & _lib.FRAME_RESCUED != 0) & (a["flags"] & _lib.FRAME_COMBINED == 0)
        assert both.sum() >= 1 and b.rescue_info(0)["rescued"] + b.rescue_info(1)["rescued"] + b.rescue_info(4)["rescued"] + b.rescue_info(5)["rescued"] >= 1
    assert b.diversity_info(1) == {"tried": state["tried"][1], "combined": state["combined"][1]}
    b.close()


def test_the_refusals():
    types = np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)

    def batch(**kw):
        return SondeBatch(7, ds.TILE * 8, types=types, **kw)

    for kw in (dict(flags=_lib.FLAG_LATE_JOIN), dict(flags=_lib.FLAG_PIPELINE)):
        b = batch(**kw)
        with pytest.raises(SondeError):
            b.set_diversity([[0, 1]])
        b.close()
    for groups, window in (([[0, 2]], 0), ([[0]], 0), ([[0, 1, 3, 4, 5]], 0), ([[0, 1]], 1201), ([[0, 1], [], [3, 4]], 0)):
        b = batch()
        with pytest.raises(SondeError):
            b.set_diversity(groups, None, window)
        b.close()
    b = batch()
    gid = np.array([0, 0, -1, 2, 2, -1, -1], dtype=np.int32)            # group ids with a gap, through the C entry
    assert b.L.sonde_batch_set_diversity(b.h, gid.ctypes.data, None, 0) < 0
    b.set_diversity([[0, 1], [3, 4, 5, 6]], None, 1200)
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                            # a second call
    b.close()
    b = batch()
    b.submit(torch.zeros((7, ds.TILE * 8, 2), dtype=torch.float32, device=DEV))
    b.sync()
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                            # after a submit
    b.close()


def test_restart_takes_whole_groups_and_clears_them():
    sc = ds.scene()
    b = SondeBatch(sc.C, sc.n // 10)
    b.set_diversity(sc.groups, sc.offsets, sc.window)
    b.submit(_iq()[:, :sc.n // 10])
    for part in ([0], [4, 5], [0, 1, 2]):
        with pytest.raises(SondeError):
            b.restart_channels(part)
    b.restart_channels([7])                                  # a channel in no group: as before
    b.close()
    # groups 0 and 2 restart behind the fifth of ten submits: what they carried and counted is gone, the others go on
    restart = (5, [0, 1, 4, 5, 6, 7])
    off = _run(_iq(), 10, restart_at=restart)
    want, state = _twin(off, sc, restart)
    on, b = _run(_iq(), 10, sc.groups, sc.offsets, sc.window, keep=True, restart_at=restart)
    _same(on, want)
    whole, st_whole = _twin(_base(False, 10), sc)
    assert state["combined"][0] < st_whole["combined"][0] and state["combined"][1] == st_whole["combined"][1] >= 2
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()


def test_poll_delivers_the_blocks_of_a_combined_frame():
    sc = ds.scene()
    seqs = {}
    for on in (False, True):
        b = SondeBatch(sc.C, sc.n)
        if on:
            b.set_diversity(sc.groups, sc.offsets, sc.window)
        b.submit(_iq())
        fr = b.frames()
        seqs[on] = {(ch, d.seq) for ch, d in b.poll() if d.fields & _lib.DATA_SEQ}
        b.close()
    off = _base(False, 1)[0]
    new = set()
    for f, o in zip(_sorted(fr), off):
        if int(f["flags"]) & _lib.FRAME_COMBINED and not block_ok([int(v) for v in o["data"][:320]], 57, 40):
            new.add((int(f["channel"]), 1000 + ds.frame_of(sc, f)[1]))
    assert len(new) >= 1 and seqs[False] <= seqs[True] and new <= seqs[True] - seqs[False], (new, seqs[True] - seqs[False])
