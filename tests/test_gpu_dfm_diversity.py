"""-m gpu: sonde_batch_set_diversity on DFM groups (DESIGN SPEC 3.3m) against its twin (tests/dfm_diversity_reference.py) on the scenes of
tests/dfm_diversity_scenes.py: with groups set the records of every submit are the twin's over the same batch's records without
groups, whole records byte for byte, however the stream is cut and with time slices, and diversity_info reports the twin's counters;
the combining rule alone equals the twin on caller-made copies; a clean scene does not change; in a mixed batch only records of
DFM-grouped channels differ from the run with the RS41 and M10 groups alone; a frame SPEC 3.3g rescued is a good copy; the refusals
hold; a restarted group starts over; poll() delivers the fields of a combined DFM frame; a group whose offset is wrong by one frame
changes nothing."""
import numpy as np
import pytest
import torch

import check_diversity_reference as ckr
import check_diversity_scenes as cks
import dfm_diversity_reference as cr
import dfm_diversity_scenes as cs
import diversity_reference as dr
import diversity_scenes as ds
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_dev_cache, _base_cache = {}, {}


def _iq(clean=False):
    if clean not in _dev_cache:
        _dev_cache[clean] = torch.from_numpy(cs.scene(clean).iq).to(DEV)
    return _dev_cache[clean]


def _types(C=None):
    return np.full(cs.scene().C if C is None else C, cs.DFM, dtype=np.uint8)


def _run(iq, steps, groups=None, offsets=None, window=0, keep=False, restart_at=None, **kw):
    """the records of each submit, [(channel, bitpos)-sorted arrays]; steps: the submits' lengths in samples"""
    assert sum(steps) == iq.shape[1]
    b = SondeBatch(iq.shape[0], max(steps), **kw)
    if groups is not None:
        b.set_diversity(groups, offsets, window)
    parts, at = [], 0
    for k, step in enumerate(steps):
        if restart_at is not None and k == restart_at[0]:
            b.restart_channels(restart_at[1])
        b.submit(iq[:, at:at + step])
        at += step
        parts.append(cs.sort_records(b.frames()))
    if keep:
        return parts, b
    b.close()
    return parts


def _steps(variant):
    sc = cs.scene()
    if variant == "late_copy":                               # two submits cut between the copies of a frame the plan combines
        first = cs.late_cut_tiles(sc) * cs.TILE
        return [first, sc.n - first], {}
    cuts, kw = {"1_submit": (1, {}), "4_submits": (4, {}), "10_submits": (10, {}), "time_slices_3": (2, dict(time_slices=3))}[variant]
    return [sc.n // cuts] * cuts, kw


def _base(variant):
    if variant not in _base_cache:
        steps, kw = _steps(variant)
        _base_cache[variant] = _run(_iq(), steps, types=_types(), **kw)
    return _base_cache[variant]


def _twin(parts, groups, offsets, window=960, restart_at=None):
    state, want = None, []
    for k, sub in enumerate(parts):
        if restart_at is not None and k == restart_at[0] and state is not None:
            for g, members in enumerate(groups):
                if set(members) <= set(restart_at[1]):
                    cr.restart_div_group(state, groups, g)
        w, _, state = cr.diversity(sub, groups, offsets, window, state)
        want.append(w)
    return want, state


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        for a, e in zip(g, w):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))


@pytest.mark.parametrize("variant", ["1_submit", "4_submits", "10_submits", "time_slices_3", "late_copy"])
def test_with_groups_the_records_are_the_twins(variant):
    sc = cs.scene()
    steps, kw = _steps(variant)
    off = _base(variant)
    want, state = _twin(off, sc.groups, sc.offsets, sc.window)
    got, b = _run(_iq(), steps, sc.groups, sc.offsets, sc.window, keep=True, types=_types(), **kw)
    _same(got, want)
    planned = sum(1 for _, e in sc.plan.values() if e == "combined")
    assert sum(state["combined"]) == planned >= 15
    assert sum(int((g["flags"] & _lib.FRAME_COMBINED != 0).sum()) for g in got) == planned
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()
    if variant == "late_copy":       # the second submit combines a frame of the delayed pair whose other copy came with the first
        firsts = {cs.frame_of(sc, f)[:2] for f in off[0] if int(f["channel"]) == 2}
        late = [f for f in got[1] if int(f["flags"]) & _lib.FRAME_COMBINED and int(f["channel"]) == 3 and cs.frame_of(sc, f)[:2] in firsts]
        assert len(late) >= 1


def test_one_submit_delivers_the_transmitted_frames():
    sc = cs.scene()
    got = _run(_iq(), [sc.n], sc.groups, sc.offsets, sc.window, types=_types())[0]
    comb = got[got["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) == sum(1 for _, e in sc.plan.values() if e == "combined")
    seen = set()
    for f in comb:
        _, _, tx = cs.frame_of(sc, f)
        fl = int(f["flags"])
        assert bytes(f["data"][:33]) == bytes(tx) and int(f["nerr"][1]) == 0 and int(f["nerr"][0]) >= 1 and fl & _lib.FRAME_RESCUED
        seen.add((_lib.frame_copies(fl), _lib.frame_joint(fl)))
    assert seen == {(2, 0), (2, 1), (3, 0), (4, 0), (4, 1)}


def test_the_combining_rule_alone_equals_the_twin():
    copies, n_copies, names, want = cs.unit_cases()
    b = SondeBatch(1, cs.TILE)
    out, status = b.test_dfm_combine(copies, n_copies)
    b.close()
    seen = set()
    for i, name in enumerate(names):
        w, st = cr.combine(copies[i], n_copies[i])
        assert int(status[i]) == st, (i, name, int(status[i]), st)
        assert want[i] is None or st == want[i], (i, name, st, want[i])
        assert out[i].tobytes() == w.tobytes(), (i, name, st)
        seen.add(st)
    assert seen == {2, 3, 4, -1, -2, -3}


def test_the_combining_rule_refuses_what_it_cannot_take():
    copies, n_copies, _, _ = cs.unit_cases()
    b = SondeBatch(1, cs.TILE)
    for bad in (1, 5):
        with pytest.raises(SondeError):
            b.test_dfm_combine(copies[:1], np.array([bad]))
    # a good copy 0; a copy 0 of another length; a copy 0 of another type; a partner of another type; a partner of another length
    for j, field, value in ((0, "nerr", 0), (0, "len", 45), (0, "type", 3), (1, "type", 0), (1, "len", 32)):
        c = copies[:1].copy()
        if field == "nerr":
            c[0, j]["nerr"] = value
        else:
            c[0, j][field] = value
        with pytest.raises(SondeError):
            b.test_dfm_combine(c, n_copies[:1])
    b.test_dfm_combine(copies[:1], n_copies[:1])
    b.close()


def test_a_clean_scene_is_unchanged():
    sc = cs.scene(clean=True)
    steps = [sc.n // 2] * 2
    off = _run(_iq(True), steps, types=_types())
    on, b = _run(_iq(True), steps, sc.groups, sc.offsets, sc.window, keep=True, types=_types())
    assert sum(len(p) for p in off) > 200
    _same(on, off)
    assert all(b.diversity_info(g) == {"tried": 0, "combined": 0} for g in range(len(sc.groups)))
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_SPLIT_FEC], ids=["one_launch", "split_fec_units"])
def test_mixed_batch_only_dfm_grouped_records_differ_from_the_run_with_the_other_groups_alone(flags):
    rs, m10, dfm = ds.scene(), cks.scene("m10"), cs.scene()
    n = rs.n
    assert m10.n == n and dfm.n < n
    rs_iq, m10_iq = torch.from_numpy(rs.iq).to(DEV), torch.from_numpy(m10.iq).to(DEV)
    dfm_iq = torch.cat([_iq(), _iq()[:, :n - dfm.n]], dim=1)       # the scene, and its beginning once more behind it
    # RS41: a pair of its scene; M10: a pair of its scene; DFM: the pair, the delayed pair and the triple; ungrouped: a DFM, an M10, an iMS-100
    src = [(0, rs_iq, 0), (0, rs_iq, 1), (3, m10_iq, 0), (3, m10_iq, 1), (1, dfm_iq, 0), (1, dfm_iq, 1), (1, dfm_iq, 2), (1, dfm_iq, 3),
           (1, dfm_iq, 4), (1, dfm_iq, 5), (1, dfm_iq, 6), (1, dfm_iq, 7), (3, m10_iq, 9), (2, None, 0)]
    types = np.array([t for t, _, _ in src], dtype=np.uint8)
    rows = [x[c, :n] if x is not None else synth.make_batch(int(t), 1, n, seed=77, ebn0_db=25.0, first_channel=i).iq[0].to(DEV)
            for i, (t, x, c) in enumerate(src)]
    iq = torch.stack(rows).contiguous()
    old_groups, all_groups = [[0, 1], [2, 3]], [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9, 10]]
    offsets = [0, 0, 0, 0, 0, 0, 0, 300, 0, 0, 0, 0, 0, 0]
    steps = [n // 2] * 2
    off = _run(iq, steps, types=types, flags=flags)
    old_only = _run(iq, steps, old_groups, offsets, 0, types=types, flags=flags)
    on, b = _run(iq, steps, all_groups, offsets, 0, keep=True, types=types, flags=flags)
    st_rs, st_ck, st_dfm, want = None, None, None, []
    for sub in off:
        w, _, st_rs = dr.diversity(sub, [[0, 1], []], offsets, 960, st_rs)
        w, _, st_ck = ckr.diversity(w, [[], [2, 3]], offsets, 960, st_ck)
        assert w.tobytes() == old_only[len(want)].tobytes()
        w, _, st_dfm = cr.diversity(w, [[], []] + all_groups[2:], offsets, 960, st_dfm)
        want.append(w)
    _same(on, want)
    a, o, r = np.concatenate(on), np.concatenate(off), np.concatenate(old_only)
    dfm_grouped = np.isin(a["channel"], range(4, 11))
    assert a[~dfm_grouped].tobytes() == r[~dfm_grouped].tobytes() and r[dfm_grouped].tobytes() == o[dfm_grouped].tobytes()
    changed = np.array([x.tobytes() != y.tobytes() for x, y in zip(a, r)])
    assert changed.sum() == sum(st_dfm["combined"]) and set(a["channel"][changed].tolist()) <= set(range(4, 11))
    assert st_rs["combined"][0] >= 2 and st_ck["combined"][1] >= 2 and min(st_dfm["combined"][2:]) >= 4
    assert ((o["channel"] == 11) & (o["nerr"][:, 1] > 0)).sum() >= 4          # the ungrouped DFM channel's failed frames stay
    for g in range(5):
        st = st_rs if g == 0 else st_ck if g == 1 else st_dfm
        assert b.diversity_info(g) == {"tried": st["tried"][g], "combined": st["combined"][g]}, g
    b.close()


def test_a_frame_the_dfm_rescue_completed_is_a_good_copy():
    """cs.rescued_partner_scene: in every other damaged frame receiver 0 fails with nothing SPEC 3.3g could go on while receiver 1's
    copy is one SPEC 3.3g rescues -- the failed copy meets a rescued partner, which is a good copy: it stays as recorded and nothing is
    tried.  In the frames between, both copies stay failed and the pass combines them.  Without the flag the first kind of frame is
    combined too."""
    sc = cs.rescued_partner_scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    off = _run(iq, [sc.n], types=_types(2), flags=_lib.FLAG_DFM_RESCUE)[0]
    on, b = _run(iq, [sc.n], sc.groups, None, 0, keep=True, types=_types(2), flags=_lib.FLAG_DFM_RESCUE)
    want, outcomes, state = cr.diversity(off, sc.groups, None, 960)
    _same(on, [want])
    n_rescued = n_hidden = 0
    for f, o, out in zip(off, on[0], outcomes):
        k = cs.frame_of(sc, f)[1]
        ch, case = int(f["channel"]), sc.plan[k]
        if case == "rescued_partner":
            n_rescued += ch == 0
            if ch == 0:           # failed, nothing marked, and its partner was rescued: stays as recorded
                assert int(f["nerr"][1]) > 0 and out == "partner_good" and o.tobytes() == f.tobytes(), k
            else:
                assert int(f["flags"]) & _lib.FRAME_RESCUED and int(f["nerr"][1]) == 0 and not int(o["flags"]) & _lib.FRAME_COMBINED, k
                assert out == "good" and o.tobytes() == f.tobytes(), k
        elif case == "both_hidden":
            n_hidden += ch == 0
            assert int(f["nerr"][1]) > 0 and not int(f["flags"]) & _lib.FRAME_RESCUED, (k, ch)
            assert out == ("combined" if ch == 0 else "partner_good"), (k, ch, out)
            if ch == 0:
                assert int(o["flags"]) & _lib.FRAME_COMBINED and bytes(o["data"][:33]) == bytes(cs.frame_of(sc, f)[2]), k
    assert n_rescued >= 3 and n_hidden >= 3
    assert b.diversity_info(0) == {"tried": n_hidden, "combined": n_hidden} == {"tried": state["tried"][0], "combined": state["combined"][0]}
    b.close()
    plain = _run(iq, [sc.n], sc.groups, None, 0, types=_types(2))[0]
    assert (plain["flags"] & _lib.FRAME_COMBINED != 0).sum() == n_rescued + n_hidden


def test_the_refusals():
    types = np.array([1, 1, 0, 0, 2, 2, 1, 1, 1, 1, 4, 5], dtype=np.uint8)

    def batch(**kw):
        return SondeBatch(12, cs.TILE * 8, types=types, **kw)

    for kw in (dict(flags=_lib.FLAG_LATE_JOIN), dict(flags=_lib.FLAG_PIPELINE)):
        b = batch(**kw)
        with pytest.raises(SondeError):
            b.set_diversity([[0, 1]])
        b.close()
    # DFM + RS41; DFM + iMS-100; an iMS-100 pair; DFM + iMet; DFM + C50; five members; one member; the window; a gap
    for groups, window in (([[0, 2]], 0), ([[1, 4]], 0), ([[4, 5]], 0), ([[0, 10]], 0), ([[0, 11]], 0), ([[0, 1, 6, 7, 8]], 0), ([[0]], 0),
                           ([[0, 1]], 1201), ([[0, 1], [], [6, 7]], 0)):
        b = batch()
        with pytest.raises(SondeError):
            b.set_diversity(groups, None, window)
        b.close()
    b = batch()
    b.set_diversity([[0, 1], [2, 3], [6, 7, 8, 9]], None, 1200)              # DFM groups next to an RS41 group
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                                           # a second call
    b.close()


def test_restart_takes_whole_groups_and_clears_them():
    sc = cs.scene()
    steps = [sc.n // 10] * 10
    b = SondeBatch(sc.C, steps[0], types=_types())
    b.set_diversity(sc.groups, sc.offsets, sc.window)
    b.submit(_iq()[:, :steps[0]])
    for part in ([0], [4, 5], [0, 1, 2]):
        with pytest.raises(SondeError):
            b.restart_channels(part)
    b.restart_channels([7])                                  # a channel in no group: as before
    b.close()
    # the first pair, the triple and the ungrouped channel restart behind the fifth of ten submits
    restart = (5, [0, 1, 4, 5, 6, 7])
    off = _run(_iq(), steps, restart_at=restart, types=_types())
    want, state = _twin(off, sc.groups, sc.offsets, sc.window, restart)
    on, b = _run(_iq(), steps, sc.groups, sc.offsets, sc.window, keep=True, restart_at=restart, types=_types())
    _same(on, want)
    _, st_whole = _twin(_base("10_submits"), sc.groups, sc.offsets, sc.window)
    assert state["combined"][0] < st_whole["combined"][0] and state["combined"][1] == st_whole["combined"][1] >= 2
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()


def _seqs(records):
    """what the poll parser makes of the frame counters (sub-packet id 0) of the DFM records it takes (nerr[1] == 0), in order"""
    out = []
    for f in records:
        if int(f["nerr"][1]) != 0:
            continue
        for blk in range(2):
            cw = f["data"][7 + 13 * blk:7 + 13 * blk + 13]
            if cw[12] >> 4 == 0:
                out.append(int((cw[6] >> 4) << 4 | (cw[7] >> 4)))
    return out


def test_poll_delivers_the_fields_of_a_combined_dfm_frame():
    sc = cs.scene()
    got, recs = {}, {}
    for on in (False, True):
        b = SondeBatch(sc.C, sc.n, types=_types())
        if on:
            b.set_diversity(sc.groups, sc.offsets, sc.window)
        b.submit(_iq())
        fr = cs.sort_records(b.frames())
        recs[on] = fr[fr["channel"] == 8]                      # the quad's first receiver: its frames with a counter are damaged ones
        got[on] = [int(d.seq) for ch, d in b.poll() if ch == 8 and d.fields & _lib.DATA_SEQ]
        b.close()
    assert (recs[True]["flags"] & _lib.FRAME_COMBINED != 0).sum() >= 6
    assert got[False] == _seqs(recs[False]) and got[True] == _seqs(recs[True]) and len(got[True]) >= len(got[False]) + 2


def test_a_group_whose_offset_is_wrong_by_one_frame_changes_nothing():
    sc = cs.scene()
    off = _base("1_submit")
    on, b = _run(_iq(), [sc.n], sc.groups, cs.OFFSETS_WRONG, sc.window, keep=True, types=_types())
    want, state = _twin(off, sc.groups, cs.OFFSETS_WRONG, sc.window)
    _same(on, want)
    mine = np.isin(off[0]["channel"], sc.groups[0])
    assert on[0][mine].tobytes() == off[0][mine].tobytes()
    assert b.diversity_info(0)["combined"] == 0 and b.diversity_info(0)["tried"] == state["tried"][0] >= 8
    assert b.diversity_info(2)["combined"] == state["combined"][2] >= 5
    b.close()
