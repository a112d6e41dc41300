"""-m gpu: sonde_batch_set_diversity on M10 / M20 / MRZ-N1 groups (DESIGN SPEC 3.3l) against its twin (tests/check_diversity_reference.py)
on the scenes of tests/check_diversity_scenes.py: with groups set the records of every submit are the twin's over the same batch's
records without groups, whole records byte for byte, however the stream is cut and with time slices, and diversity_info reports the
twin's counters; the combining rule alone equals the twin on caller-made copies; a clean scene does not change; in a mixed batch only
records of grouped channels change and the RS41 records are what they are with the RS41 groups alone; a frame SPEC 3.3f rescued is a
good copy; the refusals hold; a restarted group starts over; poll() delivers the fields of a combined M10 frame."""
import numpy as np
import pytest
import torch

import check_diversity_reference as cr
import check_diversity_scenes as cs
import diversity_reference as dr
import diversity_scenes as ds
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = list(cs.KINDS)
_dev_cache, _base_cache = {}, {}


def _iq(kind, clean=False):
    key = (kind, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(cs.scene(kind, clean).iq).to(DEV)
    return _dev_cache[key]


def _types(kind):
    return np.full(cs.scene(kind).C, cs.KINDS[kind][0], dtype=np.uint8)


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


def _steps(kind, variant):
    sc = cs.scene(kind)
    if variant == "late_copy":                               # two submits cut between the copies of a frame the plan combines
        first = cs.late_cut_tiles(sc) * cs.TILE
        return [first, sc.n - first], {}
    cuts, kw = {"1_submit": (1, {}), "4_submits": (4, {}), "10_submits": (10, {}), "time_slices_3": (2, dict(time_slices=3))}[variant]
    return [sc.n // cuts] * cuts, kw


def _base(kind, variant):
    if (kind, variant) not in _base_cache:
        steps, kw = _steps(kind, variant)
        _base_cache[(kind, variant)] = _run(_iq(kind), steps, types=_types(kind), **kw)
    return _base_cache[(kind, variant)]


def _twin(parts, sc, restart_at=None):
    state, want = None, []
    for k, sub in enumerate(parts):
        if restart_at is not None and k == restart_at[0] and state is not None:
            for g, members in enumerate(sc.groups):
                if set(members) <= set(restart_at[1]):
                    cr.restart_div_group(state, sc.groups, g)
        w, _, state = cr.diversity(sub, sc.groups, sc.offsets, sc.window, state)
        want.append(w)
    return want, state


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        for a, e in zip(g, w):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))


@pytest.mark.parametrize("variant", ["1_submit", "4_submits", "10_submits", "time_slices_3", "late_copy"])
@pytest.mark.parametrize("kind", KINDS)
def test_with_groups_the_records_are_the_twins(kind, variant):
    sc = cs.scene(kind)
    steps, kw = _steps(kind, variant)
    off = _base(kind, variant)
    want, state = _twin(off, sc)
    got, b = _run(_iq(kind), steps, sc.groups, sc.offsets, sc.window, keep=True, types=_types(kind), **kw)
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


@pytest.mark.parametrize("kind", KINDS)
def test_one_submit_delivers_the_transmitted_frames(kind):
    sc = cs.scene(kind)
    got = _run(_iq(kind), [sc.n], sc.groups, sc.offsets, sc.window, types=_types(kind))[0]
    comb = got[got["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) == sum(1 for _, e in sc.plan.values() if e == "combined")
    seen = set()
    for f in comb:
        _, _, tx = cs.frame_of(sc, f)
        fl = int(f["flags"])
        assert bytes(f["data"][:sc.len]) == bytes(tx) and int(f["nerr"][0]) == 0 and fl & _lib.FRAME_RESCUED
        assert _lib.frame_copies(fl) in (2, 3, 4)
        seen.add((_lib.frame_copies(fl), _lib.frame_unknowns(fl)))
    assert {(3, 15), (3, 5), (4, 5), (2, 8), (2, 6), (2, 2)} <= seen


def test_the_combining_rule_alone_equals_the_twin():
    copies, n_copies, names, want = cs.unit_cases()
    b = SondeBatch(1, cs.TILE)
    out, status = b.test_check_combine(copies, n_copies)
    b.close()
    seen = set()
    for i, name in enumerate(names):
        w, st = cr.combine(copies[i], n_copies[i])
        assert int(status[i]) == st, (i, name, int(status[i]), st)
        assert want[i] is None or st == want[i], (i, name, st, want[i])
        assert out[i].tobytes() == w.tobytes(), (i, name, st)
        seen.add(st if st < 0 else int(n_copies[i]))
    assert seen == {2, 3, 4, -1, -2, -3}


def test_the_combining_rule_refuses_what_it_cannot_take():
    copies, n_copies, _, _ = cs.unit_cases()
    b = SondeBatch(1, cs.TILE)
    for bad in (1, 5):
        with pytest.raises(SondeError):
            b.test_check_combine(copies[:1], np.array([bad]))
    for field, value in (("nerr", 0), ("len", 45), ("type", 0)):       # a good copy 0; copies of differing len; a type the rule is not for
        c = copies[:1].copy()
        if field == "nerr":
            c[0, 0]["nerr"] = value
        else:
            c[0, 0][field] = value
        with pytest.raises(SondeError):
            b.test_check_combine(c, n_copies[:1])
    c = copies[:1].copy()
    c[0, 1]["type"] = 6                                       # copies of differing type
    with pytest.raises(SondeError):
        b.test_check_combine(c, n_copies[:1])
    b.close()


@pytest.mark.parametrize("kind", ["m10", "mrz"])
def test_a_clean_scene_is_unchanged(kind):
    sc = cs.scene(kind, clean=True)
    steps = [sc.n // 2] * 2
    off = _run(_iq(kind, True), steps, types=_types(kind))
    on, b = _run(_iq(kind, True), steps, sc.groups, sc.offsets, sc.window, keep=True, types=_types(kind))
    assert sum(len(p) for p in off) > 100
    _same(on, off)
    assert all(b.diversity_info(g) == {"tried": 0, "combined": 0} for g in range(len(sc.groups)))
    b.close()


@pytest.mark.parametrize("flags", [0, _lib.FLAG_SPLIT_FEC], ids=["one_launch", "split_fec_units"])
def test_mixed_batch_only_grouped_records_change_and_rs41_groups_are_what_they_were(flags):
    rs, m10, mrz = ds.scene(), cs.scene("m10"), cs.scene("mrz")
    n = rs.n
    assert m10.n == n and mrz.n >= n
    rs_iq = torch.from_numpy(rs.iq).to(DEV)
    # RS41: two pairs of its scene (the second with a 300-bit delay); M10: pairs 0 and 1 of its scene; MRZ-N1: pair 0; ungrouped DFM and M10
    src = [(0, rs_iq, 0), (0, rs_iq, 1), (0, rs_iq, 2), (0, rs_iq, 3), (3, _iq("m10"), 0), (3, _iq("m10"), 1), (3, _iq("m10"), 2),
           (3, _iq("m10"), 3), (6, _iq("mrz"), 0), (6, _iq("mrz"), 1), (1, None, 0), (3, _iq("m10"), 9)]
    types = np.array([t for t, _, _ in src], dtype=np.uint8)
    rows = [x[c, :n] if x is not None else synth.make_batch(int(t), 1, n, seed=77, ebn0_db=25.0, first_channel=i).iq[0].to(DEV)
            for i, (t, x, c) in enumerate(src)]
    iq = torch.stack(rows).contiguous()
    rs_groups, all_groups = [[0, 1], [2, 3]], [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]
    offsets = [0, 0, 0, 300, 0, 0, 0, 300, 0, 0, 0, 0]
    steps = [n // 2] * 2
    off = _run(iq, steps, types=types, flags=flags)
    rs_only = _run(iq, steps, rs_groups, offsets, 0, types=types, flags=flags)
    on, b = _run(iq, steps, all_groups, offsets, 0, keep=True, types=types, flags=flags)
    st_rs, st_ck, want = None, None, []
    for sub in off:
        w, _, st_rs = dr.diversity(sub, rs_groups, offsets, 960, st_rs)
        w, _, st_ck = cr.diversity(w, [[], []] + all_groups[2:], offsets, 960, st_ck)
        want.append(w)
    _same(on, want)
    a, o, r = np.concatenate(on), np.concatenate(off), np.concatenate(rs_only)
    is_rs = a["type"] == 0
    assert a[is_rs].tobytes() == r[is_rs].tobytes() and r[~is_rs].tobytes() == o[~is_rs].tobytes()
    changed = np.array([x.tobytes() != y.tobytes() for x, y in zip(a, o)])
    assert changed.sum() == sum(st_rs["combined"]) + sum(st_ck["combined"])
    assert sum(st_rs["combined"]) >= 4 and st_ck["combined"][2] >= 2 and st_ck["combined"][3] >= 2 and st_ck["combined"][4] >= 1
    assert set(a["channel"][changed].tolist()) <= set(range(10))
    assert ((o["channel"] == 10) & (o["type"] == 1)).sum() >= 4 and ((o["channel"] == 11) & (o["nerr"][:, 0] < 0)).sum() >= 2
    for g in range(5):
        st = st_rs if g < 2 else st_ck
        assert b.diversity_info(g) == {"tried": st["tried"][g], "combined": st["combined"][g]}, g
    b.close()


def test_a_frame_the_manchester_rescue_corrected_is_a_good_copy():
    """cs.rescued_partner_scene: in every other damaged frame receiver 0 fails with nothing SPEC 3.3f could go on while receiver 1's
    copy is one SPEC 3.3f rescues -- the failed copy meets a rescued partner, which is a good copy: its visit ends as partner_good,
    it stays as recorded and nothing is tried.  In the frames between, both copies stay failed and the pass combines them.  Without
    the flag (or with the pass in front of the rescue) the first kind of frame would be combined too."""
    sc = cs.rescued_partner_scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    types = np.full(2, 3, dtype=np.uint8)
    off = _run(iq, [sc.n], types=types, flags=_lib.FLAG_MANCHESTER_RESCUE)[0]
    on, b = _run(iq, [sc.n], sc.groups, None, 0, keep=True, types=types, flags=_lib.FLAG_MANCHESTER_RESCUE)
    want, outcomes, state = cr.diversity(off, sc.groups, None, 960)
    _same(on, [want])
    got = on[0]
    n_rescued = n_hidden = 0
    for f, o, out in zip(off, got, outcomes):
        k = cs.frame_of(sc, f)[1]
        ch, case = int(f["channel"]), sc.plan[k]
        if case == "rescued_partner":
            n_rescued += ch == 0
            if ch == 0:       # failed, nothing marked, and its partner was rescued: stays as recorded
                assert int(f["nerr"][0]) < 0 and int(f["nerr"][1]) == 0 and out == "partner_good" and o.tobytes() == f.tobytes(), k
            else:
                assert int(f["flags"]) & _lib.FRAME_RESCUED and int(f["nerr"][0]) == 0 and not int(o["flags"]) & _lib.FRAME_COMBINED, k
                assert out == "good" and o.tobytes() == f.tobytes(), k
        elif case == "both_hidden":
            n_hidden += ch == 0
            assert int(f["nerr"][0]) < 0 and not int(f["flags"]) & _lib.FRAME_RESCUED, (k, ch)
            assert out == ("combined" if ch == 0 else "partner_good"), (k, ch, out)
            if ch == 0:
                assert int(o["flags"]) & _lib.FRAME_COMBINED and bytes(o["data"][:sc.len]) == bytes(cs.frame_of(sc, f)[2]), k
    assert n_rescued >= 3 and n_hidden >= 3
    assert b.diversity_info(0) == {"tried": n_hidden, "combined": n_hidden} == {"tried": state["tried"][0], "combined": state["combined"][0]}
    b.close()
    # with the flag off the partner of the first kind of frame stays failed, and the pass combines those frames too
    plain = _run(iq, [sc.n], sc.groups, None, 0, types=types)[0]
    assert (plain["flags"] & _lib.FRAME_COMBINED != 0).sum() == n_rescued + n_hidden


def test_the_refusals():
    types = np.array([3, 3, 6, 6, 0, 0, 1, 2, 4, 5], dtype=np.uint8)

    def batch(**kw):
        return SondeBatch(10, cs.TILE * 8, types=types, **kw)

    for kw in (dict(flags=_lib.FLAG_LATE_JOIN), dict(flags=_lib.FLAG_PIPELINE)):
        b = batch(**kw)
        with pytest.raises(SondeError):
            b.set_diversity([[0, 1]])
        b.close()
    # mixed types in one group (M10 + MRZ-N1, M10 + RS41, MRZ-N1 + RS41); a member of a type outside the three; sizes; the window; a gap
    for groups, window in (([[0, 2]], 0), ([[1, 4]], 0), ([[2, 3, 5]], 0), ([[0, 1, 6]], 0), ([[6, 7]], 0), ([[8, 9]], 0), ([[0]], 0),
                           ([[0, 1]], 1201), ([[0, 1], [], [2, 3]], 0)):
        b = batch()
        with pytest.raises(SondeError):
            b.set_diversity(groups, None, window)
        b.close()
    b = batch()
    gid = np.array([0, 0, 2, 2, -1, -1, -1, -1, -1, -1], dtype=np.int32)   # group ids with a gap, through the C entry
    assert b.L.sonde_batch_set_diversity(b.h, gid.ctypes.data, None, 0) < 0
    b.set_diversity([[0, 1], [2, 3], [4, 5]], None, 1200)                  # one group of each kind
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                                           # a second call
    b.close()
    b = batch()
    b.submit(torch.zeros((10, cs.TILE * 8, 2), dtype=torch.float32, device=DEV))
    b.sync()
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                                           # after a submit
    b.close()


def test_restart_takes_whole_groups_and_clears_them():
    sc = cs.scene("m10")
    steps = [sc.n // 10] * 10
    b = SondeBatch(sc.C, steps[0], types=_types("m10"))
    b.set_diversity(sc.groups, sc.offsets, sc.window)
    b.submit(_iq("m10")[:, :steps[0]])
    for part in ([0], [6, 7], [0, 1, 2]):
        with pytest.raises(SondeError):
            b.restart_channels(part)
    b.restart_channels([9])                                  # a channel in no group: as before
    b.close()
    # the first pair, the triple and the ungrouped channel restart behind the fifth of ten submits
    restart = (5, [0, 1, 6, 7, 8, 9])
    off = _run(_iq("m10"), steps, restart_at=restart, types=_types("m10"))
    want, state = _twin(off, sc, restart)
    on, b = _run(_iq("m10"), steps, sc.groups, sc.offsets, sc.window, keep=True, restart_at=restart, types=_types("m10"))
    _same(on, want)
    _, st_whole = _twin(_base("m10", "10_submits"), sc)
    assert state["combined"][0] < st_whole["combined"][0] and state["combined"][1] == st_whole["combined"][1] >= 2
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()


def test_poll_delivers_the_fields_of_a_combined_m10_frame():
    sc = cs.scene("m10")
    alts = {}
    for on in (False, True):
        b = SondeBatch(sc.C, sc.n, types=_types("m10"))
        if on:
            b.set_diversity(sc.groups, sc.offsets, sc.window)
        b.submit(_iq("m10"))
        fr = cs.sort_records(b.frames())
        alts[on] = {(ch, round(float(d.alt))) for ch, d in b.poll() if d.fields}
        b.close()
    comb = fr[fr["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) >= 15
    # synth's frame k of a stream reports the altitude 1000 + 5 k m: the combined frames' altitudes are delivered, and only with groups
    new = {(int(f["channel"]), 1000 + 5 * cs.frame_of(sc, f)[1]) for f in comb}
    assert alts[False] <= alts[True] and new <= alts[True] - alts[False], (sorted(new), sorted(alts[True] - alts[False]))
