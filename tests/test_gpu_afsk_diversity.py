"""-m gpu: sonde_batch_set_diversity on iMet and SRS-C50 groups (SONDE_FLAG_AFSK_DIVERSITY, DESIGN SPEC 3.3o) against its twin
(tests/afsk_diversity_reference.py) on the scenes of tests/afsk_diversity_scenes.py: with groups set the records of every submit are
the twin's over the same batch's records without groups, whole records byte for byte, however the stream is cut, and diversity_info
reports the twin's counters; the combining rule alone equals the twin on caller-made copies; a clean scene does not change; with the
flag and no AFSK group, and without the flag, nothing changes; a packet SPEC 3.3i repaired is a good copy; the refusals hold; a
restarted group starts over; poll() delivers the fields of a combined iMet PTU packet."""
import numpy as np
import pytest
import torch

import afsk_diversity_reference as ad
import afsk_diversity_scenes as ds
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = list(ds.KINDS)
FLAG = getattr(_lib, "FLAG_AFSK_DIVERSITY", 4096)
_dev_cache, _base_cache = {}, {}


def _iq(kind, clean=False):
    key = (kind, clean)
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(ds.scene(kind, clean).iq).to(DEV)
    return _dev_cache[key]


def _types(kind):
    return np.full(ds.scene(kind).C, ds.KINDS[kind][0], dtype=np.uint8)


def _run(iq, steps, groups=None, offsets=None, window=0, keep=False, restart_at=None, flags=FLAG, **kw):
    """the records of each submit, [(channel, bitpos)-sorted arrays]; steps: the submits' lengths in samples"""
    assert sum(steps) == iq.shape[1]
    b = SondeBatch(iq.shape[0], max(steps), flags=flags, **kw)
    if groups is not None:
        b.set_diversity(groups, offsets, window)
    parts, at = [], 0
    for k, step in enumerate(steps):
        if restart_at is not None and k == restart_at[0]:
            b.restart_channels(restart_at[1])
        b.submit(iq[:, at:at + step])
        at += step
        parts.append(ds.sort_records(b.frames()))
    if keep:
        return parts, b
    b.close()
    return parts


def _steps(kind, variant):
    sc = ds.scene(kind)
    if variant == "late_copy":                               # two submits cut between the copies of a packet the plan combines
        first = sc.late_cut_granules * ds.GRANULE
        return [first, sc.n - first]
    cuts = {"1_submit": 1, "4_submits": 4, "finest": sc.n // ds.GRANULE}[variant]
    return [sc.n // cuts] * cuts


def _base(kind, variant):
    if (kind, variant) not in _base_cache:
        _base_cache[(kind, variant)] = _run(_iq(kind), _steps(kind, variant), types=_types(kind))
    return _base_cache[(kind, variant)]


def _twin(parts, sc, restart_at=None):
    state, want = None, []
    for k, sub in enumerate(parts):
        if restart_at is not None and k == restart_at[0] and state is not None:
            for g, members in enumerate(sc.groups):
                if set(members) <= set(restart_at[1]):
                    ad.restart_div_group(state, sc.groups, g)
        w, _, state = ad.diversity(sub, sc.groups, sc.offsets, 0, state)
        want.append(w)
    return want, state


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        for a, e in zip(g, w):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))


@pytest.mark.parametrize("variant", ["1_submit", "4_submits", "finest", "late_copy"])
@pytest.mark.parametrize("kind", KINDS)
def test_with_groups_the_records_are_the_twins(kind, variant):
    sc = ds.scene(kind)
    steps = _steps(kind, variant)
    off = _base(kind, variant)
    want, state = _twin(off, sc)
    got, b = _run(_iq(kind), steps, sc.groups, sc.offsets, 0, keep=True, types=_types(kind))
    _same(got, want)
    assert sum(state["combined"]) >= 12
    assert sum(int((g["flags"] & _lib.FRAME_COMBINED != 0).sum()) for g in got) == sum(state["combined"])
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()
    if variant == "late_copy":       # the second submit combines a packet of the delayed pair whose other copy came with the first
        key = (ds.DELAYED_STREAM, sc.late_cut_packet)
        assert any(ds.frame_of(sc, f) and ds.frame_of(sc, f)[:2] == key and int(f["channel"]) == 2 for f in off[0])
        late = [f for f in got[1] if int(f["flags"]) & _lib.FRAME_COMBINED and int(f["channel"]) == 3 and ds.frame_of(sc, f)[:2] == key]
        assert len(late) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_one_submit_delivers_the_transmitted_packets(kind):
    sc = ds.scene(kind)
    got = _run(_iq(kind), [sc.n], sc.groups, sc.offsets, 0, types=_types(kind))[0]
    comb = got[got["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) >= 12
    seen = set()
    for f in comb:
        _, _, tx = ds.frame_of(sc, f)
        fl = int(f["flags"])
        assert int(f["len"]) == len(tx) and bytes(f["data"][:len(tx)]) == bytes(tx) and int(f["nerr"][0]) == 0 and fl & _lib.FRAME_RESCUED
        seen.add((_lib.frame_copies(fl), _lib.frame_unknowns(fl)))
    assert {2, 3, 4} == {c for c, _ in seen}
    assert {(2, 6), (2, 8), (2, 2), (3, 12), (3, 5), (4, 5)} <= seen


def test_the_combining_rule_alone_equals_the_twin():
    copies, n_copies, names, want = ds.unit_cases()
    b = SondeBatch(1, ds.TILE)
    out, status = b.test_afsk_combine(copies, n_copies)
    b.close()
    seen = set()
    for i, name in enumerate(names):
        w, st = ad.combine(copies[i], n_copies[i])
        assert int(status[i]) == st, (i, name, int(status[i]), st)
        assert want[i] is None or st == want[i], (i, name, st, want[i])
        assert out[i].tobytes() == w.tobytes(), (i, name, st)
        seen.add(st if st < 0 else int(n_copies[i]))
    assert seen == {2, 3, 4, -1, -2, -3}


def test_the_combining_rule_refuses_what_it_cannot_take():
    copies, n_copies, _, _ = ds.unit_cases()
    b = SondeBatch(1, ds.TILE)
    for bad in (1, 5):
        with pytest.raises(SondeError):
            b.test_afsk_combine(copies[:1], np.array([bad]))
    for field, value in (("nerr", 0), ("len", 4), ("len", 65), ("type", 3)):    # a good copy 0; lengths no packet has; a type the rule is not for
        c = copies[:1].copy()
        if field == "nerr":
            c[0, 0]["nerr"] = value
        else:
            c[0, 0][field] = value
        with pytest.raises(SondeError):
            b.test_afsk_combine(c, n_copies[:1])
    c = copies[:1].copy()
    c[0, 1]["len"] = int(c[0, 0]["len"]) + 1                  # copies of differing len
    with pytest.raises(SondeError):
        b.test_afsk_combine(c, n_copies[:1])
    c = copies[:1].copy()
    c[0, 0]["type"], c[0, 0]["len"] = 5, 10                   # a C50 record that is not 9 bytes
    with pytest.raises(SondeError):
        b.test_afsk_combine(c, n_copies[:1])
    c = copies[:1].copy()
    c[0, 1]["type"] = 5                                       # copies of differing type
    with pytest.raises(SondeError):
        b.test_afsk_combine(c, n_copies[:1])
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_clean_scene_is_unchanged(kind):
    sc = ds.scene(kind, clean=True)
    steps = [sc.n // 2] * 2
    off = _run(_iq(kind, True), steps, types=_types(kind))
    on, b = _run(_iq(kind, True), steps, sc.groups, sc.offsets, 0, keep=True, types=_types(kind))
    assert sum(len(p) for p in off) > 100
    _same(on, off)
    assert all(b.diversity_info(g) == {"tried": 0, "combined": 0} for g in range(len(sc.groups)))
    b.close()


def _mixed():
    """the first two pairs of each AFSK scene next to each other, cut to the shorter scene"""
    n = min(ds.scene("imet").n, ds.scene("c50").n)
    iq = torch.cat([_iq("imet")[:4, :n], _iq("c50")[:4, :n]]).contiguous()
    return iq, np.array([4] * 4 + [5] * 4, dtype=np.uint8), n


def test_with_the_flag_and_no_group_and_without_the_flag_nothing_changes():
    iq, types, n = _mixed()
    steps = [n // 2] * 2
    witness = _run(iq, steps, types=types, flags=0)
    _same(_run(iq, steps, types=types, flags=FLAG), witness)
    # and with groups the flag is what admits them: the same groups change records
    on = _run(iq, steps, [[0, 1], [4, 5]], None, 0, types=types, flags=FLAG)
    changed = sum(a.tobytes() != e.tobytes() for g, w in zip(on, witness) for a, e in zip(g, w))
    assert changed >= 4
    b = SondeBatch(8, n, types=types, flags=0)
    with pytest.raises(SondeError, match="SONDE_MRZN1 or SONDE_DFM09"):      # the parent's words
        b.set_diversity([[0, 1]])
    b.close()


def test_a_packet_the_afsk_rescue_repaired_is_a_good_copy():
    """ds.rescued_partner_scene: in every other damaged packet receiver 0 fails with two separated wrong bits (SPEC 3.3i has no pattern
    for them) while receiver 1's one wrong bit is repaired -- the failed copy meets a repaired partner, a good copy: it stays as
    recorded and nothing is tried.  In the packets between, both copies stay failed and the pass combines them."""
    sc = ds.rescued_partner_scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    types = np.full(2, 4, dtype=np.uint8)
    fl = FLAG | _lib.FLAG_AFSK_RESCUE
    off = _run(iq, [sc.n], types=types, flags=fl)[0]
    on, b = _run(iq, [sc.n], sc.groups, None, 0, keep=True, types=types, flags=fl)
    want, outcomes, state = ad.diversity(off, sc.groups, None, 0)
    _same(on, [want])
    n_rescued = n_both = 0
    for f, o, out in zip(off, on[0], outcomes):
        hit = ds.frame_of(sc, f)
        if hit is None:
            continue
        ch, case = int(f["channel"]), sc.plan[hit[1]]
        if case == "rescued_partner":
            if ch == 0:
                n_rescued += 1
                assert int(f["nerr"][0]) < 0 and out == "partner_good" and o.tobytes() == f.tobytes(), hit[1]
            else:
                assert int(f["flags"]) & _lib.FRAME_RESCUED and int(f["nerr"][0]) == 0 and out == "good" and o.tobytes() == f.tobytes(), hit[1]
        elif case == "both_failed":
            n_both += ch == 0
            assert int(f["nerr"][0]) < 0 and out == ("combined" if ch == 0 else "partner_good"), (hit[1], ch, out)
            if ch == 0:
                assert int(o["flags"]) & _lib.FRAME_COMBINED and bytes(o["data"][:len(hit[2])]) == bytes(hit[2]), hit[1]
    assert n_rescued >= 2 and n_both >= 2
    assert b.diversity_info(0) == {"tried": n_both, "combined": n_both} == {"tried": state["tried"][0], "combined": state["combined"][0]}
    b.close()
    # with the rescue pass off the partner of the first kind of packet stays failed, and the pass combines those packets too
    plain = _run(iq, [sc.n], sc.groups, None, 0, types=types, flags=FLAG)[0]
    assert (plain["flags"] & _lib.FRAME_COMBINED != 0).sum() == n_rescued + n_both


def test_the_refusals():
    types = np.array([4, 4, 5, 5, 0, 0, 3, 3, 4, 5], dtype=np.uint8)

    def batch(flags=FLAG):
        return SondeBatch(10, ds.GRANULE, types=types, flags=flags)

    b = batch(0)                                              # no flag: the parent's words
    with pytest.raises(SondeError, match="a member that is not SONDE_RS41, SONDE_M10, SONDE_MRZN1 or SONDE_DFM09"):
        b.set_diversity([[0, 1]])
    with pytest.raises(SondeError, match="a member that is not SONDE_RS41, SONDE_M10, SONDE_MRZN1 or SONDE_DFM09"):
        b.set_diversity([[2, 3]])
    b.close()
    for fl in (_lib.FLAG_LATE_JOIN, _lib.FLAG_PIPELINE):
        b = batch(FLAG | fl)
        with pytest.raises(SondeError):
            b.set_diversity([[0, 1]])
        b.close()
    # iMet + C50 in one group; AFSK + another type; the window with and without a C50 group
    for groups, window in (([[0, 2]], 0), ([[1, 9]], 0), ([[0, 4]], 0), ([[2, 6]], 0), ([[0, 1, 6]], 0), ([[2, 3]], 45), ([[0, 1], [2, 3]], 45),
                           ([[0, 1]], 1201), ([[0]], 0)):
        b = batch()
        with pytest.raises(SondeError):
            b.set_diversity(groups, None, window)
        b.close()
    for kw in (dict(learn=True), dict(mark_duplicates=True), dict(learn=True, mark_duplicates=True)):      # any mode bit with a C50 group
        b = batch()
        with pytest.raises(SondeError, match="C50"):
            b.set_diversity([[0, 1], [2, 3]], None, 0, **kw)
        b.close()
    b = batch()
    b.set_diversity([[0, 1], [2, 3], [4, 5], [6, 7]], None, 44)           # what is taken: 44 with a C50 group, next to the other kinds
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                                          # a second call
    b.close()
    b = batch()
    b.set_diversity([[0, 1, 8]], None, 1200, learn=True, mark_duplicates=True)      # iMet groups alone: the window of the call, both mode bits
    b.close()


def test_refused_behind_a_channelizer():
    from sdrpp_radiosonde_amd.batch import SondeChannelizer
    ch = SondeChannelizer(types=np.full(512, 0, dtype=np.uint8))         # whatever its bins hold: the refusal comes first
    with pytest.raises(SondeError, match="channelizer"):
        ch.batch.set_diversity([[0, 1]])
    ch.close()


def test_restart_takes_whole_groups_and_clears_them():
    sc = ds.scene("imet")
    steps = [ds.GRANULE] * (sc.n // ds.GRANULE)
    b = SondeBatch(sc.C, steps[0], types=_types("imet"), flags=FLAG)
    b.set_diversity(sc.groups, sc.offsets, 0)
    b.submit(_iq("imet")[:, :steps[0]])
    for part in ([0], [6, 7], [0, 1, 2]):
        with pytest.raises(SondeError):
            b.restart_channels(part)
    b.restart_channels([9])                                  # a channel in no group: as before
    b.close()
    # the first pair, the triple and the ungrouped channel restart behind the fourth of eight submits
    restart = (4, [0, 1, 6, 7, 8, 9])
    off = _run(_iq("imet"), steps, restart_at=restart, types=_types("imet"))
    want, state = _twin(off, sc, restart)
    on, b = _run(_iq("imet"), steps, sc.groups, sc.offsets, 0, keep=True, restart_at=restart, types=_types("imet"))
    _same(on, want)
    _, st_whole = _twin(_base("imet", "finest"), sc)
    # (a restarted channel's demodulator settles anew, so the restarted groups can only lose packets; the pair left alone loses none)
    assert state["combined"][0] <= st_whole["combined"][0] and state["combined"][2] == st_whole["combined"][2] >= 2
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()


def test_poll_delivers_the_fields_of_a_combined_imet_ptu_packet():
    sc = ds.scene("imet")
    seqs = {}
    for on in (False, True):
        b = SondeBatch(sc.C, sc.n, types=_types("imet"), flags=FLAG)
        if on:
            b.set_diversity(sc.groups, sc.offsets, 0)
        b.submit(_iq("imet"))
        fr = ds.sort_records(b.frames())
        seqs[on] = sorted((ch, int(d.seq)) for ch, d in b.poll() if d.fields & _lib.DATA_PTU)
        b.close()
    comb = fr[(fr["flags"] & _lib.FRAME_COMBINED != 0) & (fr["len"] == 14)]
    assert len(comb) >= 3
    # a PTU packet (01 01 <packet number, u16> ...) reports its number as SondeData.seq: the combined ones are delivered, only with groups
    new = sorted((int(f["channel"]), int(f["data"][2]) | int(f["data"][3]) << 8) for f in comb)
    rest = list(seqs[True])
    for x in seqs[False]:
        rest.remove(x)
    assert sorted(rest) == new
