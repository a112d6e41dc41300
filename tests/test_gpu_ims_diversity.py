"""-m gpu: sonde_batch_set_diversity on iMS-100 groups (SONDE_FLAG_IMS_DIVERSITY, DESIGN SPEC 3.3n) against its twin
(tests/ims_diversity_reference.py) on the scenes of tests/ims_diversity_scenes.py: with groups set the records of every submit are the
twin's over the records of the same batch without groups and the chips its bit rings hold at that moment, whole records byte for
byte, however the stream is cut, and diversity_info reports the twin's counters; the combining rule alone equals the twin on
caller-made block sets; with the flag and no iMS-100 group every record is what it is without the flag; without the flag an iMS-100
pair is refused, and with it everything else stays refused; a restarted group starts over; a frame SPEC 3.3h rescued is a good copy;
a group whose offset is wrong by one frame changes nothing; a partner whose chips are no longer held is left out; beyond 2^32 chips the records are the unaged run's with bitpos shifted."""
import numpy as np
import pytest
import torch

import age_scenes as A
import demod_reference as D
import diversity_scenes as ds
import ims_diversity_reference as cr
import ims_diversity_scenes as cs
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeChannelizer, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAG = _lib.FLAG_IMS_DIVERSITY
_dev_cache = {}


def _iq(clean=False):
    if clean not in _dev_cache:
        _dev_cache[clean] = torch.from_numpy(cs.scene(clean).iq).to(DEV)
    return _dev_cache[clean]


def _types(C=None):
    return np.full(cs.scene().C if C is None else C, cs.IMS, dtype=np.uint8)


def _both(iq, steps, groups, offsets, window=0, restart_at=None, flags=0, types=None, keep=False, **mut):
    """the scene through a batch without groups and one with them, submit by submit; behind every submit the twin runs over the first
    batch's records and ring chips.  Returns (records without groups, records with groups, the twin's records, the twin's state)."""
    assert sum(steps) == iq.shape[1]
    types = _types(iq.shape[0]) if types is None else types
    b0 = SondeBatch(iq.shape[0], max(steps), types=types, flags=flags)
    b = SondeBatch(iq.shape[0], max(steps), types=types, flags=flags | FLAG)
    b.set_diversity(groups, offsets, window)
    off, on, want, state, at = [], [], [], None, 0
    for k, step in enumerate(steps):
        if restart_at is not None and k == restart_at[0]:
            for x in (b0, b):
                x.restart_channels(restart_at[1])
            for g, members in enumerate(groups):
                if state is not None and set(members) <= set(restart_at[1]):
                    cr.restart_div_group(state, groups, g)
        for x in (b0, b):
            x.submit(iq[:, at:at + step])
        at += step
        off.append(cs.sort_records(b0.frames()))
        on.append(cs.sort_records(b.frames()))
        w, _, state = cr.diversity(off[-1], groups, cs.ring_chips(b0), offsets, window or cr.WINDOW, state, **mut)
        want.append(w)
    b0.close()
    if keep:
        return off, on, want, state, b
    b.close()
    return off, on, want, state


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        for a, e in zip(g, w):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))


def _steps(variant):
    sc = cs.scene()
    if variant == "late_copy":                               # two submits cut between the copies of a frame the plan combines
        first = cs.late_cut_tiles(sc) * cs.TILE
        return [first, sc.n - first]
    return [t * cs.TILE for t in {"1_submit": [100], "3_submits": [34, 33, 33], "5_submits": [20] * 5, "9_submits": [12] * 8 + [4]}[variant]]


@pytest.mark.parametrize("variant", ["1_submit", "3_submits", "5_submits", "9_submits", "late_copy"])
def test_with_groups_the_records_are_the_twins(variant):
    sc = cs.scene()
    off, on, want, state, b = _both(_iq(), _steps(variant), sc.groups, sc.offsets, sc.window, keep=True)
    _same(on, want)
    planned = sum(1 for _, e in sc.plan.values() if e in ("combined", "miscorrected"))
    assert sum(state["combined"]) == planned >= 25
    assert sum(int((g["flags"] & _lib.FRAME_COMBINED != 0).sum()) for g in on) == planned
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    assert state["combined"][cs.WRONG_GROUP] == 0 and state["tried"][cs.WRONG_GROUP] >= 16      # one frame off: the guard refuses every frame
    b.close()
    if variant == "late_copy":       # the second submit combines a frame of the delayed pair whose other copy came with the first
        firsts = {cs.frame_of(sc, f)[:2] for f in off[0] if int(f["channel"]) == 2}
        late = [f for f in on[1] if int(f["flags"]) & _lib.FRAME_COMBINED and int(f["channel"]) == 3 and cs.frame_of(sc, f)[:2] in firsts]
        assert len(late) >= 1


def test_one_submit_delivers_the_transmitted_frames():
    sc = cs.scene()
    _, on, _, _ = _both(_iq(), [sc.n], sc.groups, sc.offsets, sc.window)
    got = on[0]
    comb = got[got["flags"] & _lib.FRAME_COMBINED != 0]
    seen = set()
    for f in comb:
        s, k, tx = cs.frame_of(sc, f)
        fl = int(f["flags"])
        assert int(f["nerr"][1]) == 0 and int(f["nerr"][0]) >= 3 and fl & _lib.FRAME_RESCUED
        assert bytes(f["data"][:51]) == bytes(tx) or sc.plan[(s, k)][0] == "dist6"
        seen.add((_lib.frame_copies(fl), _lib.frame_joint(fl)))
    assert seen == {(2, 0), (2, 1), (3, 0), (3, 1), (4, 1)}


def test_the_combining_rule_alone_equals_the_twin():
    records, n_copies, blocks, names, want = cs.unit_cases()
    b = SondeBatch(1, cs.TILE)
    out, status = b.test_ims_combine(records, n_copies, blocks)
    b.close()
    seen = set()
    for i, name in enumerate(names):
        w, st = cs.twin_unit(records, n_copies, blocks, i)
        assert int(status[i]) == st, (i, name, int(status[i]), st)
        assert want[i] is None or st == want[i], (i, name, st, want[i])
        assert out[i].tobytes() == w.tobytes(), (i, name, st)
        seen.add(st)
    assert seen == {2, 3, 4, 0, -1, -2, -3}


def test_the_combining_rule_refuses_what_it_cannot_take():
    records, n_copies, blocks, _, _ = cs.unit_cases()
    b = SondeBatch(1, cs.TILE)
    for bad in (0, 1, 5):
        with pytest.raises(SondeError, match="n_copies"):
            b.test_ims_combine(records[:1], np.array([bad]), blocks[:1])
    for field, value in (("nerr", 0), ("len", 33), ("type", 1)):       # a good copy 0; another length; another type
        r = records[:1].copy()
        if field == "nerr":
            r[0]["nerr"][1] = value
        else:
            r[0][field] = value
        with pytest.raises(SondeError):
            b.test_ims_combine(r, n_copies[:1], blocks[:1])
    b.test_ims_combine(records[:1], n_copies[:1], blocks[:1])
    b.close()


def test_with_the_flag_and_no_ims_group_every_record_is_what_it_is_without():
    sc = cs.scene()

    def run(iq, flags, groups=None, offsets=None, **kw):
        b = SondeBatch(iq.shape[0], iq.shape[1] // 2, flags=flags, **kw)
        if groups is not None:
            b.set_diversity(groups, offsets)
        parts = []
        for k in range(2):
            b.submit(iq[:, k * (iq.shape[1] // 2):(k + 1) * (iq.shape[1] // 2)])
            parts.append(cs.sort_records(b.frames()))
        b.close()
        return np.concatenate(parts)

    # the flag set and set_diversity never called: the damaged iMS-100 scene
    plain = run(_iq(), 0, types=_types())
    assert run(_iq(), FLAG, types=_types()).tobytes() == plain.tobytes() and (plain["nerr"][:, 1] > 0).sum() >= 60
    # the flag set and RS41 groups only: the RS41 diversity scene with its groups
    rs = ds.scene()
    rs_iq = torch.from_numpy(rs.iq).to(DEV)
    without = run(rs_iq, 0, rs.groups, rs.offsets)
    assert run(rs_iq, FLAG, rs.groups, rs.offsets).tobytes() == without.tobytes()
    assert (without["flags"] & _lib.FRAME_COMBINED != 0).sum() >= 2


def test_the_refusals():
    types = np.array([2, 2, 1, 1, 2, 2, 2, 2, 2, 0, 4, 5], dtype=np.uint8)

    def batch(flags=FLAG):
        return SondeBatch(12, cs.TILE * 8, types=types, flags=flags)

    b = batch(0)                                              # without the flag an iMS-100 pair is refused, in the parent's words
    with pytest.raises(SondeError, match="SONDE_MRZN1 or SONDE_DFM09"):
        b.set_diversity([[0, 1]])
    b.close()
    for flags in (FLAG | _lib.FLAG_LATE_JOIN, FLAG | _lib.FLAG_PIPELINE):
        b = batch(flags)
        with pytest.raises(SondeError, match="LATE_JOIN"):
            b.set_diversity([[0, 1]])
        b.close()
    # iMS-100 + DFM; iMS-100 + RS41; iMS-100 + iMet; iMS-100 + C50; five members; one member; the window; a gap
    for groups, window in (([[0, 2]], 0), ([[0, 9]], 0), ([[0, 10]], 0), ([[0, 11]], 0), ([[0, 1, 4, 5, 6]], 0), ([[0]], 0), ([[0, 1]], 1201),
                           ([[0, 1], [], [4, 5]], 0)):
        b = batch()
        with pytest.raises(SondeError):
            b.set_diversity(groups, None, window)
        b.close()
    b = batch()
    gid = np.full(12, -1, dtype=np.int32)
    gid[[0, 1]] = 0
    assert b.L.sonde_batch_set_diversity_auto(b.h, gid.ctypes.data, None, 0, 4) < 0        # mode bits 4 and 8 stay unknown
    assert b.L.sonde_batch_set_diversity_auto(b.h, gid.ctypes.data, None, 0, 8) < 0
    b.set_diversity([[0, 1], [2, 3], [4, 5, 6, 7]], None, 1200)                            # iMS-100 groups next to a DFM group
    with pytest.raises(SondeError):
        b.set_diversity([[0, 1]])                                                         # a second call
    b.close()
    ch = SondeChannelizer(types=np.full(512, cs.IMS, dtype=np.uint8))
    with pytest.raises(SondeError, match="channelizer"):
        ch.batch.set_diversity([[0, 1]])
    ch.close()


def test_restart_takes_whole_groups_and_clears_them():
    sc = cs.scene()
    steps = [20 * cs.TILE] * 5
    b = SondeBatch(sc.C, steps[0], types=_types(), flags=FLAG)
    b.set_diversity(sc.groups, sc.offsets, sc.window)
    b.submit(_iq()[:, :steps[0]])
    for part in ([0], [4, 5], [0, 1, 2]):
        with pytest.raises(SondeError, match="all members"):
            b.restart_channels(part)
    b.restart_channels([7])                                  # a channel in no group: as before
    b.close()
    # the first pair, the triple and the ungrouped channel restart behind the second of five submits
    restart = (2, [0, 1, 4, 5, 6, 7])
    _, on, want, state, b = _both(_iq(), steps, sc.groups, sc.offsets, sc.window, restart_at=restart, keep=True)
    _same(on, want)
    _, _, _, whole = _both(_iq(), steps, sc.groups, sc.offsets, sc.window)
    assert state["combined"][0] < whole["combined"][0] and state["combined"][1] == whole["combined"][1] >= 4
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == {"tried": state["tried"][g], "combined": state["combined"][g]}, g
    b.close()


def test_a_frame_the_ims_rescue_completed_is_a_good_copy():
    """cs.rescued_partner_scene: in every other damaged frame receiver 0 fails with nothing SPEC 3.3h could go on while receiver 1's
    copy is one SPEC 3.3h rescues -- the failed copy meets a rescued partner, which is a good copy: it stays as recorded and nothing is
    tried.  In the frames between, both copies stay failed and the pass combines them."""
    sc = cs.rescued_partner_scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    off, on, want, state, b = _both(iq, [sc.n], sc.groups, None, 0, flags=_lib.FLAG_IMS_RESCUE, keep=True)
    _same(on, want)
    n_rescued = n_hidden = 0
    for f, o in zip(off[0], on[0]):
        k = cs.frame_of(sc, f)[1]
        ch, case = int(f["channel"]), sc.plan[k]
        if case == "rescued_partner":
            n_rescued += ch == 0
            assert o.tobytes() == f.tobytes(), k
            assert int(f["nerr"][1]) > 0 if ch == 0 else (int(f["flags"]) & _lib.FRAME_RESCUED and int(f["nerr"][1]) == 0), (k, ch)
        elif case == "both_hidden":
            n_hidden += ch == 0
            assert int(f["nerr"][1]) > 0 and not int(f["flags"]) & _lib.FRAME_RESCUED, (k, ch)
            if ch == 0:
                assert int(o["flags"]) & _lib.FRAME_COMBINED and bytes(o["data"][:51]) == bytes(cs.frame_of(sc, f)[2]), k
    assert n_rescued >= 3 and n_hidden >= 3
    assert b.diversity_info(0) == {"tried": n_hidden, "combined": n_hidden} == {"tried": state["tried"][0], "combined": state["combined"][0]}
    b.close()


def test_a_partner_whose_chips_are_no_longer_held_is_left_out():
    """cs.left_out_scene: the visited copy has two failed partners, the first of them a carried record 9000 chips old in a ring of 8192.
    Step 3 leaves that one out (the twin is refused the chips by sonde_batch_read_bits) and the frame is combined from members 1 and 2
    of the three: SONDE_FRAME_COPIES = 2 in a triple."""
    sc = cs.left_out_scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    steps = [sc.step] * (sc.n // sc.step)
    types = _types(sc.C)
    b0 = SondeBatch(sc.C, sc.step, types=types)
    b = SondeBatch(sc.C, sc.step, types=types, flags=FLAG)
    b.set_diversity(sc.groups, sc.offsets, sc.window)
    refused, state, seen = [], None, []
    for k in range(len(steps)):
        for x in (b0, b):
            x.submit(iq[:, k * sc.step:(k + 1) * sc.step])
        off, on = cs.sort_records(b0.frames()), cs.sort_records(b.frames())
        ring = cs.ring_chips(b0)

        def chips(channel, start, count):
            got = ring(channel, start, count)
            if got is None:
                refused.append((k, channel, start))
            return got

        want, outcomes, state = cr.diversity(off, sc.groups, chips, sc.offsets, sc.window, state)
        _same([on], [want])
        seen += [(int(f["channel"]), o, cr.copies_of(w["flags"])) for f, o, w in zip(off, outcomes, want) if o not in ("other", "good")]
    p1 = sc.stream_frames[0][1][0]
    assert [(ch, abs(start - p1) < 64) for _, ch, start in refused] == [(0, True)]            # receiver 0's record of frame 1, asked for once
    # receiver 0's copy finds no partner yet; receiver 1's is combined from itself and receiver 2's; receiver 2's then finds it good
    assert seen == [(0, "no_partner", 0), (1, "combined", 2), (2, "partner_good", 0)], seen
    assert b.diversity_info(0) == {"tried": 1, "combined": 1} == {"tried": state["tried"][0], "combined": state["combined"][0]}
    b0.close()
    b.close()


@pytest.mark.parametrize("mode", ["offsets", "learn_mark"])
def test_ims_groups_beyond_two_to_the_32_chips(mode):
    """the scene in ten submits, every member's origin moved past 2^32 chips by sonde_batch_test_shift_age once a pair, the triple and the
    quad have each combined a frame (carried records exist and must move; the partners' ring reads are 64-bit chip arithmetic): the
    records equal the unaged run's with bitpos shifted, byte for byte, and so do the counters and offsets"""
    sc = cs.scene()
    iq, C, cuts, boundary = _iq(), sc.C, 10, 1 << 32
    step = sc.n // cuts
    ring = A.ring_bits_of([D.modem(sc.type)], step)
    kw = dict(offsets=sc.offsets) if mode == "offsets" else dict(offsets=None, learn=True, mark_duplicates=True)

    def run(shift_after=None):
        b = SondeBatch(C, step, types=_types(), flags=FLAG)
        b.set_diversity(sc.groups, window_bits=sc.window, **kw)
        parts, added = [], 0
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            parts.append((b.frames(), [added] * C))
            if k == shift_after:
                turns = A.turns_below(boundary, max(b.nbits(c) for c in range(C)), ring)
                got = b.test_shift_age(np.arange(C), [0] * C, [turns] * C)
                assert all(int(g) == turns * ring for g in got)
                added = turns * ring
        return b, parts, added

    a, pa, _ = run()
    comb = [{int(c) for c in f["channel"][f["flags"] & _lib.FRAME_COMBINED != 0]} for f, _ in pa]
    sizes = {len(g): {c for h in sc.groups if len(h) == len(g) for c in h} for g in sc.groups}
    k0 = next(k for k in range(cuts) if all(any(c in members for s in comb[:k + 1] for c in s) for members in sizes.values()))
    assert sum(len(s) for s in comb[k0 + 1:]) >= 8, "too few frames are combined behind the shift"
    b, pb, added = run(shift_after=k0)
    for k, ((fa, _), (fb, add)) in enumerate(zip(pa, pb)):
        why = A.frames_diff(fa, fb, add)
        assert not why, (k, why[:3])
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == a.diversity_info(g), g
        assert b.diversity_offsets(g) == a.diversity_offsets(g), g
    for c in range(C):
        assert b.nbits(c) == a.nbits(c) + added > boundary, c
    a.close()
    b.close()
