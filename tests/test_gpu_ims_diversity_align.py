"""-m gpu: the align step of sonde_batch_set_diversity_auto for iMS-100 groups (DESIGN SPEC 3.3k with the predicates of SPEC 3.3n) against its
twin (ims_diversity_reference.align / run): with learn=True and no offsets the members of the scene's groups -- the triple 0, 300 and
2700 chips late, the last pair with no wrong offset to mislead it -- lock at the first frame that is good in two members and combine
from then on, the duplicates are the twin's, diversity_offsets is the twin's state; the align step alone, with the iMS-100 predicates,
equals the twin on caller-made 51-byte records (sonde_batch_test_diversity_align_kind); and DiversityReceiver(ims_diversity=True) with an
RS41 and an iMS-100 sonde on two antennas' wideband streams, one of them two granules late, delivers frames no single antenna
delivers, none of them wrong."""
import numpy as np
import pytest
import torch

import diversity_align_scenes as das
import ims_diversity_reference as cr
import ims_diversity_scenes as cs
import ims_rescue_scenes as isc
from sdrpp_radiosonde_amd import _chain, _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE = cr.LEARN | cr.MARK


@pytest.mark.parametrize("cuts", [1, 2])
def test_members_lock_at_the_twins_submit_and_combine_from_then_on(cuts):
    sc = cs.scene(align=True)
    iq = torch.from_numpy(sc.iq).to(DEV)
    step = sc.n // cuts
    types = np.full(sc.C, sc.type, dtype=np.uint8)
    b0 = SondeBatch(sc.C, step, types=types)
    b = SondeBatch(sc.C, step, types=types, flags=_lib.FLAG_IMS_DIVERSITY)
    b.set_diversity(sc.groups, None, sc.window, learn=True, mark_duplicates=True)
    state = cr.new_state(sc.groups, None, MODE)
    on = []
    for k in range(cuts):
        for x in (b0, b):
            x.submit(iq[:, k * step:(k + 1) * step])
        sub, got = cs.sort_records(b0.frames()), cs.sort_records(b.frames())
        want, _, state = cr.run(sub, sc.groups, cs.ring_chips(b0), state, MODE, sc.window)
        assert len(got) == len(want), k
        for a, e in zip(got, want):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), hex(int(a["flags"])), hex(int(e["flags"])))
        if k == 0:                   # every group has a frame good in two members in the first submit: all lock there
            assert all(b.diversity_offsets(g)["locked"] == (1 << len(m)) - 1 for g, m in enumerate(sc.groups))
        on.append(got)
    b0.close()
    assert all(state["locked"][ch] for members in sc.groups for ch in members)
    a = np.concatenate(on)
    assert (a["flags"] & _lib.FRAME_DUPLICATE != 0).sum() == sum(state["duplicates"]) >= 40
    for g, members in enumerate(sc.groups):
        o = b.diversity_offsets(g)
        assert o["offsets"][:len(members)] == [state["off"][ch] for ch in members], g
        assert o["locked"] == (1 << len(members)) - 1 and o["learned"] == state["learned"][g] and o["duplicates"] == state["duplicates"][g], (g, o)
        assert b.diversity_info(g) == {"tried": state["div"]["tried"][g], "combined": state["div"]["combined"][g]}, g
        for ch in members[1:]:       # the learned offsets are the true delays, to the chip
            assert abs(o["offsets"][members.index(ch)] - o["offsets"][0] - (sc.sonde[ch][1] - sc.sonde[members[0]][1])) <= 1, (g, ch)
    assert state["div"]["combined"][2] >= 4 and state["div"]["combined"][cs.WRONG_GROUP] >= 4
    comb = a[a["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) == sum(state["div"]["combined"]) >= 25
    for f in comb:
        s, k, tx = cs.frame_of(sc, f)
        assert bytes(f["data"][:51]) == bytes(tx) or sc.plan[(s, k)][0] == "dist6"
    b.close()


def test_the_align_step_alone_with_the_ims100_predicates_equals_the_twin():
    """caller-made records of 51 bytes: the quick-reject key (words 11 and 12, three bytes of the latter) and the byte compare behind
    it, a jump followed, every pair order under every lock state, the mode bits; and the same cases under the RS41 predicates (the
    older entry) find no good record at all"""
    cases = cs.align_unit_cases()
    records, counts, nm, carried, off, locked, mode = das.pack_cases(cases)
    assert records.shape[2] == 70 and set(nm.tolist()) == {2, 3, 4} and set(mode.tolist()) == {0, 1, 2, 3}
    b = SondeBatch(1, cs.TILE)
    rec, o, lk, learned, dups = b.test_diversity_align(records, counts, nm, carried, off, locked, mode, kind=cs.IMS)
    for k, c in enumerate(cases):
        per, woff, wlk, wle, wdu = cs.twin_align_case(c)
        assert ([int(v) for v in o[k]], int(lk[k]), int(learned[k]), int(dups[k])) == (woff, wlk, wle, wdu), c["name"]
        for m, p in enumerate(per):
            assert rec[k, m, :len(p)].tobytes() == p.tobytes(), (c["name"], m)
    assert int(dups.sum()) > 50 and int(learned.sum()) > 50
    by_name = {c["name"]: k for k, c in enumerate(cases)}
    for name in ("same_key_byte_0_differs", "same_key_byte_43_differs", "same_key_words_0_to_10_differ", "byte_44_differs", "byte_47_differs",
                 "byte_48_differs", "last_byte_differs", "same_bytes_other_len"):
        assert int(lk[by_name[name]]) == 0 and int(dups[by_name[name]]) == 0, name
    for name in ("byte_behind_the_frame_differs_and_matches", "bytes_behind_the_frame_differ_in_the_carried"):
        assert int(lk[by_name[name]]) == 3 and int(dups[by_name[name]]) == 1, name
    k = by_name["a_jump_is_followed"]
    assert [int(v) for v in o[k][:2]] == [0, 467] and int(learned[k]) == 1
    # the older entry (RS41 predicates) and kind = SONDE_RS41 are one: a 51-byte record is no RS41 frame, nothing is learned or marked
    for kw in (dict(), dict(kind=0)):
        rec0, o0, lk0, le0, du0 = b.test_diversity_align(records, counts, nm, carried, off, locked, mode, **kw)
        assert rec0.tobytes() == records.tobytes() and (o0 == off).all() and (lk0 == locked).all() and not le0.any() and not du0.any()
    for bad in (4, 5, 7):            # iMet, C50, no type: no group has such a kind
        with pytest.raises(SondeError, match="kind"):
            b.test_diversity_align(records[:1], counts[:1], nm[:1], carried[:1], off[:1], locked[:1], mode[:1], kind=bad)
    b.close()


def test_diversity_receiver_with_an_rs41_and_an_ims100_sonde_on_two_antennas():
    """two sondes in one wideband stream heard on two antennas, antenna 1 two granules late.  In every other iMS-100 frame each antenna
    has three wrong bits in a block of its own (chips flipped before the modulator): neither antenna delivers the frame, the receiver
    does.  What the receiver delivers is also what a batch delivers that is fed the receiver's own tuners' rows by hand with the same
    groups"""
    from sdrpp_radiosonde_amd.diversity import DiversityReceiver
    fs, sondes = 2_400_000, [(200_000, 0), (-350_000, 2)]
    for bad in (dict(), dict(dfm_diversity=True), dict(ims_rescue=True), dict(ims_diversity=True, afsk_rescue=True),
                dict(ims_diversity=True, sondes=sondes + [(0, 1)])):
        with pytest.raises(SondeError):
            DiversityReceiver(fs, bad.pop("sondes", sondes), **bad)
    with pytest.raises(SondeError, match="RS41 sondes only"):
        DiversityReceiver(fs, sondes)
    kw = dict(antennas=2, max_in=20 * 102_400, ims_diversity=True)
    rx = DiversityReceiver(fs, sondes, ims_rescue=True, **kw)               # ims_rescue= is passed on to the batch
    assert rx.batch.flags & _lib.FLAG_IMS_DIVERSITY and rx.batch.flags & _lib.FLAG_IMS_RESCUE
    rx.close()
    rx = DiversityReceiver(fs, sondes, **kw)                               # without it here: the flipped chips would be SPEC 3.3h's to repair
    assert rx.batch.flags & _lib.FLAG_IMS_DIVERSITY and not rx.batch.flags & _lib.FLAG_IMS_RESCUE
    n, delay = 80 * rx.granule, 2 * rx.granule
    nsym = int(n * synth.SCENE_BAUD[2] / fs) + 16
    rows, frames = synth.chip_streams(2, 31, np.arange(1), nsym)
    rng = np.random.default_rng(31)
    damaged, chips = [], [rows[0].copy(), rows[0].copy()]
    for k, (pos, tx) in enumerate(frames[0]):
        if k % 2 == 1 and pos + cs.FRAME_CHIPS + 64 <= nsym - int(delay * synth.SCENE_BAUD[2] / fs):
            dmg = cs.place("r_only", rng, tx[:51])
            for a in range(2):
                isc._apply(chips[a], pos, [(c, "a") for c in dmg[a]])
            damaged.append(bytes(tx[:51]))
    ants = []
    for a in range(2):
        iq, _, _ = synth.make_wideband_scene(sondes, n, fs=fs, ebn0_db=25.0, seed=5, device=DEV, bits=[None, chips[a]])
        ants.append(iq)
    ants[1] = torch.cat([torch.zeros_like(ants[1][:delay]), ants[1][:n - delay]]).contiguous()
    S, K = len(sondes), 2
    types = [t for _, t in sondes] * K
    n48 = _chain.plan(fs, [t for _, t in sondes], kw["max_in"]).n48
    hand = _chain.batch(K * S, n48, types, 0, (False,) * 5, flags=_lib.FLAG_IMS_DIVERSITY)
    hand.set_diversity([[a * S + i for a in range(K)] for i in range(S)], None, 0, learn=True, mark_duplicates=True)
    single = _chain.batch(K * S, n48, types, 0, (False,) * 5)              # the antennas on their own
    got, want, alone = [], [], []
    for a in range(0, n, rx.max_in):
        rx.submit([ants[0][a:a + rx.max_in], ants[1][a:a + rx.max_in]])
        got.append(rx.frames()[0])
        for x in (hand, single):
            x.submit(rx._rows[:, :rx._n48].clone())
        f = hand.frames()
        f = f[(f["flags"] & _lib.FRAME_DUPLICATE) == 0]
        f["channel"] %= S
        want.append(f)
        alone.append(single.frames())
    got, want, alone = np.concatenate(got), np.concatenate(want), np.concatenate(alone)
    assert got.tobytes() == want.tobytes()
    for i in range(S):
        o = rx.offsets(i)
        assert o == hand.diversity_offsets(i) and o["locked"] == 3 and o["learned"] >= 1, (i, o)
    sent = {bytes(np.asarray(tx)[:51]) for _, tx in frames[0]}
    ims = got[(got["channel"] == 1) & (got["nerr"][:, 1] == 0)]
    seen = [bytes(r["data"][:51]) for r in ims]
    assert len(set(seen)) == len(seen) and set(seen) <= sent             # one record per transmitted frame, none of them wrong
    by_one = {bytes(r["data"][:51]) for r in alone[(alone["type"] == 2) & (alone["nerr"][:, 1] == 0)]}
    comb = {bytes(r["data"][:51]) for r in ims if int(r["flags"]) & _lib.FRAME_COMBINED}
    assert len(comb) >= 3 and comb <= set(damaged) and not comb & by_one   # frames no single antenna delivers
    assert set(seen) == by_one | comb
    rs = got[(got["channel"] == 0) & (got["nerr"][:, 0] >= 0) & (got["nerr"][:, 1] >= 0)]
    assert len(rs) >= 3 and (rs["type"] == 0).all()
    for x in (hand, single, rx):
        x.close()
