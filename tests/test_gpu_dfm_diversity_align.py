"""-m gpu: the align step of sonde_batch_set_diversity_auto for DFM groups (DESIGN SPEC 3.3k with the predicates of SPEC 3.3m) against its
twin (dfm_diversity_reference.align / run): with learn=True and no offsets the members of the scene's groups -- the triple 0, 300 and
5000 chips late -- lock at the twin's submit and combine from then on, the duplicates are the twin's, diversity_offsets is the twin's
state; and DiversityReceiver(dfm_diversity=True) with an RS41, a DFM and an M10 sonde on two antennas' wideband streams delivers what
a batch fed by hand delivers."""
import numpy as np
import pytest
import torch

import dfm_diversity_reference as cr
import dfm_diversity_scenes as cs
from sdrpp_radiosonde_amd import _chain, _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE = cr.LEARN | cr.MARK


def _run(sc, iq, cuts, learn):
    step = sc.n // cuts
    b = SondeBatch(sc.C, step, types=np.full(sc.C, sc.type, dtype=np.uint8))
    if learn:
        b.set_diversity(sc.groups, None, sc.window, learn=True, mark_duplicates=True)
    parts = []
    for k in range(cuts):
        b.submit(iq[:, k * step:(k + 1) * step])
        parts.append(cs.sort_records(b.frames()))
    return parts, b


@pytest.mark.parametrize("cuts", [1, 2])
def test_members_lock_at_the_twins_submit_and_combine_from_then_on(cuts):
    sc = cs.scene(align=True)
    iq = torch.from_numpy(sc.iq).to(DEV)
    off, b0 = _run(sc, iq, cuts, False)
    b0.close()
    on, b = _run(sc, iq, cuts, True)
    state = cr.new_state(sc.groups, None, MODE)
    for k, (sub, got) in enumerate(zip(off, on)):
        want, _, state = cr.run(sub, sc.groups, state, MODE, sc.window)
        assert len(got) == len(want), k
        for a, e in zip(got, want):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), hex(int(a["flags"])), hex(int(e["flags"])))
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
    # the triple, 5000 chips apart, combines once its offsets are known
    assert state["div"]["combined"][2] >= 2
    comb = a[a["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) == sum(state["div"]["combined"]) >= 15
    for f in comb:
        assert bytes(f["data"][:33]) == bytes(cs.frame_of(sc, f)[2])
    b.close()


def test_diversity_receiver_with_an_rs41_a_dfm_and_an_m10_sonde_on_two_antennas():
    """three sondes in one wideband stream heard on two antennas; antenna 1 gets the same block two granules late and each antenna has a
    noise floor of its own.  What the receiver delivers is what a batch delivers that is fed the receiver's own tuners' rows by hand,
    with the same groups"""
    from sdrpp_radiosonde_amd.diversity import DiversityReceiver
    fs, sondes = 2_400_000, [(200_000, 0), (-350_000, 1), (500_000, 3)]
    for bad in (dict(), dict(dfm_rescue=True), dict(dfm_diversity=True, ims_rescue=True), dict(dfm_diversity=True, sondes=sondes + [(0, 2)])):
        with pytest.raises(SondeError):
            DiversityReceiver(fs, bad.pop("sondes", sondes), **bad)
    with pytest.raises(SondeError, match="RS41 sondes only"):
        DiversityReceiver(fs, sondes)
    kw = dict(antennas=2, max_in=20 * 102_400, dfm_diversity=True, dfm_rescue=True, manchester_rescue=True)
    rx = DiversityReceiver(fs, sondes, **kw)
    n, delay = 80 * rx.granule, 2 * rx.granule
    iq, frames, _ = synth.make_wideband_scene(sondes, n, fs=fs, ebn0_db=20.0, seed=5, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    ant0 = iq + 0.01 * torch.randn(iq.shape, generator=g, device=DEV)
    ant1 = iq + 0.01 * torch.randn(iq.shape, generator=g, device=DEV)
    ant1 = torch.cat([torch.zeros_like(ant1[:delay]), ant1[:n - delay]]).contiguous()
    S, K = len(sondes), 2
    hand = _chain.batch(K * S, _chain.plan(fs, [t for _, t in sondes], kw["max_in"]).n48, [t for _, t in sondes] * K, 0,
                        (False, True, True, False, False))
    hand.set_diversity([[a * S + i for a in range(K)] for i in range(S)], None, 0, learn=True, mark_duplicates=True)
    got, want = [], []
    for a in range(0, n, rx.max_in):
        rx.submit([ant0[a:a + rx.max_in], ant1[a:a + rx.max_in]])
        got.append(rx.frames()[0])
        hand.submit(rx._rows[:, :rx._n48].clone())
        f = hand.frames()
        f = f[(f["flags"] & _lib.FRAME_DUPLICATE) == 0]
        f["channel"] %= S
        want.append(f)
    got, want = np.concatenate(got), np.concatenate(want)
    assert got.tobytes() == want.tobytes()
    for i, (_, t) in enumerate(sondes):
        o = rx.offsets(i)
        assert o == hand.diversity_offsets(i) and o["locked"] == 3 and o["learned"] >= 1, (i, o)
        ok = (got["nerr"][:, 1] == 0) if t == 1 else (got["nerr"][:, 0] >= 0) & ((got["nerr"][:, 1] >= 0) | (t != 0))
        f = got[(got["channel"] == i) & ok]
        assert (f["type"] == t).all() and len(f) >= 3, (i, len(f))
        lo = 8 if t == 0 else 0
        seen = [bytes(r["data"][lo:int(r["len"])]) for r in f]
        assert len(set(seen)) == len(seen), i                 # one record per transmitted frame: no duplicates
        sent = {bytes(np.asarray(tx)[lo:len(seen[0]) + lo]) for _, tx in frames[i]}
        assert set(seen) <= sent, i
    hand.close()
    rx.close()
