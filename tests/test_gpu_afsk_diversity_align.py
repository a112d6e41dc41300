"""-m gpu: the align step of sonde_batch_set_diversity_auto for iMet groups (DESIGN SPEC 3.3k with the predicates of SPEC 3.3o) against
its twin (afsk_diversity_reference.align / run): with learn=True and no offsets the members of the scene's groups -- the triple 0, 300
and 5000 symbols late -- lock at the twin's submit and combine from then on, the duplicates are the twin's (PTU and GPS packets, no
XDATA packet), diversity_offsets is the twin's state; and DiversityReceiver(afsk_diversity=True) with two iMet sondes on two antennas'
wideband streams delivers what a batch fed by hand delivers."""
import numpy as np
import pytest
import torch

import afsk_diversity_reference as ad
import afsk_diversity_scenes as ds
from sdrpp_radiosonde_amd import _chain, _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE = ad.LEARN | ad.MARK
FLAG = _lib.FLAG_AFSK_DIVERSITY


def _run(sc, iq, cuts, learn):
    step = sc.n // cuts
    b = SondeBatch(sc.C, step, types=np.full(sc.C, sc.type, dtype=np.uint8), flags=FLAG)
    if learn:
        b.set_diversity(sc.groups, None, 0, learn=True, mark_duplicates=True)
    parts = []
    for k in range(cuts):
        b.submit(iq[:, k * step:(k + 1) * step])
        parts.append(ds.sort_records(b.frames()))
    return parts, b


@pytest.mark.parametrize("cuts", [1, 2])
def test_members_lock_at_the_twins_submit_and_combine_from_then_on(cuts):
    sc = ds.scene("imet", align=True)
    iq = torch.from_numpy(sc.iq).to(DEV)
    off, b0 = _run(sc, iq, cuts, False)
    b0.close()
    on, b = _run(sc, iq, cuts, True)
    state = ad.new_state(sc.groups, None, MODE)
    for k, (sub, got) in enumerate(zip(off, on)):
        want, _, state = ad.run(sub, sc.groups, state, MODE, 0)
        assert len(got) == len(want), k
        for a, e in zip(got, want):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), hex(int(a["flags"])), hex(int(e["flags"])))
    a = np.concatenate(on)
    dup = a["flags"] & _lib.FRAME_DUPLICATE != 0
    assert dup.sum() == sum(state["duplicates"]) >= 40
    assert not (dup & ~np.isin(a["len"], (14, 18))).any() and (a["len"] == 13).sum() >= 40      # no XDATA copy is marked
    for g, members in enumerate(sc.groups):
        o = b.diversity_offsets(g)
        assert o["offsets"][:len(members)] == [state["off"][ch] for ch in members], g
        assert o["locked"] == sum(1 << m for m, ch in enumerate(members) if state["locked"][ch]), (g, o)
        assert o["learned"] == state["learned"][g] and o["duplicates"] == state["duplicates"][g], (g, o)
        assert b.diversity_info(g) == {"tried": state["div"]["tried"][g], "combined": state["div"]["combined"][g]}, g
    if cuts == 1:                    # every copy of a packet is seen at once: every member locks, at its true delay
        assert all(state["locked"].values())
        o = b.diversity_offsets(3)["offsets"]
        assert abs(o[1] - o[0] - 300) <= 7 and abs(o[2] - o[0] - 5000) <= 7      # the demodulators' delays lie 6..13 symbols
    comb = a[a["flags"] & _lib.FRAME_COMBINED != 0]
    assert len(comb) == sum(state["div"]["combined"]) >= 12
    for f in comb:
        tx = ds.frame_of(sc, f)[2]
        assert bytes(f["data"][:len(tx)]) == bytes(tx)
    b.close()


def test_diversity_receiver_with_two_imet_sondes_on_two_antennas():
    """two iMet sondes in one wideband stream heard on two antennas; antenna 1 gets the same block one granule late and each antenna
    has a noise floor of its own.  What the receiver delivers is what a batch delivers that is fed the receiver's own tuners' rows by
    hand, with the same groups.  1 MS/s is the smallest rate the tuner takes; its granule with an AFSK sonde is 1 024 000 samples."""
    from sdrpp_radiosonde_amd.diversity import DiversityReceiver
    fs, sondes = 1_000_000, [(200_000, 4), (-150_000, 4)]
    with pytest.raises(SondeError, match="RS41 sondes only"):            # without afsk_diversity an iMet sonde is refused as before
        DiversityReceiver(fs, sondes)
    with pytest.raises(SondeError):
        DiversityReceiver(fs, sondes, afsk_rescue=True)
    with pytest.raises(SondeError):
        DiversityReceiver(fs, sondes + [(0, 5)], afsk_diversity=True)     # C50: no learned offsets
    kw = dict(antennas=2, afsk_diversity=True, afsk_rescue=True)
    rx = DiversityReceiver(fs, sondes, **kw)
    assert rx.granule == 1_024_000 and rx.max_in == rx.granule
    n, delay = 5 * rx.granule, rx.granule
    iq, frames, _ = synth.make_wideband_scene(sondes, n, fs=fs, ebn0_db=20.0, seed=5, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    ant0 = iq + 0.01 * torch.randn(iq.shape, generator=g, device=DEV)
    ant1 = iq + 0.01 * torch.randn(iq.shape, generator=g, device=DEV)
    ant1 = torch.cat([torch.zeros_like(ant1[:delay]), ant1[:n - delay]]).contiguous()
    S, K = len(sondes), 2
    hand = _chain.batch(K * S, _chain.plan(fs, [t for _, t in sondes]).n48, [t for _, t in sondes] * K, 0,
                        (False, False, False, False, True), flags=FLAG)
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
    for i in range(S):
        o = rx.offsets(i)
        assert o == hand.diversity_offsets(i), (i, o)
        f = got[(got["channel"] == i) & (got["nerr"][:, 0] >= 0)]
        assert (f["type"] == 4).all() and len(f) >= 3, (i, len(f))
    hand.close()
    rx.close()
