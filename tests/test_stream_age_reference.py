"""The CPU half of the stream-age tests (DESIGN "Stream age"; the GPU half is test_gpu_stream_age.py).

Preconditions, on the CPU oracle fed the scenes of tests/age_scenes.py: the float64 replay accepts every tile of the stretch the
per-tile stages feed with an ambiguous share within AMB_LIMIT (so that the replay judges the aged kernel as sharply as the unaged
one), and in the wpos stages every sonde type has a frame whose bits span the boundary (so that "frames across 2^32 / 2^37" is about
something).  Mutations: the comparison helpers reject, on the oracle's output, a record whose bitpos is truncated to 32 bits, a
t_next reduced mod 2^48 and a tone mixer whose phase is taken from the sample count truncated to 32 bits -- the bugs the GPU tests
exist for.  Last, tests/tuner_reference.py's phase() stays exact at any age."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import age_scenes as A
import demod_reference as D
import tuner_reference as R
from test_demod_reference import AMB_LIMIT, check

SETS = ["iq", "iq-wide", "iq16", "real", "afsk"]


@functools.lru_cache(maxsize=None)
def observed(name: str):
    """the oracle over one scene set, submit by submit as the GPU tests feed it: per channel the states and new bits after every tile
    of the per-tile stretch, the bit count after the wpos stage's warm-up submit and at the end, and all records"""
    import oracle_lib as oracle
    oracle.build()
    L = oracle.lib()
    S, xs = A.scene_set(name)
    tin = A.tile_in(S)
    per_tile = (A.WARM + (3 * A.STAGE if tin == D.TILE else 4 * 6)) * tin           # the stretch the per-tile stages feed
    warm = A.SUBMIT * D.TILE
    out = []
    for s, x in zip(S, xs):
        m = A.scene_modem(s)
        default = D.modem(s.stype).decim
        if m.decim != default:
            L.or_modem_set_decim(s.stype, m.decim)
        try:
            ch = oracle.Channel(s.stype, 0)
            dmod = L.or_channel_demod(ch.h)
            states, bits, nb, nb_warm = [], [], 0, None
            for off in range(0, len(x), tin):
                ch.feed(np.ascontiguousarray(x[off:off + tin], dtype=np.float32), is_iq=s.kind.startswith("iq"))
                n = int(L.or_demod_nbits(dmod))
                if off + tin <= per_tile:
                    got = np.zeros(n - nb, np.uint8)
                    if n > nb:
                        L.or_demod_getbits(dmod, nb, n - nb, oracle.u8ptr(got))
                    bits.append(got)
                    states.append(ch.state())
                nb = n
                if off + tin == warm:
                    nb_warm = n
            out.append(dict(states=states, bits=bits, nb_warm=nb_warm, nbits=nb, frames=ch.frames()))
            del ch
        finally:
            if m.decim != default:
                L.or_modem_set_decim(s.stype, default)
    return out


@pytest.mark.parametrize("name", SETS)
def test_replay_accepts_the_oracle_on_the_new_scenes(name):
    S, xs = A.scene_set(name)
    amb = nbits = 0
    for s, x, o in zip(S, xs, observed(name)):
        n = len(o["states"]) * A.tile_in(S)
        chk = check(s, x[:n], o["states"], o["bits"])
        assert not chk.failures(), chk.line(s.name)
        assert chk.nbits > 0
        if s.ebn0 >= 10.0:
            assert chk.amb <= AMB_LIMIT * chk.nbits, chk.line(s.name)
        amb += chk.amb
        nbits += chk.nbits
    print(f"STREAM-AGE {name}: channels={len(S)} tiles={len(o['states'])} bits={nbits} ambiguous={amb} ({amb / max(nbits, 1):.2e})")


@pytest.mark.parametrize("boundary", [1 << 32, 1 << 37], ids=["2^32", "2^37"])
@pytest.mark.parametrize("name", SETS)
def test_every_type_has_a_frame_across_the_boundary(name, boundary):
    """the wpos stage as test_gpu_stream_age.py runs it: a warm-up submit, whole ring turns to less than a ring below the boundary,
    submits_to_cross(S) submits"""
    S, _ = A.scene_set(name)
    obs = observed(name)
    ring = A.ring_bits(S)
    added = [A.turns_below(boundary, o["nb_warm"], ring) * ring for o in obs]
    frames = []
    for c, o in enumerate(obs):
        f = o["frames"].copy()
        f["channel"] = c
        frames.append(f[f["bitpos"] >= o["nb_warm"]])
        assert o["nb_warm"] + added[c] < boundary <= o["nbits"] + added[c], (c, "the stage does not cross")
    got = A.spanning_types(np.concatenate(frames), added, boundary)
    assert got == {s.stype for s in S}, got


# ---------------------------------------------------------------- the checks see the bugs they exist for
def _aged(name="iq"):
    """the oracle's records and end states of a set as A, and as an aged B: every channel shifted as the wpos stage shifts it, and by
    2^32 internal samples"""
    S, _ = A.scene_set(name)
    obs = observed(name)
    ring = A.ring_bits(S)
    added = [A.turns_below(1 << 32, o["nb_warm"], ring) * ring for o in obs]
    fa = []
    for c, o in enumerate(obs):
        f = o["frames"].copy()
        f["channel"] = c
        fa.append(f[f["bitpos"] >= o["nb_warm"]])
    fa = np.concatenate(fa)
    fb = fa.copy()
    fb["bitpos"] += np.asarray([added[int(c)] for c in fb["channel"]], np.uint64)
    return fa, fb, added, obs


def test_a_bitpos_truncated_to_32_bits_is_rejected():
    fa, fb, added, _ = _aged()
    assert not A.frames_diff(fa, fb, added)
    over = np.flatnonzero(fb["bitpos"] >= np.uint64(1 << 32))
    assert len(over) > 0
    bad = fb.copy()
    bad["bitpos"][over[0]] &= np.uint64(0xFFFFFFFF)
    assert A.frames_diff(fa, bad, added)


def test_a_t_next_reduced_mod_2_48_is_rejected():
    _, _, _, obs = _aged()
    dt = (1 << 32) << 16                              # n0 shifted by 2^32 internal samples
    for o in obs:
        sa = o["states"][-1]
        sb = dict(sa, t_next=sa["t_next"] + dt)
        assert not A.state_diff(sa, sb, dt)
        assert sb["t_next"] >= 1 << 48
        assert A.state_diff(sa, dict(sb, t_next=sb["t_next"] % (1 << 48)), dt)
        assert A.state_diff(sa, dict(sb, period=sb["period"] + 1), dt)


def _afsk_run(s, x, af_n: int, wrap32: bool, tiles: int):
    """the oracle over the first tiles of an AFSK scene with the tone front-end's sample count started at af_n: (state, bits) per tile"""
    import oracle_lib as oracle
    L = oracle.lib()
    ch = oracle.Channel(s.stype, 0)
    dmod = L.or_channel_demod(ch.h)
    L.or_demod_test_set_af_n(dmod, af_n, int(wrap32))
    out, nb = [], 0
    tin = 8 * D.TILE
    for j in range(tiles):
        ch.feed(np.ascontiguousarray(x[j * tin:(j + 1) * tin], dtype=np.float32), is_iq=True)
        n = int(L.or_demod_nbits(dmod))
        got = np.zeros(n - nb, np.uint8)
        if n > nb:
            L.or_demod_getbits(dmod, nb, n - nb, oracle.u8ptr(got))
        nb = n
        out.append((ch.state(), got))
    return out


@pytest.mark.parametrize("stype", [4, 5])
def test_a_tone_mixer_phase_from_32_bits_of_the_sample_count_is_rejected(stype):
    """the oracle's tone front-end aged to less than 30720 samples below 2^32: with the SPEC's phase n mod 480 (n mod 240) its states
    and bits are the unaged ones; with the phase taken from the low 32 bits of n (2^32 mod 480 = 256: a phase jump) the comparison the
    GPU tests apply after every submit rejects it, on every channel of the type"""
    S, xs = A.scene_set("afsk")
    start = A.samples_below(1 << 32, 0)
    assert 0 < (1 << 32) - start <= A.Q
    seen = 0
    for s, x in zip(S, xs):
        if s.stype != stype:
            continue
        base, aged, bug = (_afsk_run(s, x, n, w, A.WARM) for n, w in ((0, False), (start, False), (start, True)))
        assert all(not A.state_diff(a[0], b[0], 0) and np.array_equal(a[1], b[1]) for a, b in zip(base, aged)), s.name
        assert any(A.state_diff(a[0], b[0], 0) for a, b in zip(base, bug)), s.name
        seen += 1
    assert seen == 16


def test_reference_tuner_phase_is_exact_at_any_age():
    rng = np.random.default_rng(1)
    for fs in (20_000_000, 10_000_000, 2_400_000, 1_999_999):
        for start in (0, (1 << 31) - 5, (1 << 32) - 5, 1 << 40, (1 << 62) - 777, (1 << 62) + 12345):
            n = rng.integers(0, 200_000, 64)
            for f in (-fs // 2 + 1, -1, 1, 7, fs // 2 - 1, int(rng.integers(-fs // 2, fs // 2))):
                want = [(f * (start + int(k))) % fs for k in n]                  # Python integers: exact at any size
                assert R.phase(f, n, fs, start).tolist() == want, (fs, start, f)
