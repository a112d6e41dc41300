"""The demodulator core (SPEC 3.0-3.0e, 3.2, 3.2b, 3.6, 3.6b: kernel A's K0-K3 and the oracle's or_dsp.c) against the float64
reference of tests/demod_reference.py, which is written from DESIGN.md alone.  The oracle is fed one tile at a time and, after every
tile, its bits and loop state are checked against ONE step of the SPEC's recurrence started from its own state before the tile
(demod_reference.replay): the bit count exactly, every bit unless the reference's y_k lies within its bound of the threshold, and the
level, timing, period, 3.6b and AFC updates within bounds that are formulas.  The mutation test at the end perturbs the REFERENCE the way
the bugs these bounds exist for would perturb a kernel and asserts that each is rejected.  The GPU half
(test_gpu_demod_reference.py) applies the same replay to SondeBatch."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import pytest

import demod_reference as D
from sdrpp_radiosonde_amd import synth

NT = 16                    # tiles per scene
# ambiguous bits per symbol at Eb/N0 >= 10 dB.  From the formula, not from a run: at 10 dB and 2.4 samples per symbol the noise on y_k
# has sigma >= 0.05 quadrant, and a Gaussian y_k lands within b of the threshold with probability <= 2 b / (sigma sqrt(2 pi)).  The
# tight layer's y bound is ~1e-5 outside squelched and noise-only stretches: <= 3e-4.  (The loose layer's, (2e-3 rad in quadrants) x
# sum |H| <= 1.2 = 1.5e-3, gives up to 5 %, so it asserts no limit.)
AMB_LIMIT = 0.01


@dataclass(frozen=True)
class Scene:
    """One channel.  kind: iq, iq16, iq8, real (48 kS/s discriminator audio) or dec (feed_decimated rows)."""
    name: str
    stype: int
    wide: bool = False
    kind: str = "iq"
    ebn0: float = 30.0
    cfo: float = 0.0
    ppm: float = 0.0
    level: float = 1.0          # IQ scale; for iq16 / iq8 the amplitude in counts (clipped at full scale)
    seed: int = 1
    m20: bool = False
    squelch: tuple = ()         # tiles replaced by zeros
    noise_tiles: int = 0        # leading tiles of noise only (the burst starts after them)
    ntiles: int = NT
    ramp_ppm: float = 0.0       # a symbol clock that drifts linearly from 0 to this offset (own NRZ FSK modulator)
    dc: float = 0.0             # dec rows only: a constant added in quadrants (a carrier 5 kHz x dc off a channelizer bin's centre)


def _tile_in(s: Scene) -> int:
    return D.TILE * (8 if s.stype in (4, 5) else 1)


def make_input(s: Scene):
    """float32 / integer input of one scene: [n, 2] for the IQ kinds, [n] for real, [n / decim] for dec"""
    n = s.ntiles * _tile_in(s)
    kw = dict(fs=D.FS / (1.0 + 1e-6 * s.ppm))
    if s.ramp_ppm:
        z = ramp_clock(n, synth.SONDE_BAUD[s.stype], s.ramp_ppm, s.ebn0, s.seed)
        x = (np.stack([z.real, z.imag], axis=1) * s.level).astype(np.float32)
        return x if s.kind == "iq" else _audio_of(s, x)
    if s.stype in (4, 5):
        sb = synth.make_batch(s.stype, 1, n, seed=s.seed, ebn0_db=s.ebn0, cfo_max_hz=0.0, **kw)
    else:
        sb = synth.make_batch(s.stype, 1, n, seed=s.seed, ebn0_db=s.ebn0, cfo_max_hz=0.0, m20=s.m20, **kw)
    iq = sb.iq.numpy()[0].astype(np.float64)
    z = (iq[:, 0] + 1j * iq[:, 1]) * np.exp(2j * np.pi * (s.cfo / D.FS * np.arange(n) % 1.0))
    if s.noise_tiles:
        rng = np.random.default_rng(s.seed + 77)
        sig = np.abs(z).mean() * math.sqrt(D.FS / synth.SONDE_BAUD.get(s.stype, 1200.0) / (2 * 10 ** (s.ebn0 / 10)))
        nn = s.noise_tiles * _tile_in(s)
        z[:nn] = sig * (rng.standard_normal(nn) + 1j * rng.standard_normal(nn))
    for t in s.squelch:
        z[t * _tile_in(s):(t + 1) * _tile_in(s)] = 0.0
    if s.kind in ("iq16", "iq8"):
        top = 32767 if s.kind == "iq16" else 127
        v = np.rint(np.stack([z.real, z.imag], axis=1) * s.level / np.abs(z).mean())
        return np.clip(v, -top, top).astype(np.int16 if s.kind == "iq16" else np.int8)
    x = (np.stack([z.real, z.imag], axis=1) * s.level).astype(np.float32)
    if s.kind == "iq":
        return x
    return _audio_of(s, x)


def _audio_of(s: Scene, x):
    """real input: the discriminator audio of the IQ (any float32 stream will do; this one carries the signal)"""
    zz = x[:, 0].astype(np.float64) + 1j * x[:, 1]
    audio = (np.angle(zz * np.conj(np.concatenate([[0], zz[:-1]]))) * (2 / np.pi)).astype(np.float32)
    if s.kind == "real":
        return audio
    dec = D.modem(s.stype, s.wide).decim
    return (audio.reshape(-1, dec).mean(1) + s.dc).astype(np.float32)


def ramp_clock(n: int, baud: float, ppm_end: float, ebn0: float, seed: int) -> np.ndarray:
    """random NRZ FSK (deviation baud / 2, transitions smoothed over a third of a symbol) whose symbol clock drifts linearly from the
    nominal rate to ppm_end off it over the n samples: the timing loop follows it until the period clamp of SPEC 3.2 stops it"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    sym = np.cumsum(baud / D.FS * (1.0 + 1e-6 * ppm_end * t / n))
    a = rng.choice([-1.0, 1.0], size=int(sym[-1]) + 3)
    k = np.floor(sym).astype(np.int64)
    w = np.clip((sym - k - 2.0 / 3.0) * 3.0, 0.0, 1.0)
    f = (a[k] + (a[k + 1] - a[k]) * 0.5 * (1.0 - np.cos(np.pi * w))) * baud / 2
    z = np.exp(2j * np.pi * np.cumsum(f) / D.FS)
    sig = math.sqrt(D.FS / baud / (2 * 10 ** (ebn0 / 10)))
    return z + sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def reference_disc(s: Scene, x, u_after, loose: bool = False, **mut):
    m = D.modem(s.stype, s.wide and s.kind != "real" and s.kind != "dec")
    if s.stype in (4, 5):
        return D.disc_afsk(x, s.stype, is_iq=s.kind != "real", loose=loose, **mut)
    if s.kind in ("real", "dec"):
        return D.disc_real(x, m, decimated=s.kind == "dec", **mut)
    return D.disc_iq(x, m, u_after, loose=loose, **mut)


def scene_modem(s: Scene) -> D.Modem:
    return D.modem(s.stype, s.wide and s.kind not in ("real", "dec"))


def check(s: Scene, x, states, bits, loose: bool = False, **mut) -> D.Check:
    u_after = np.array([st["afc_u"] for st in states])
    d, bd = reference_disc(s, x, u_after, loose=loose, **mut)
    return D.replay(d, bd, scene_modem(s), states, bits, afc=s.kind.startswith("iq") and s.stype not in (4, 5), **mut)


# ---------------------------------------------------------------- the oracle, one tile at a time
def run_oracle(oracle, s: Scene, x):
    """feed the oracle tile by tile: (states after every tile, new bits of every tile)"""
    L = oracle.lib()
    m = scene_modem(s)
    default = D.modem(s.stype).decim
    if m.decim != default:
        L.or_modem_set_decim(s.stype, m.decim)
    try:
        ch = oracle.Channel(s.stype, 0)
        dmod = L.or_channel_demod(ch.h)
        states, bits = [], []
        nb = 0
        tin = _tile_in(s)
        for j in range(s.ntiles):
            if s.kind == "dec":
                ch.feed_decimated(x[j * tin // m.decim:(j + 1) * tin // m.decim], m.decim)
            else:
                xt = np.ascontiguousarray(x[j * tin:(j + 1) * tin], dtype=np.float32)
                ch.feed(xt, is_iq=s.kind.startswith("iq"))
            n = int(L.or_demod_nbits(dmod))
            out = np.zeros(n - nb, np.uint8)
            if n > nb:
                L.or_demod_getbits(dmod, nb, n - nb, oracle.u8ptr(out))
            bits.append(out)
            nb = n
            states.append(ch.state())
        del ch
    finally:
        if m.decim != default:
            L.or_modem_set_decim(s.stype, default)
    return states, bits


# the pre-decimated path (what a channelizer bin feeds the loop, SPEC 3.5b) for every bin type at 10 and 20 dB, with the DC term an
# off-centre carrier leaves (+-0.9 quadrant = 4.5 kHz), clocks +-100 ppm, a noise-only lead-in, a squelched stretch, the period at its
# clamp, and M10's 2:1 class (more than 256 symbols per tile).  18 tiles: whole spans of 3 and of 6 (test_bins_reference.py hides states)
DEC_SCENES = [Scene("rs41-10dB-dec+0.9dc+100ppm", 0, kind="dec", ebn0=10.0, dc=0.9, ppm=100.0, seed=201, ntiles=18),
              Scene("rs41-20dB-dec-0.9dc-100ppm", 0, kind="dec", ebn0=20.0, dc=-0.9, ppm=-100.0, seed=202, ntiles=18),
              Scene("dfm-10dB-dec-0.9dc+100ppm", 1, kind="dec", ebn0=10.0, dc=-0.9, ppm=100.0, seed=203, ntiles=18),
              Scene("dfm-20dB-dec+0.4dc-100ppm", 1, kind="dec", ebn0=20.0, dc=0.4, ppm=-100.0, seed=204, ntiles=18),
              Scene("ims-10dB-dec+0.4dc-100ppm", 2, kind="dec", ebn0=10.0, dc=0.4, ppm=-100.0, seed=205, ntiles=18),
              Scene("ims-20dB-dec+0.9dc+100ppm", 2, kind="dec", ebn0=20.0, dc=0.9, ppm=100.0, seed=206, ntiles=18),
              Scene("mrz-10dB-dec-0.4dc+100ppm", 6, kind="dec", ebn0=10.0, dc=-0.4, ppm=100.0, seed=207, ntiles=18),
              Scene("mrz-20dB-dec-0.9dc-100ppm", 6, kind="dec", ebn0=20.0, dc=-0.9, ppm=-100.0, seed=208, ntiles=18),
              Scene("dfm-12dB-dec-noise-then-burst", 1, kind="dec", ebn0=12.0, dc=0.9, noise_tiles=4, seed=209, ntiles=18),
              Scene("rs41-20dB-dec-squelch", 0, kind="dec", ebn0=20.0, dc=-0.4, squelch=(5, 6, 7), seed=210, ntiles=18),
              Scene("rs41-20dB-dec-clock-ramp-to-clamp", 0, kind="dec", ebn0=20.0, ramp_ppm=-6000.0, seed=211, ntiles=420),
              Scene("m10-15dB-dec", 3, kind="dec", ebn0=15.0, dc=0.4, ppm=100.0, seed=212, ntiles=18)]


def _scenes():
    S = []
    seed = 10
    for t, nm in ((0, "rs41"), (1, "dfm"), (2, "ims"), (3, "m10"), (6, "mrz")):
        seed += 10
        S += [Scene(f"{nm}-10dB+1k+100ppm", t, ebn0=10.0, cfo=1000.0, ppm=100.0, seed=seed),
              Scene(f"{nm}-30dB-2k-100ppm", t, ebn0=30.0, cfo=-2000.0, ppm=-100.0, seed=seed + 1),
              Scene(f"{nm}-wide-12dB+2k", t, wide=True, ebn0=12.0, cfo=2000.0, seed=seed + 2)]
    S += [Scene("m20-12dB-1k", 3, m20=True, ebn0=12.0, cfo=-1000.0, seed=91),
          Scene("rs41-12dB-0k", 0, ebn0=12.0, seed=92),
          Scene("rs41-20dB+2k-iq16", 0, kind="iq16", ebn0=20.0, cfo=2000.0, level=20000.0, seed=93),
          Scene("dfm-20dB-2k-iq16-clip", 1, kind="iq16", ebn0=20.0, cfo=-2000.0, level=40000.0, seed=94),
          Scene("rs41-20dB-1k-iq8-8counts", 0, kind="iq8", ebn0=20.0, cfo=-1000.0, level=8.0, seed=95),
          Scene("mrz-20dB+1k-iq8-full", 6, kind="iq8", ebn0=20.0, cfo=1000.0, level=150.0, seed=96),
          Scene("rs41-15dB-real", 0, kind="real", ebn0=15.0, cfo=300.0, seed=97),
          Scene("m10-15dB-real", 3, kind="real", ebn0=15.0, cfo=-300.0, seed=98),
          Scene("dfm-15dB-dec", 1, kind="dec", ebn0=15.0, cfo=300.0, seed=99),
          Scene("rs41-20dB-clock+5000ppm", 0, ebn0=20.0, ppm=5000.0, seed=100),
          Scene("ims-20dB-clock-5000ppm", 2, ebn0=20.0, ppm=-5000.0, seed=101),
          Scene("rs41-20dB-clock-ramp-to-clamp", 0, ebn0=20.0, ramp_ppm=-6000.0, seed=111, ntiles=420),
          Scene("rs41-20dB+1k-squelch", 0, ebn0=20.0, cfo=1000.0, squelch=(5, 6, 7), seed=102),
          Scene("dfm-12dB-noise-then-burst", 1, ebn0=12.0, cfo=-1000.0, noise_tiles=4, seed=103),
          Scene("rs41-20dB-level1e-6", 0, ebn0=20.0, cfo=500.0, level=1e-6, seed=104),
          Scene("m10-20dB-level1e6", 3, ebn0=20.0, cfo=-500.0, level=1e6, seed=105),
          Scene("rs41-wide-iq16", 0, wide=True, kind="iq16", ebn0=15.0, cfo=-1500.0, level=3000.0, seed=106),
          *DEC_SCENES,
          Scene("imet-20dB", 4, ebn0=20.0, seed=107, ntiles=6),
          Scene("imet-12dB-real", 4, kind="real", ebn0=12.0, seed=108, ntiles=6),
          Scene("imet-20dB-iq8", 4, kind="iq8", ebn0=20.0, level=60.0, seed=109, ntiles=6),
          Scene("c50-20dB", 5, ebn0=20.0, seed=110, ntiles=6)]
    return S


SCENES = _scenes()
_CACHE: dict = {}


def observed(oracle, s: Scene):
    if s.name not in _CACHE:
        x = make_input(s)
        _CACHE[s.name] = (x,) + run_oracle(oracle, s, x)
    return _CACHE[s.name]


# ---------------------------------------------------------------- tap rows
def _rows_close(got, m: D.Modem, **mut):
    H = D.taps(m, **mut)
    got = np.asarray(got, np.float64)
    # the rows are computed in double and rounded once to float32 (u of each tap; the window is zero at -T/2 up to a cosine's rounding)
    ok = np.abs(got[:, :m.T] - H) <= D.U * np.abs(H) + 1e-15
    return bool(ok.all() and not got[:, m.T:].any())


@pytest.mark.parametrize("stype", [0, 1, 2, 3, 4, 5, 6])
def test_product_tap_rows_match_closed_form(stype):
    from sdrpp_radiosonde_amd.batch import get_taps
    got = get_taps(stype)
    assert _rows_close(got, D.modem(stype)), stype
    assert not _rows_close(got, D.modem(stype), cutoff=0.60)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("stype", [0, 1, 2, 3, 4, 5, 6])
def test_oracle_tap_rows_match_closed_form(oracle, stype, wide):
    L = oracle.lib()
    m = D.modem(stype, wide)
    default = D.modem(stype).decim
    if m.decim != default:
        L.or_modem_set_decim(stype, m.decim)
    try:
        got = np.zeros((32, 32), np.float32)
        L.or_make_taps(L.or_modem(stype), oracle.fptr(got.reshape(-1)))
    finally:
        if m.decim != default:
            L.or_modem_set_decim(stype, default)
    assert _rows_close(got, m)
    assert not _rows_close(got, m, normalise=False)


def test_recip_within_its_bound(oracle):
    """SPEC 3.2's recip (seed + three Newton steps) against the bound the reference uses, over every binade and the integers the
    loop divides by"""
    L = oracle.lib()
    rng = np.random.default_rng(3)
    xs = np.concatenate([np.arange(1, 513, dtype=np.float64), 2.0 ** rng.uniform(-60, 60, 20000),
                         (1.0 + np.arange(4096) / 4096.0) * 1e-3]).astype(np.float32)
    worst = max(abs(L.or_recip(float(x)) * float(x) - 1.0) for x in xs)
    assert worst <= D.RECIP_ERR, worst / D.U


# ---------------------------------------------------------------- the replay
def _report(s: Scene, chk: D.Check, tag: str = ""):
    print(chk.line(s.name + tag))


@pytest.mark.parametrize("s", SCENES, ids=[s.name for s in SCENES])
def test_oracle_replay(oracle, s):
    x, states, bits = observed(oracle, s)
    chk = check(s, x, states, bits)
    _report(s, chk)
    assert not chk.failures(), (s.name, chk.failures())
    assert chk.nbits > 0
    if s.ramp_ppm:          # the edge this scene exists for: the period sits at the clamp
        m = scene_modem(s)
        assert max(abs(st["period"] - m.period0) for st in states) == m.period0 >> 8
    if s.ebn0 >= 10.0:
        assert chk.amb <= AMB_LIMIT * chk.nbits, chk.line(s.name)


LOOSE = [s for s in SCENES if s.kind == "iq" and s.ebn0 >= 20.0]


@pytest.mark.parametrize("s", LOOSE, ids=[s.name for s in LOOSE])
def test_oracle_replay_loose(oracle, s):
    """the same with np.arctan2 plus SPEC 3.1's approximation error in place of the SPEC's atan2q"""
    x, states, bits = observed(oracle, s)
    chk = check(s, x, states, bits, loose=True)
    _report(s, chk, "/loose")
    assert not chk.failures(), (s.name, chk.failures())


# ---------------------------------------------------------------- the bounds reject the bugs
def _rejects(oracle, mut: dict) -> str | None:
    for s in SCENES:
        if "mix_hz" in mut or "box_blocks" in mut:
            if s.stype not in (4, 5):
                continue
        x, states, bits = observed(oracle, s)
        chk = check(s, x, states, bits, **mut)
        if chk.failures():
            return f"{s.name}: {chk.failures()}"
    return None


@pytest.mark.parametrize("name", sorted(D.MUTATIONS))
def test_mutation_is_rejected(oracle, name):
    why = _rejects(oracle, D.MUTATIONS[name])
    print(f"DEMOD-REF mutation {name}: rejected by {why}")
    assert why is not None, name
