"""Scenes for the tests of the coherent antenna combiner (DESIGN SPEC 3.14): one clean 48 kHz signal per sonde (the generator's
modulators at 60 dB, amplitude 1), which each of K antennas hears through its own complex gain and its own fade windows, under its
own white noise -- the antennas on one sample clock, started together.

    antennas()          the K rows of every sonde, signal and noise apart (linearity lets a test weigh them separately)
    fade_windows()      60 ms windows in which an antenna drops to 0.05 of its amplitude, never two antennas at once
    delivered()         how many of the transmitted frames the CPU oracle decodes from a set of rows

Shared by test_combine_reference.py (CPU) and test_gpu_combine.py; each scene is built once."""
from __future__ import annotations

import functools
import math

import numpy as np

from sdrpp_radiosonde_amd import synth

FS = 48000
FADE_SAMPLES = 2880              # 60 ms
FADE_DEPTH = 0.05
FADE_PERIOD = 9600               # antenna a's windows start at 960 + a * FADE_PERIOD / K + k * FADE_PERIOD
# What an antenna still hears in a null is scatter, not the direct path: its phase is unrelated to the path's and moves.  The scene
# lets it rotate at this rate (half a turn per 256-sample block), so that a weight phase that leans on a faded antenna is seen to.
FADE_SPIN_HZ = 93.75


@functools.lru_cache(maxsize=None)
def clean(t: int, channels: int, n: int, seed: int):
    """(s [channels, n] complex128 of amplitude 1, frames: per channel [(symbol offset, bytes)], baud)"""
    sb = synth.make_batch(t, channels, n, seed=seed, ebn0_db=60.0, amp_range=(1.0, 1.0))
    iq = sb.iq.numpy().astype(np.float64)
    s = iq[:, :, 0] + 1j * iq[:, :, 1]
    s.setflags(write=False)
    return s, sb.frames, synth.SCENE_BAUD[t]


def sigma(t: int, ebn0_db: float) -> float:
    """the noise's standard deviation per component that puts a GFSK carrier of amplitude 1 at this Eb/N0 (synth.gfsk_modulate's rule)"""
    return math.sqrt((FS / synth.SCENE_BAUD[t]) / (2.0 * 10.0 ** (ebn0_db / 10.0)))


def fade_windows(n: int, K: int):
    """per antenna the first samples of its windows: antenna a fades FADE_SAMPLES from 960 + a * FADE_PERIOD / K + k * FADE_PERIOD on"""
    assert FADE_PERIOD // K >= FADE_SAMPLES + 960
    return [list(range(960 + a * (FADE_PERIOD // K), n - FADE_SAMPLES, FADE_PERIOD)) for a in range(K)]


def fade_gain(n: int, starts) -> np.ndarray:
    """an antenna's gain factor over the stream: 1, and FADE_DEPTH times the scatter's moving phase inside its windows"""
    f = np.ones(n, np.complex128)
    spin = FADE_DEPTH * np.exp(2j * np.pi * FADE_SPIN_HZ / FS * np.arange(n))
    for a in starts:
        f[a:a + FADE_SAMPLES] = spin[a:a + FADE_SAMPLES]
    return f


def gains(K: int, seed: int, equal: bool = True) -> np.ndarray:
    """the antennas' complex gains: unit amplitude (equal=False: 1, 0.8, 0.9, 0.7) at phases of their own"""
    rng = np.random.default_rng(1000 + seed)
    amp = np.ones(K) if equal else np.array([1.0, 0.8, 0.9, 0.7])[:K]
    return amp * np.exp(2j * np.pi * rng.uniform(size=K))


def antennas(s: np.ndarray, K: int, sig: float, seed: int, *, fades: bool = False, equal: bool = True):
    """s [C, n] -> (signal [C, K, n], noise [C, K, n]) complex128; the rows an antenna delivers are their sum"""
    C, n = s.shape
    rng = np.random.default_rng(77 + seed)
    g = gains(K, seed, equal)
    f = [fade_gain(n, w) for w in fade_windows(n, K)] if fades else [np.ones(n, np.complex128)] * K
    signal = np.stack([np.stack([g[a] * f[a] * s[c] for a in range(K)]) for c in range(C)])
    noise = sig * (rng.standard_normal((C, K, n)) + 1j * rng.standard_normal((C, K, n)))
    return signal, noise


def as_f32(x: np.ndarray) -> np.ndarray:
    """what a float32 row holds of x, as complex128"""
    return x.real.astype(np.float32).astype(np.float64) + 1j * x.imag.astype(np.float32).astype(np.float64)


def delivered(t: int, rows: np.ndarray, frames) -> tuple[int, int]:
    """(transmitted whole, of those decoded by the CPU oracle) over rows [C, n] complex at 48 kHz"""
    import oracle_lib
    import track_reference as TR
    rows = np.asarray(rows)
    n = rows.shape[1] // 2048 * 2048
    iq = np.stack([rows.real[:, :n], rows.imag[:, :n]], axis=2).astype(np.float32)
    got = oracle_lib.batch_run(int(t), np.ascontiguousarray(iq), nthreads=4)
    symbols = int(n * synth.SCENE_BAUD[t] / FS)
    tally = TR.tally(got, [t] * len(frames), frames, [symbols] * len(frames))
    return sum(x[0] for x in tally), sum(x[1] for x in tally)
