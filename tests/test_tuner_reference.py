"""The wideband tuner's CPU half (DESIGN SPEC 3.9): rates and tap counts, the product's float32 taps against the float64 formula of
tests/tuner_reference.py, the filter's response, the float64 reference's own tone checks, and the mutations the GPU comparison's
error bound must reject.  No GPU needed: sonde_tuner_ratio / sonde_tuner_taps are host functions of the library."""
from __future__ import annotations

import numpy as np
import pytest

import tuner_reference as R
from sdrpp_radiosonde_amd import tuner
from sdrpp_radiosonde_amd.batch import SondeError

# (Fs, R, B) -> (up, down, T, N)
TABLE = [
    ((10_000_000, 10_000, 10_000), (1, 1000, 32_000, 32_000)),
    ((10_000_000, 48_000, 10_000), (3, 625, 32_000, 96_000)),
    ((10_000_000, 15_000, 15_000), (3, 2000, 21_344, 64_032)),
    ((10_000_000, 48_000, 40_000), (3, 625, 8_000, 24_000)),
    ((10_000_000, 50_000, 50_000), (1, 200, 6_400, 6_400)),
    ((2_400_000, 48_000, 20_000), (1, 50, 3_840, 3_840)),
    ((2_400_000, 15_000, 15_000), (1, 160, 5_120, 5_120)),
    ((2_048_000, 15_000, 15_000), (15, 2048, 4_384, 65_760)),
    ((2_048_000, 48_000, 10_000), (3, 128, 6_560, 19_680)),
    ((20_000_000, 100_000, 5_000), (1, 200, 128_000, 128_000)),
]
# the response checks of the issue: float32 taps, ripple <= 0.01 dB up to 0.4 B, <= -70 dB beyond 0.6 B, -6 dB at B / 2
RESPONSE = [(10_000_000, 10_000, 10_000), (10_000_000, 48_000, 10_000), (10_000_000, 15_000, 15_000), (10_000_000, 48_000, 40_000),
            (2_400_000, 48_000, 20_000), (2_048_000, 15_000, 15_000)]


@pytest.mark.parametrize("args,want", TABLE)
def test_ratio_and_tap_counts(args, want):
    fs, r, b = args
    up, down, T, N = want
    assert R.ratio(fs, r) == (up, down) == tuner.ratio(fs, r)
    assert R.taps_per_phase(fs, b) == T and up * T == N
    assert tuner.tuner_taps(fs, r, b).shape == (up, T)


@pytest.mark.parametrize("fs,r", [(10_000_000, 48_001), (999_999, 10_000), (20_000_001, 10_000), (10_000_000, 100_001),
                                  (400_000 * 8 - 8, 400_000), (1_000_000, 125_001), (1_000_000, 0)])
def test_refused_rates(fs, r):
    with pytest.raises(ValueError):
        R.ratio(fs, r)
    with pytest.raises(SondeError, match="sonde_tuner_ratio"):
        tuner.ratio(fs, r)


@pytest.mark.parametrize("b", [4999, 10_001])
def test_refused_bandwidths(b):
    with pytest.raises(SondeError, match="bandwidth"):
        tuner.tuner_taps(10_000_000, 10_000, b)


@pytest.mark.parametrize("args", [a for a, _ in TABLE])
def test_taps_within_one_ulp_of_the_float64_formula(args):
    g = tuner.tuner_taps(*args)
    want = R.taps64(*args)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(g.astype(np.float64) - want)
    assert np.all(err <= ulp), float(np.max(err / ulp))
    differ = int(np.count_nonzero(g != want.astype(np.float32)))
    # a different order of the double sums may flip a few roundings; report how many
    print(f"{args}: {differ} of {g.size} taps differ from the float64 formula rounded to float32 (each by one ulp at most)")
    assert differ <= max(16, g.size // 1000)


@pytest.mark.parametrize("args", [a for a, _ in TABLE])
def test_unit_dc_gain_per_phase(args):
    g = tuner.tuner_taps(*args).astype(np.float64)
    T = g.shape[1]
    assert np.all(np.abs(g.sum(axis=1) - 1.0) <= T * R.U * np.abs(g).sum(axis=1) + 2 * R.U)


@pytest.mark.parametrize("fs,r,b", RESPONSE)
def test_response_from_the_float32_taps(fs, r, b):
    g = tuner.tuner_taps(fs, r, b)
    f_pass = np.linspace(0.0, 0.4 * b, 401)
    assert np.max(np.abs(R.response_db(g, fs, f_pass))) <= 0.01
    assert abs(R.response_db(g, fs, np.array([0.5 * b]))[0] + 6.02) <= 0.1
    f_stop = np.concatenate([np.linspace(0.6 * b, 3.0 * b, 4001), np.linspace(3.0 * b, 0.5 * fs, 4001)])
    assert np.max(R.response_db(g, fs, f_stop)) <= -70.0


@pytest.mark.parametrize("d", [0.0, 1234.0, -2600.0, 4000.0, 6000.0])
def test_reference_tone_comes_out_at_d_with_gain_H(d):
    """A tone at f_k + d leaves VFO k as a tone at d with the prototype's gain |H(d)| (float64 reference, float64 taps)."""
    fs, r, b, f = 1_000_000, 10_000, 10_000, -123_457
    up, down = R.ratio(fs, r)
    g = R.taps64(fs, r, b)
    T = g.shape[1]
    n = 3 * T + 40 * down
    x = np.exp(2j * np.pi * (f + d) * np.arange(n) / fs)
    y, _ = R.tuner_ref(x, fs, r, g, [f], [n], j_range=(-(-T * up // down) + 1, n * up // down))
    j = np.arange(n * up // down)[-len(y):]
    H = 10.0 ** (R.response_db(g, fs, np.array([d]))[0] / 20.0)
    want = H * np.exp(2j * np.pi * d * (j * down / up) / fs) * np.exp(-2j * np.pi * d * (T - 1) / 2 / fs)     # linear phase, delay (T - 1) / 2
    assert np.max(np.abs(np.abs(y) - H)) <= 1e-6 + 1e-4 * H
    assert np.max(np.abs(y - want)) <= 1e-6 + 1e-3 * H


def _scene(fs, n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = sum(a * np.exp(2j * np.pi * (fo * t / fs + rng.uniform())) for a, fo in ((0.8, 31_234), (0.5, 36_000), (0.3, -200_000)))
    return (x + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64).astype(np.complex128)


@pytest.mark.parametrize("mutation", [dict(flip_sign=True), dict(tap_shift=1), dict(phase_shift=1), dict(drop_history=True),
                                      dict(local_mixer=True)])
def test_every_mutation_breaks_the_bound(mutation):
    """The GPU comparison (tests/test_gpu_tuner.py) accepts a row within R.bound of the reference; each of these bugs moves some
    output further than that."""
    fs, r, b, f = 2_048_000, 15_000, 15_000, 31_234          # off the 1 kHz raster: f n_base mod Fs != 0 at every boundary
    up, down = R.ratio(fs, r)
    g = R.taps64(fs, r, b)
    T = g.shape[1]
    subs = [3 * down, 2 * down + 0, 4 * down]
    x = _scene(fs, sum(subs))
    offs = [f] * len(subs)
    y, A = R.tuner_ref(x, fs, r, g, offs, subs)
    ym, _ = R.tuner_ref(x, fs, r, g, offs, subs, **mutation)
    bnd = R.bound(A, T)
    dev = np.maximum(np.abs(ym.real - y.real), np.abs(ym.imag - y.imag))
    assert np.any(dev > 10.0 * bnd), (mutation, float(np.max(dev / np.maximum(bnd, 1e-30))))


def test_phase_is_exact_for_large_indices():
    fs = 10_000_000
    n = np.array([0, 1, fs - 1, fs, 10 ** 14 + 7, 2 ** 52 + 3], dtype=np.int64)
    for f in (1, -1, 4_999_999, -4_999_999, 123_457):
        want = [(f * int(k)) % fs for k in n]
        assert R.phase(f, n, fs).tolist() == want
