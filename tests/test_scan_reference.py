"""The band scanner's host half (DESIGN SPEC 3.10) without a GPU: the library's window and automatic FFT size against
tests/scan_reference.py, sonde_scan_search against search_ref on reference spectra of whole scenes and of a hand-built spectrum,
the reference against the truth of the scenes, and the spectrum bound against the mutations it exists to reject."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import scan_reference as R
from sdrpp_radiosonde_amd import scan, synth
from sdrpp_radiosonde_amd.batch import SondeError

FS = 10_000_000
N_SCAN = 1_280_000
# tests/test_gpu_tuner.py's SCENE: (offset, type, m20)
SCENE = [(-3_512_345, 0, False), (-2_100_777, 1, False), (1_234_567, 2, False), (2_500_003, 3, False), (3_700_111, 3, True),
         (-700_321, 4, False), (150_013, 5, False), (4_200_999, 6, False)]
ADJACENT = [(1_000_003, 0), (1_020_003, 0)]


@functools.lru_cache(maxsize=None)
def _scene(which: str, ebn0):
    if which == "scene":
        iq, _, _ = synth.make_wideband_scene(SCENE, N_SCAN, fs=FS, ebn0_db=ebn0, seed=21, cfo_max_hz=0.0)
    elif which == "adjacent":
        iq, _, _ = synth.make_wideband_scene(ADJACENT, N_SCAN, fs=FS, ebn0_db=[20.0, 50.0], seed=33, cfo_max_hz=0.0)
    else:
        iq, _, _ = synth.make_wideband_scene([], N_SCAN, fs=FS, seed=22, cfo_max_hz=0.0)
    a = iq.numpy().astype(np.float64)
    return a[:, 0] + 1j * a[:, 1]


@functools.lru_cache(maxsize=None)
def _spectrum(which: str, ebn0, N: int) -> np.ndarray:
    P, S, _ = R.spectrum_ref(_scene(which, ebn0), FS, N)
    assert S == (N_SCAN - N) // (N // 2) + 1
    return P.astype(np.float32)


def _same(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for g, r in zip(got, ref):
        assert (int(g["bin"]), int(g["offset_hz"]), int(g["bandwidth_hz"])) == (r["bin"], r["offset_hz"], r["bandwidth_hz"]), (g, r)
        assert abs(float(g["cn0_dbhz"]) - r["cn0_dbhz"]) <= 1e-4 and abs(float(g["excess_db"]) - r["excess_db"]) <= 1e-4, (g, r)


def test_window_bit_for_bit_and_auto_fft_size():
    for n in (1024, 2048, 4096, 8192, 16384):
        assert np.array_equal(scan.window(n).view(np.uint32), R.window(n).view(np.uint32)), n
    table = {1_000_000: 1024, 2_048_000: 2048, 2_400_000: 4096, 10_000_000: 16384, 20_000_000: 16384}
    for fs, n in table.items():
        assert scan.auto_fft_size(fs) == R.auto_fft_size(fs) == n, fs
    with pytest.raises(SondeError, match="fft_size"):
        scan.window(1000)
    with pytest.raises(SondeError, match="rate_in"):
        scan.auto_fft_size(999_999)


PARAMS = [dict(), dict(smooth_hz=5000, min_sep_hz=25000, centroid_hz=12000, threshold=2.5)]


@pytest.mark.parametrize("par", PARAMS, ids=["defaults", "other"])
@pytest.mark.parametrize("which,ebn0,N", [("scene", 20.0, 16384), ("scene", 12.0, 8192), ("adjacent", None, 16384), ("noise", None, 8192)])
def test_search_equals_the_reference_on_scenes(which, ebn0, N, par):
    P = _spectrum(which, ebn0, N)
    ref = R.search_ref(P, FS, **par)
    _same(scan.search(P, FS, **par), ref)
    if which == "noise":
        assert ref == []
    if which == "adjacent" and not par:
        assert len(ref) == 2 and all(abs(c["offset_hz"] - f) <= 500 for c, (f, _) in zip(ref, ADJACENT)), ref


def _hand_built(N: int) -> np.ndarray:
    """a floor with a fixed ripple, flat-topped carriers (equal neighbours: ties in the moving sum), two equal carriers inside one
    separation window (the band-edge carriers are added by the test, where its parameters put the edges)"""
    P = (1.0 + 0.25 * np.sin(0.37 * np.arange(N)) ** 2).astype(np.float32)
    for a, b, v in ((300, 306, 50.0), (500, 501, 80.0), (504, 505, 80.0), (700, 700, 30.0), (703, 703, 30.0)):
        P[a:b + 1] = v
    return P


@pytest.mark.parametrize("par", [dict(), dict(smooth_hz=12000, min_sep_hz=6000, centroid_hz=4000, threshold=1.5)], ids=["defaults", "other"])
def test_search_ties_and_band_edges(par):
    N, fs = 1024, 2_048_000
    P = _hand_built(N)
    delta = fs / N
    h = max(1, int(math.floor(par.get("smooth_hz", 8000) / (2 * delta) + 0.5)))
    g = max(1, int(math.floor(par.get("centroid_hz", 16000) / (2 * delta) + 0.5)))
    e0 = max(h, g)
    for k in range(-3, 4):                       # the moving sum peaks exactly at the first bin a candidate may have and at the last
        P[e0 + k] = P[N - 1 - e0 + k] = 120.0 - 10.0 * abs(k)
    ref = R.search_ref(P, fs, **par)
    bins = [c["bin"] for c in ref]
    assert e0 in bins and N - 1 - e0 in bins and len(ref) >= 5, bins
    _same(scan.search(P, fs, **par), ref)


def test_search_refusals():
    P = np.ones(1024, np.float32)
    with pytest.raises(SondeError, match="fft_size"):
        scan.search(P[:1000], 2_048_000)
    with pytest.raises(SondeError, match="rate_in"):
        scan.search(P, 30_000_000)
    with pytest.raises(SondeError, match="threshold"):
        scan.search(P, 2_048_000, threshold=-1.0)
    assert len(scan.search(P, 2_048_000)) == 0


@pytest.mark.parametrize("N", [8192, 16384])
@pytest.mark.parametrize("ebn0", [20.0, 12.0])
def test_reference_finds_every_sonde_of_the_scene(ebn0, N):
    """The reference against the truth: one candidate per sonde and none elsewhere, offsets within 500 Hz, C/N0 within 1 dB of what
    the scene sets, every M10 / M20 wider than every RS41."""
    cand = R.search_ref(_spectrum("scene", ebn0, N), FS)
    assert len(cand) == len(SCENE), [c["offset_hz"] for c in cand]
    truth = sorted(SCENE)
    bw = {}
    for c, (f, t, m20) in zip(cand, truth):
        assert abs(c["offset_hz"] - f) <= 500, (c, f, t)
        want = ebn0 + 10.0 * math.log10(48000.0 if t in (4, 5) else synth.SCENE_BAUD[t])
        assert abs(c["cn0_dbhz"] - want) <= 1.0, (c, t, want)
        bw.setdefault(t, []).append(c["bandwidth_hz"])
    assert min(bw[3]) > max(bw[0]), bw


def test_noise_alone_gives_no_candidate():
    for N in (8192, 16384):
        assert R.search_ref(_spectrum("noise", None, N), FS, threshold=2.0) == []
        assert len(scan.search(_spectrum("noise", None, N), FS, threshold=2.0)) == 0


def _case_stream(case):
    fs, N, kind, cuts = case
    N = N or R.auto_fft_size(fs)
    return fs, N, kind, cuts, R.make_stream(fs, N, kind, sum(cuts) + 1, seed=fs % 997 + N, burst=True)


@pytest.mark.parametrize("case", R.SPECTRUM_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in R.SPECTRUM_CASES])
def test_bound_rejects_mutations_and_stays_below_one_percent(case):
    """On every stream the GPU test uses: the bound is below 1 % of the reference at every bin, and a rectangular window, segments
    one sample late, one segment dropped and a mirrored frequency axis each exceed it somewhere."""
    fs, N, kind, cuts, x = _case_stream(case)
    P, S, norms = R.spectrum_ref(x, fs, N, cuts)
    assert S == (sum(cuts) - N) // (N // 2) + 1 and len(norms) == S
    B = R.spectrum_bound(P, N, norms)
    assert np.all(B < 0.01 * P), float(np.max(B / P))
    P2, _, _ = R.spectrum_ref(x[:sum(cuts)], fs, N)                  # the cuts do not matter
    assert np.array_equal(P, P2)
    for name, kw in (("rect", dict(rect_window=True)), ("shift", dict(shift=1)), ("drop", dict(drop_segment=S // 2)), ("mirror", dict(mirror=True))):
        Pm, _, _ = R.spectrum_ref(x, fs, N, cuts, **kw)
        assert np.any(np.abs(Pm - P) > B), name
