"""The band scanner on the GPU (DESIGN SPEC 3.10) against tests/scan_reference.py: the spectrum within a formula bound at several
rates, sizes and input kinds; bit-identical spectra however the stream is cut; reset; candidates equal to the reference search over
the GPU's own spectrum; refusals; then whole scenes with no truth handed over: scan, tune, decode, and survey() (scan, detect the
types) then decode."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import scan_reference as R
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeError
from sdrpp_radiosonde_amd.scan import SondeScanner, survey
from sdrpp_radiosonde_amd.tuner import WidebandReceiver

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IQ, IQ16, IQ8 = _lib.INPUT_IQ, _lib.INPUT_IQ16, _lib.INPUT_IQ8
KIND = {"iq": IQ, "iq16": IQ16, "iq8": IQ8}
DT = {IQ: torch.float32, IQ16: torch.int16, IQ8: torch.int8}


def _dev(x, kind):
    return torch.from_numpy(np.stack([x.real, x.imag], axis=1)).to(DT[kind]).to(DEV)


def _run(sc, dev, cuts):
    a = 0
    for k in cuts:
        sc.submit(dev[a:a + k].contiguous())
        a += k
    assert a == dev.shape[0]
    return sc.spectrum()[1]


def _chunks(n, k):
    return [k] * (n // k) + ([n % k] if n % k else [])


@pytest.mark.parametrize("case", R.SPECTRUM_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in R.SPECTRUM_CASES])
def test_spectrum_within_the_bound(case):
    fs, N, kind, cuts = case
    n = sum(cuts)
    N0 = N or R.auto_fft_size(fs)
    x = R.make_stream(fs, N0, kind, n + 1, seed=fs % 997 + N0, burst=True)[:n]          # the stream tests/test_scan_reference.py checks the bound on
    sc = SondeScanner(fs, max(cuts), fft_size=N, input_kind=KIND[kind])
    assert sc.fft_size == N0
    assert min(cuts) == 1 and any(1 < c < N0 // 2 for c in cuts)
    P = _run(sc, _dev(x, KIND[kind]), cuts)
    freqs = sc.spectrum()[0]
    assert sc.segments == (n - N0) // (N0 // 2) + 1
    assert freqs[0] == -fs / 2 and freqs[N0 // 2] == 0.0 and P.dtype == np.float32
    ref, S, norms = R.spectrum_ref(x, fs, N0, cuts)
    assert S == sc.segments
    bnd = R.spectrum_bound(ref, N0, norms)
    err = np.abs(P.astype(np.float64) - ref)
    print(f"fs {fs} N {N0} {kind}: max |P - ref| / bound {float(np.max(err / bnd)):.4f}, max |P - ref| / ref {float(np.max(err / ref)):.3e}")
    assert np.all(err <= bnd), float(np.max(err / bnd))
    _same(sc.candidates(), R.search_ref(P, fs))
    sc.close()


def test_spectrum_bit_identical_however_the_stream_is_cut():
    fs, N, n = 10_000_000, 8192, 200_003
    x16 = R.make_stream(fs, N, "iq16", n, seed=5, burst=True)
    f32 = _dev(x16, IQ)
    one = _run(SondeScanner(fs, n, fft_size=N), f32, [n])
    ragged = [1, 4095, 3000, 8192, 100_000, 7, 50_001]
    ragged.append(n - sum(ragged))
    small = _chunks(n, 2731)                                     # max_in smaller than N: most submits only lengthen the carried tail
    for cuts in (ragged, small, _chunks(n, N // 2), _chunks(n, N)):
        got = _run(SondeScanner(fs, max(cuts), fft_size=N), f32, cuts)
        assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), cuts[:4]
    got = _run(SondeScanner(fs, max(ragged), fft_size=N, input_kind=IQ16), _dev(x16, IQ16), ragged)
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32))
    x8 = R.make_stream(fs, N, "iq8", n, seed=6, burst=True)
    one8 = _run(SondeScanner(fs, n, fft_size=N), _dev(x8, IQ), [n])
    got = _run(SondeScanner(fs, max(small), fft_size=N, input_kind=IQ8), _dev(x8, IQ8), small)
    assert np.array_equal(got.view(np.uint32), one8.view(np.uint32))
    assert not np.array_equal(one8.view(np.uint32), one.view(np.uint32))


def test_a_long_submit_takes_several_launches():
    """more segments in one submit than one launch holds power rows for (at most 2048): the same spectrum as in short submits"""
    fs, N, n = 2_048_000, 1024, 1_200_001
    x = R.make_stream(fs, N, "iq", n, seed=8, burst=True)
    dev = _dev(x, IQ)
    one = _run(SondeScanner(fs, n, fft_size=N), dev, [n])
    got = _run(SondeScanner(fs, 100_000, fft_size=N), dev, _chunks(n, 100_000))
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32))
    ref, S, norms = R.spectrum_ref(x, fs, N)
    assert S > 2048 and np.all(np.abs(one.astype(np.float64) - ref) <= R.spectrum_bound(ref, N, norms))


def test_reset():
    fs, N = 2_400_000, 4096
    a = _dev(R.make_stream(fs, N, "iq", 50_001, seed=1), IQ)
    b = _dev(R.make_stream(fs, N, "iq", 70_003, seed=2, burst=True), IQ)
    sc = SondeScanner(fs, 40_000, fft_size=N)
    _run(sc, a, _chunks(50_001, 40_000))
    sc.reset()
    assert sc.segments == 0
    with pytest.raises(SondeError, match="segment"):
        sc.spectrum()
    got = _run(sc, b, _chunks(70_003, 33_333))
    fresh = _run(SondeScanner(fs, 70_003, fft_size=N), b, [70_003])
    assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32))


def _same(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for g, r in zip(got, ref):
        assert (int(g["bin"]), int(g["offset_hz"]), int(g["bandwidth_hz"])) == (r["bin"], r["offset_hz"], r["bandwidth_hz"]), (g, r)
        assert abs(float(g["cn0_dbhz"]) - r["cn0_dbhz"]) <= 1e-4 and abs(float(g["excess_db"]) - r["excess_db"]) <= 1e-4, (g, r)


def test_refusals():
    with pytest.raises(SondeError, match="input_kind"):
        SondeScanner(10_000_000, 1000, input_kind=_lib.INPUT_REAL)
    for fs in (999_999, 20_000_001):
        with pytest.raises(SondeError, match="rate_in"):
            SondeScanner(fs, 1000)
    for n in (1000, 512, 32768):
        with pytest.raises(SondeError, match="fft_size"):
            SondeScanner(10_000_000, 1000, fft_size=n)
    with pytest.raises(SondeError, match="max_in"):
        SondeScanner(10_000_000, 0)
    with pytest.raises(SondeError, match="sonde_scan_create: no such HIP device"):
        SondeScanner(10_000_000, 1000, device=torch.cuda.device_count())
    sc = SondeScanner(10_000_000, 5000, fft_size=4096)
    blk = torch.zeros((5000, 2), device=DEV)
    with pytest.raises(SondeError, match="n_in"):
        sc.submit(blk[:0])
    with pytest.raises(SondeError, match="n_in"):
        sc.submit(torch.zeros((5001, 2), device=DEV))
    with pytest.raises(SondeError, match="float32"):
        sc.submit(blk.to(torch.int16))
    with pytest.raises(SondeError, match="device tensor"):
        sc.submit(blk.cpu())
    sc.submit(blk[:4095])
    assert sc.segments == 0
    with pytest.raises(SondeError, match="segment"):
        sc.spectrum()
    with pytest.raises(SondeError, match="segment"):
        sc.candidates()
    sc.submit(blk[:1])
    assert sc.segments == 1 and np.all(sc.spectrum()[1] == 0.0)
    sc.close()


# ---------------------------------------------------------------- whole scenes, no truth handed over
FS = 10_000_000
N_SCENE = 30_720_000                       # tests/test_gpu_tuner.py's scene
N_SCAN = 1_280_000
N_SURVEY = 20_480_000
CFO_MAX = 300.0                            # synth.make_wideband_scene's default
SCENE = [(-3_512_345, 0, False), (-2_100_777, 1, False), (1_234_567, 2, False), (2_500_003, 3, False), (3_700_111, 3, True),
         (-700_321, 4, False), (150_013, 5, False), (4_200_999, 6, False)]
ORDER = sorted(range(len(SCENE)), key=lambda i: SCENE[i][0])          # candidates come in ascending frequency


def _match(t, m20, f, txs):
    if t == 0:
        return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx[8:], f["data"][8:f["len"]])]
    if t == 3 and m20:
        return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx[:70], f["data"][:70])]
    if t == 5:
        return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx, f["data"][:len(tx)])]
    return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx, f["data"][:f["len"]])]


def _check_frames(got, sondes, frames, symbols, allow_lost=1):
    for i, (_, t, m20) in enumerate(sondes):
        fr = got[got["channel"] == i]
        hit = set()
        for f in fr:
            m = _match(t, m20, f, frames[i])
            assert m, f"sonde {i} (type {t}): a decoded frame matches no transmitted one"
            hit.update(m)
        starts = np.array([p for p, _ in frames[i]])
        period = int(np.median(np.diff(starts))) if len(starts) > 1 else symbols[i]
        complete = [k for k, p in enumerate(starts) if p + period <= symbols[i]]
        lost = len(set(complete) - hit)
        assert len(complete) >= 1 and lost <= allow_lost, (i, t, len(complete), sorted(hit))


def _decode(iq, sondes):
    rx = WidebandReceiver(FS, sondes, chain="iq48", max_in=N_SCENE // 3)
    got = []
    for a in range(0, N_SCENE, rx.max_in):
        rx.submit(iq[a:a + rx.max_in])
        got.append(rx.frames())
    rx.close()
    return np.concatenate(got)


def test_scan_then_decode_every_type():
    """The scanner's offsets are good enough for the decoder (the type still given)."""
    iq, frames, symbols = synth.make_wideband_scene(SCENE, N_SCENE, fs=FS, ebn0_db=20.0, seed=21, device=DEV)
    iq = iq.contiguous()
    sc = SondeScanner(FS, N_SCAN)
    sc.submit(iq[:N_SCAN])
    cand = sc.candidates()
    _same(cand, R.search_ref(sc.spectrum()[1], FS))                    # the search has no tolerance: over the GPU's own spectrum
    par = dict(smooth_hz=5000, min_sep_hz=25000, centroid_hz=12000, threshold=2.5)
    _same(sc.candidates(**par), R.search_ref(sc.spectrum()[1], FS, **par))
    sc.close()
    assert len(cand) == len(SCENE), cand["offset_hz"]
    for c, i in zip(cand, ORDER):
        print(f"type {SCENE[i][1]} m20 {SCENE[i][2]}: offset error {int(c['offset_hz']) - SCENE[i][0]} Hz, bandwidth {c['bandwidth_hz']}, C/N0 {c['cn0_dbhz']:.1f}")
        assert abs(int(c["offset_hz"]) - SCENE[i][0]) <= 500 + CFO_MAX, (c, SCENE[i])
    got = _decode(iq, [(int(c["offset_hz"]), SCENE[i][1]) for c, i in zip(cand, ORDER)])
    _check_frames(got, [SCENE[i] for i in ORDER], [frames[i] for i in ORDER], [symbols[i] for i in ORDER])


@pytest.fixture(scope="module")
def surveyed():
    iq, frames, symbols = synth.make_wideband_scene(SCENE, N_SCENE, fs=FS, ebn0_db=30.0, seed=45, device=DEV)
    iq = iq.contiguous()
    found = survey(iq[:N_SURVEY], FS)
    for r in found:
        print("survey:", r)
    known = [(f, t) for f, t, _, _ in found if t >= 0]
    got = _decode(iq, known) if known else None
    return found, known, got, frames, symbols


def test_survey_finds_eight(surveyed):
    found = surveyed[0]
    assert len(found) == len(SCENE), found
    for (f, t, cn0, bw), i in zip(found, ORDER):
        assert abs(f - SCENE[i][0]) <= 500 + CFO_MAX, (f, SCENE[i])


@pytest.mark.parametrize("k", range(len(SCENE)), ids=[f"type{SCENE[i][1]}{'-m20' if SCENE[i][2] else ''}" for i in ORDER])
def test_survey_then_decode(surveyed, k):
    """The whole flow, no outside knowledge: the k-th result (ascending offset) has the true type, and the receiver built from the
    survey's own list decodes that sonde's frames."""
    found, known, got, frames, symbols = surveyed
    assert len(found) == len(SCENE)
    i = ORDER[k]
    f, t, _, _ = found[k]
    assert t == SCENE[i][1], (found[k], SCENE[i])
    ch = known.index((f, t))
    mine = got[got["channel"] == ch].copy()
    mine["channel"] = 0
    _check_frames(mine, [SCENE[i]], [frames[i]], [symbols[i]])
