"""Float64 reference of the band scanner, written from DESIGN.md SPEC 3.10 and nothing else: it imports neither the oracle nor the
product.  The spectrum is numpy's float64 FFT of each windowed segment, segments taken by absolute index; the search is the text of
SPEC 3.10 step by step, every sum in ascending order in double (cumsum and explicit loops: numpy's pairwise sum would not be the
SPEC's order).  The error bound of a spectrum comparison is a formula (below), not a constant fitted to data.

spectrum_ref() takes mutation keywords (a rectangular window, segments one sample late, one segment dropped, the frequency axis
mirrored) so that the tests can show that the bound rejects the bugs it exists for."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24                   # float32 unit roundoff
DEFAULTS = dict(smooth_hz=8000, min_sep_hz=10000, centroid_hz=16000, threshold=4.0)


def auto_fft_size(fs: int) -> int:
    """the smallest power of two in 1024 .. 16384 with Fs / N <= 1000 Hz, else 16384"""
    if not (1_000_000 <= fs <= 20_000_000):
        raise ValueError("Fs out of range")
    n = 1024
    while n < 16384 and fs > 1000 * n:
        n *= 2
    return n


def window(n: int) -> np.ndarray:
    """periodic Hann: w[i] = (float)(0.5 - 0.5 cos(2 pi i / N)), the cosine in double"""
    i = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / n)).astype(np.float32)


def n_segments(n: int, N: int) -> int:
    return 0 if n < N else (n - N) // (N // 2) + 1


def spectrum_ref(x: np.ndarray, fs: int, N: int, cuts=None, *, rect_window=False, shift=0, drop_segment=None, mirror=False):
    """SPEC 3.10 "Spectrum" in float64.  x: the whole stream since create / reset (complex), cuts: the n_in of the submits (only
    their sum counts: the spectrum does not depend on where the stream was cut).  Returns (P, S, norms): P[i] in ascending frequency
    (bin i <-> (i - N / 2) Fs / N), the number of segments, and ||w x_s||_2 per segment (for spectrum_bound)."""
    x = np.asarray(x, np.complex128)
    n = len(x) if cuts is None else int(sum(cuts))
    assert n <= len(x)
    S = n_segments(n, N)
    w = np.ones(N) if rect_window else window(N).astype(np.float64)
    A = np.zeros(N)
    norms = []
    used = 0
    for s in range(S):
        a = s * (N // 2) + shift
        if a + N > len(x) or s == drop_segment:
            continue
        y = w * x[a:a + N]
        X = np.fft.fft(y)
        A += X.real * X.real + X.imag * X.imag
        norms.append(math.sqrt(float(np.sum(y.real * y.real + y.imag * y.imag))))
        used += 1
    P = np.roll(A / max(used, 1), N // 2)           # P[(k + N / 2) mod N] = A[k] / S
    if mirror:
        P = P[::-1].copy()
    return P, S, np.array(norms)


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def spectrum_bound(P_ref: np.ndarray, N: int, norms: np.ndarray) -> np.ndarray:
    """Per-bin bound of |P_float32_pipeline - P_ref| for a pipeline that follows SPEC 3.10 in float32.

    One segment, y = w x its windowed samples (exact), X = FFT(y) (exact), p = |X|^2:
      * the window product is one rounding per component, and the stored window may be one float32 ulp off the SPEC's (a cosine a
        last place apart): y^ = y + dy, |dy_n| <= 2u |y_n|, so every bin of FFT(dy) is at most 2u ||y||_1 <= 2u sqrt(N) ||y||_2;
      * the transform: a radix-2 FFT of t = log2 N stages with twiddles of absolute error mu computes X^ with
        ||X^ - X||_2 <= t eta / (1 - t eta) ||X||_2, eta = mu + gamma_4 (sqrt 2 + mu) (Higham, Accuracy and Stability of Numerical
        Algorithms, 2nd ed., theorem 24.2), and ||X||_2 = sqrt(N) ||y||_2.  Twiddles made in double and stored as float have
        mu <= 2u.  A radix-4 stage is two radix-2 levels of additions with one twiddle product between them, so t = log2 N covers
        it (a radix-2 stage more where log2 N is odd).  One bin's error is at most the 2-norm of all of them:
            |X^_k - X_k| <= e_s = (t eta / (1 - t eta) + 2u (1 + t eta)) sqrt(N) ||y_s||_2
      * the power: p^ = fmaf(re, re, im im) has two roundings, |p^ - |X^|^2| <= gamma_2 |X^|^2, and
        | |X^|^2 - |X|^2 | <= 2 |X_k| e_s + e_s^2.
    The mean over the S segments, by Cauchy-Schwarz (mean_s |X_sk| e_s <= sqrt(mean_s |X_sk|^2) sqrt(mean_s e_s^2)):
            |P^ - P| <= (1 + gamma_2) (2 sqrt(P_ref[k]) e_rms + e_rms^2) + (gamma_2 + u + S 2^-53) P_ref[k]
    with e_rms^2 = mean_s e_s^2; u is the final rounding to float32, S 2^-53 the S additions and the division in double.  The
    formula holds N, the unit roundoff, the segments' norms and the reference spectrum: nothing measured from an implementation."""
    t = int(round(math.log2(N)))
    mu = 2.0 * U
    eta = mu + gamma(4) * (math.sqrt(2.0) + mu)
    c = t * eta / (1.0 - t * eta) + 2.0 * U * (1.0 + t * eta)
    e2 = float(np.mean((c * math.sqrt(N) * np.asarray(norms, np.float64)) ** 2))
    S = len(norms)
    P = np.asarray(P_ref, np.float64)
    return (1.0 + gamma(2)) * (2.0 * np.sqrt(P * e2) + e2) + (gamma(2) + U + (S + 1) * 2.0 ** -53) * P


def _rnd(x: float) -> float:
    return math.floor(x + 0.5)


def search_ref(P, fs: int, **params):
    """SPEC 3.10 "Search", steps 1-6, over the float32 spectrum P in ascending frequency.  Returns a list of dicts (bin, offset_hz,
    bandwidth_hz, cn0_dbhz, excess_db) in ascending bin order.  threshold travels as a float32 (the ABI's field)."""
    par = dict(DEFAULTS)
    par.update({k: v for k, v in params.items() if v})
    P = np.asarray(P, np.float32).astype(np.float64)
    N = len(P)
    thr = float(np.float32(par["threshold"]))
    delta = float(fs) / N
    h = max(1, int(_rnd(par["smooth_hz"] / (2.0 * delta))))
    W = 2 * h + 1
    g = max(1, int(_rnd(par["centroid_hz"] / (2.0 * delta))))
    D = max(1, int(_rnd(par["min_sep_hz"] / delta)))
    c = np.concatenate([[0.0], np.cumsum(P)])                    # sequential: c[j + 1] = c[j] + P[j]
    Sm = np.full(N, -np.inf)
    idx = np.arange(h, N - h)
    Sm[idx] = c[idx + h + 1] - c[idx - h]
    v = np.sort(Sm[h:N - h])
    m = len(v)
    floor = float(v[m // 2]) if m & 1 else (float(v[m // 2 - 1]) + float(v[m // 2])) / 2.0
    n0 = floor / W
    out = []
    e0 = max(h, g)
    for i in range(e0, N - 1 - e0 + 1):
        if not Sm[i] >= thr * floor:
            continue
        a, b = max(h, i - D), min(N - 1 - h, i + D)
        if int(np.argmax(Sm[a:b + 1])) + a != i:                 # argmax: the first index of the maximum
            continue
        se = sj = 0.0
        for j in range(i - g, i + g + 1):
            e = float(P[j]) - n0
            se += e
            sj += e * j
        if not se > 0.0:
            continue
        cen = sj / se
        a, b = max(0, i - D), min(N - 1, i + D)
        q = [max(float(P[j]) - n0, 0.0) for j in range(a, b + 1)]
        E = 0.0
        for t in q:
            E += t
        run, j05, j95 = 0.0, None, None
        for j, t in zip(range(a, b + 1), q):
            run += t
            if j05 is None and run >= 0.05 * E:
                j05 = j
            if j95 is None and run >= 0.95 * E:
                j95 = j
        out.append(dict(bin=i, offset_hz=int(_rnd((cen - N // 2) * delta)), bandwidth_hz=int(_rnd((j95 - j05 + 1) * delta)),
                        cn0_dbhz=float(np.float32(10.0 * math.log10(E * delta / n0))),
                        excess_db=float(np.float32(10.0 * math.log10(Sm[i] / floor)))))
    return out


# ---------------------------------------------------------------- the streams of the spectrum tests (CPU and GPU use the same ones)
# (Fs, N (0 = auto), input kind name, submits): ragged, one shorter than N / 2, one of a single sample
SPECTRUM_CASES = [
    (10_000_000, 16384, "iq", [300_000, 1, 5_000, 131_072, 250_001, 40_000]),
    (10_000_000, 8192, "iq16", [100_000, 1, 3_000, 65_536, 200_001]),
    (2_400_000, 0, "iq8", [50_000, 1, 2_000, 32_768, 90_001]),
    (20_000_000, 16384, "iq", [1, 400_000, 8_000, 300_001]),
    (2_048_000, 1024, "iq", [20_000, 1, 500, 4_096, 30_001]),
]
PEAK = {"iq": 30000.0, "iq16": 30000.0, "iq8": 120.0}
TONES_DB = (40.0, 43.0, 46.0)          # above the per-bin noise floor of the windowed transform


def make_stream(fs: int, N: int, kind: str, n: int, seed: int, burst: bool = False) -> np.ndarray:
    """integer-valued complex samples (exact in every input kind): white noise plus three tones 40, 43 and 46 dB above the per-bin
    floor, the first two within a bin of the band's lower and upper edge.  burst: a fourth tone of the strongest one's amplitude, on
    the centre of an odd bin and keyed on for the first half of every N / 2 samples: a signal whose spectrum depends on where the
    segments lie (its two bursts per segment meet in opposite phase, so that the Hann window's overlap-add does not cancel a shift)."""
    rng = np.random.default_rng(seed)
    delta = fs / N
    freqs = (-fs / 2 + 0.6 * delta, fs / 2 - 0.7 * delta, 0.1234 * fs)
    # per-bin floor of noise with variance 2 sn^2: 2 sn^2 sum w^2 = 2 sn^2 3N/8; a tone of amplitude A on a bin: A^2 (N/2)^2
    rel = [math.sqrt(2.0 * 1.5 * 10.0 ** (db / 10.0) / N) for db in TONES_DB]          # A / sn
    extra = rel[2] if burst else 0.0
    sn = math.floor(PEAK[kind] / (4.5 + sum(rel) + extra))
    assert sn >= 3
    t = np.arange(n, dtype=np.float64)
    x = sn * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for r, f in zip(rel, freqs):
        x = x + sn * r * np.exp(2j * np.pi * (f * t / fs + rng.uniform()))
    if burst:
        on = (np.arange(n) % (N // 2)) < N // 4
        x = x + on * sn * extra * np.exp(2j * np.pi * ((-2 * (N // 7) + 1) * t / N + rng.uniform()))
    lim = 127.0 if kind == "iq8" else 32767.0
    return np.clip(np.round(x.real), -lim, lim) + 1j * np.clip(np.round(x.imag), -lim, lim)
