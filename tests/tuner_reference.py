"""Float64 / exact-integer reference of the wideband tuner, written from DESIGN.md SPEC 3.9 and nothing else: it imports neither the
oracle nor the product.  Rates and tap counts are integers, the mixer phase is exact integer arithmetic, the prototype and the
filter sums are float64.  The error bound of a comparison is a formula (the float32 rounding of the kernel's summation order plus
the mixer's allowance), not a constant fitted to data.

tuner_ref() takes mutation keywords (the offset's sign flipped, the window one tap off, the wrong phase p, the history dropped at
submit boundaries, the mixer indexed by the in-submit index) so that the tests can show that the bound rejects the bugs it exists
for."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24                   # float32 unit roundoff
MIXER_ERR = 2.0 ** -22           # SPEC 3.9: the complex exponential's error per component
LANES = 64                       # the kernel's summation order (SPEC 3.9 "Kernel"): 64 chains of ceil(T / 64) taps, then a 6-level tree


def ratio(fs: int, r: int) -> tuple[int, int]:
    """up / down = R / Fs in lowest terms; ValueError for what SPEC 3.9 refuses"""
    if not (1_000_000 <= fs <= 20_000_000):
        raise ValueError("Fs out of range")
    if not (0 < r <= 100_000) or 8 * r > fs:
        raise ValueError("R out of range")
    g = math.gcd(fs, r)
    up, down = r // g, fs // g
    if up > 64:
        raise ValueError("up > 64")
    return up, down


def taps_per_phase(fs: int, b: int) -> int:
    return 32 * -(-fs // b)


def prototype(fs: int, r: int, b: int) -> np.ndarray:
    """the float64 Blackman-windowed sinc of SPEC 3.7 with N = up T taps, cutoff B / 2 at Fs up"""
    up, _ = ratio(fs, r)
    N = up * taps_per_phase(fs, b)
    fc = 0.5 * b / (float(fs) * up)
    i = np.arange(N, dtype=np.float64)
    t = i - 0.5 * (N - 1)
    x = i / (N - 1)
    w = 0.42 - 0.5 * np.cos(2.0 * np.pi * x) + 0.08 * np.cos(4.0 * np.pi * x)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 2.0 * fc, np.sin(2.0 * np.pi * fc * t) / (np.pi * t))
    return s * w


def taps64(fs: int, r: int, b: int) -> np.ndarray:
    """g[p][t] = h[t up + p] / sum_t h[t up + p] in float64: [up, T]"""
    up, _ = ratio(fs, r)
    h = prototype(fs, r, b).reshape(-1, up).T          # [p][t] = h[t up + p]
    return h / h.sum(axis=1, keepdims=True)


def response_db(g: np.ndarray, fs: int, freqs_hz: np.ndarray) -> np.ndarray:
    """|H(f)| in dB of the prototype rebuilt from per-phase taps g [up, T] (at rate Fs up, divided by up: 0 dB at DC)"""
    up, T = g.shape
    h = np.asarray(g, np.float64).T.reshape(-1)                     # h[t up + p]
    nfft = 1 << int(math.ceil(math.log2(max(4 * len(h), 1 << 16))))
    H = np.abs(np.fft.rfft(h, nfft)) / up
    f = np.arange(len(H)) * (float(fs) * up / nfft)
    return 20.0 * np.log10(np.maximum(np.interp(np.abs(freqs_hz), f, H), 1e-30))


def phase(f_hz: int, n: np.ndarray, fs: int, start: int = 0) -> np.ndarray:
    """phi(n) = (f (start + n)) mod Fs, exact at any stream age: n and start are reduced mod Fs in integers BEFORE anything is added
    or multiplied (start as a Python integer, so that it may be 2^62 and beyond), both factors are then below Fs <= 2e7 and the
    product fits 64-bit integers with room to spare"""
    fs = int(fs)
    n_mod = (np.asarray(n, np.int64) % fs + np.int64(int(start) % fs)) % fs
    return (np.int64(int(f_hz) % fs) * n_mod) % fs


def tuner_ref(x: np.ndarray, fs: int, r: int, g: np.ndarray, offsets, submits, *, j_range=None,
              flip_sign=False, tap_shift=0, phase_shift=0, drop_history=False, local_mixer=False, start: int = 0, thetas=None):
    """SPEC 3.9 for one VFO.  x: the whole stream (complex, absolute index 0 ..), g: [up, T] taps (float64 values), offsets: one
    offset per submit (a retune applies from the submit on), submits: the n_in of each submit.  Returns (y, A): the outputs of the
    submits (or those with absolute index in j_range) and A = sum_t |g| (|Re x| + |Im x|) per output (for the error bound).
    start (a multiple of down): x[0] has the absolute index `start` and the stream before it is silence; everything but the mixer's
    phase is relative to it (start up / down is an integer, so the filter phase (j down) mod up is that of the relative index), and
    j_range counts from it.  thetas: the mixer's phase offset of each submit (a continuous retune's theta; default zeros)."""
    up, down = ratio(fs, r)
    assert int(start) % down == 0 and start >= 0
    thetas = [0] * len(submits) if thetas is None else thetas
    T = g.shape[1]
    x = np.asarray(x, np.complex128)
    ys, As, n_base = [], [], 0
    for f, n_in, theta in zip(offsets, submits, thetas):
        assert n_in % down == 0
        f = -f if flip_sign else f
        lo = max(0, n_base - (T - 1) - abs(tap_shift))
        idx = np.arange(lo, n_base + n_in)
        ph = (phase(f, idx - n_base, fs) if local_mixer else phase(f, idx, fs, start)) + np.int64(int(theta) % fs)
        v = x[lo:n_base + n_in] * np.exp(-2j * np.pi * ph.astype(np.float64) / fs)
        if drop_history:
            v[idx < n_base] = 0.0
        ax = np.abs(x[lo:n_base + n_in].real) + np.abs(x[lo:n_base + n_in].imag)
        j0, j1 = n_base * up // down, (n_base + n_in) * up // down
        js = np.arange(j0, j1)
        if j_range is not None:
            js = js[(js >= j_range[0]) & (js < j_range[1])]
        for j in js:
            p = (j * down) % up
            i0 = (j * down) // up
            pp = (p + phase_shift) % up
            s = i0 - np.arange(T) - tap_shift - lo          # v index of x[i0 - t]
            ok = s >= 0
            vv = np.where(ok, v[np.clip(s, 0, None)], 0.0)
            ys.append(np.dot(g[pp], vv))
            As.append(np.dot(np.abs(g[p]), np.where(ok, ax[np.clip(s, 0, None)], 0.0)))
        n_base += n_in
    return np.array(ys), np.array(As)


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def bound(A: np.ndarray, T: int) -> np.ndarray:
    """per-component bound of |product - reference| for outputs with sum_t |g| |x|_1 = A: the kernel sums each output in 64 fmaf
    chains of ceil(T / 64) taps and a 6-level tree (gamma_n with n = ceil(T / 64) + 6, the sequential chain's gamma_T at most), on
    mixed samples whose error per component is at most |x|_1 (2^-22 + 2u) (the phasor's allowance plus two roundings)"""
    eps = MIXER_ERR + 2.0 * U
    return A * (gamma(-(-T // LANES) + 6) * (1.0 + eps) + eps)
