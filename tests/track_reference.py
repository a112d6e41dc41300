"""Float64 reference of the carrier meter, the tracking step and the continuous retune, written from DESIGN.md SPEC 3.11 and the
amended SPEC 3.9 and nothing else: it imports neither the product nor its kernels (the decoder of the whole-receiver reference is
the CPU oracle).  The meter's error bound is a formula (the float32 roundings of the kernel's summation order), not a constant
fitted to data; meter_ref() takes mutation keywords (lag off by one, looks one block late, a dropped block, the conjugate on the
wrong factor) so that the tests can show that the bound rejects the bugs it exists for."""
from __future__ import annotations

import math

import numpy as np

import tuner_reference as R

U = 2.0 ** -24                   # float32 unit roundoff
BLK = 256
DEADBAND_HZ, MAX_STEP_HZ = 400, 4000          # SPEC 3.11 defaults
VFO_RATE = {0: 10000, 1: 15000, 2: 20000, 3: 50000, 4: 20000, 5: 20000, 6: 20000}     # the reference's VFO bandwidth per type
IQ48_MAX_BW = 40000


def defaults(rate: int) -> tuple[int, int]:
    """(L, d) of SPEC 3.11: L = 256 ceil(R / 2560), d = max(1, R div 24000)"""
    return BLK * -(-rate // 2560), max(1, rate // 24000)


# ---------------------------------------------------------------- the meter
def _terms(x: np.ndarray, d: int, conj_wrong: bool = False):
    """per sample m (from the restart): c[m] = x[m] conj(x[m - d]) (x[m < 0] = 0), p[m] = |x[m]|^2, and the magnitudes the bound needs"""
    x = np.asarray(x, np.complex128)
    y = np.concatenate([np.zeros(d, np.complex128), x[:len(x) - d]]) if d else x
    c = (np.conj(x) * y) if conj_wrong else (x * np.conj(y))
    m_re = np.abs(x.real * y.real) + np.abs(x.imag * y.imag)
    m_im = np.abs(x.imag * y.real) + np.abs(x.real * y.imag)
    return c, x.real ** 2 + x.imag ** 2, m_re, m_im


def meter_ref(x: np.ndarray, L: int, d: int, *, lag_shift=0, late_blocks=0, drop_block=None, conj_wrong=False):
    """Every finished look of one row that starts (create or restart) at x[0].  Returns (A [K] complex, P [K], M [K, 3]): M = the sums of
    |products| per look for (Re A, Im A, P), which bound() scales."""
    c, p, m_re, m_im = _terms(x, d + lag_shift, conj_wrong)
    if drop_block is not None:
        s = slice(drop_block * BLK, (drop_block + 1) * BLK)
        c = c.copy(); p = p.copy()
        c[s] = 0.0; p[s] = 0.0
    o = late_blocks * BLK
    K = (len(c) - o) // L
    A = np.array([c[o + k * L:o + (k + 1) * L].sum() for k in range(K)])
    P = np.array([p[o + k * L:o + (k + 1) * L].sum() for k in range(K)])
    M = np.array([[m_re[o + k * L:o + (k + 1) * L].sum(), m_im[o + k * L:o + (k + 1) * L].sum(), p[o + k * L:o + (k + 1) * L].sum()]
                  for k in range(K)]).reshape(K, 3)
    return A, P, M


def gamma(n: int, u: float = U) -> float:
    return n * u / (1.0 - n * u)


def bound(M: np.ndarray, L: int) -> np.ndarray:
    """|kernel - float64 sum| per look and quantity, for sums of |products| M.  A product is one rounded multiplication inside one
    fmaf (two roundings: gamma_2 of its two terms' magnitudes); a sample's product then passes through 3 additions in its lane and 6
    butterfly levels (gamma_9): gamma_11 of the block's magnitude in all.  The block sums are exact as doubles and are added in
    L / 256 double additions (at most (L / 256) 2^-53 of the magnitudes, themselves (1 + gamma_11) larger at most); the reference's own
    double sum (numpy's pairwise one over L <= 2^22 terms, and the roundings of its products) is allowed 32 * 2^-53."""
    lb = L // BLK
    return np.asarray(M) * (gamma(11) + (lb * (1.0 + gamma(11)) + 32.0) * 2.0 ** -53)


class Meter:
    """the streaming form: feed() rows piece by piece, restart() as SPEC 3.11; looks() returns the (index, A, P) finished since the last call"""

    def __init__(self, rate: int, L: int = 0, d: int = 0):
        L0, d0 = defaults(rate)
        self.rate, self.L, self.d = rate, L or L0, d or d0
        self.restart()

    def restart(self):
        self.buf = np.zeros(0, np.complex128)
        self.done = 0
        self.out = []

    def feed(self, y: np.ndarray):
        self.buf = np.concatenate([self.buf, np.asarray(y, np.complex128)])
        K = len(self.buf) // self.L
        if K > self.done:
            A, P, _ = meter_ref(self.buf[:K * self.L], self.L, self.d)
            self.out += [(k, A[k], P[k]) for k in range(self.done, K)]
            self.done = K

    def looks(self):
        o, self.out = self.out, []
        return o


# ---------------------------------------------------------------- host conversions and the step rule
def err_hz(rate: int, d: int, a: complex) -> float:
    return rate / (2.0 * math.pi * d) * math.atan2(a.imag, a.real)


def level_db(p: float, L: int) -> float:
    return 10.0 * math.log10(p / L)


def quality(a: complex, p: float) -> float:
    return math.hypot(a.real, a.imag) / p if p > 0.0 else 0.0


def step_ref(offset_hz: int, bw: int, fs: int, rate: int, d: int, a: complex, deadband_hz: float = DEADBAND_HZ,
             max_step_hz: float = MAX_STEP_HZ) -> int:
    """SPEC 3.11's rule: hold inside the deadband; else step by rnd(err), the step clamped to +- max_step, the result to the band"""
    e = err_hz(rate, d, a)
    if abs(e) < deadband_hz:
        return offset_hz
    s = min(max(math.floor(e + 0.5), -max_step_hz), max_step_hz)
    lim = (fs - bw) // 2
    return int(min(max(offset_hz + int(s), -lim), lim))


# ---------------------------------------------------------------- the tuner with theta (SPEC 3.9 as amended)
class Tuner:
    """One VFO of SPEC 3.9 over the whole stream x (complex, absolute index 0 ..): phi(n) = (f n + theta) mod Fs in exact integers.
    g: [up, T] taps (float64 values).  process(n_in) returns the submit's outputs (and, with want_A, A = sum_t |g| |x|_1 per output for
    tuner_reference.bound)."""

    def __init__(self, x: np.ndarray, fs: int, r: int, g: np.ndarray, offset_hz: int):
        self.x = np.asarray(x, np.complex128)
        self.fs, self.r, self.g = int(fs), int(r), np.asarray(g, np.float64)
        self.up, self.down = R.ratio(fs, r)
        self.T = self.g.shape[1]
        self.f, self.theta, self.n_base = int(offset_hz), 0, 0

    def retune(self, f: int, continuous: bool = False):
        if continuous:
            fs = self.fs
            self.theta = (self.theta + ((self.f - int(f)) % fs) * ((self.n_base - self.T // 2) % fs)) % fs
        else:
            self.theta = 0
        self.f = int(f)

    def process(self, n_in: int, want_A: bool = False):
        fs, up, down, T = self.fs, self.up, self.down, self.T
        assert n_in % down == 0
        n0, n1 = self.n_base, self.n_base + n_in
        lo = n0 - (T - 1)                                     # the window's first absolute index (may be negative: v = 0 there)
        idx = np.arange(max(lo, 0), n1, dtype=np.int64)
        ph = (((self.f % fs) * (idx % fs)) % fs + self.theta) % fs
        xs = self.x[max(lo, 0):n1]
        v = np.zeros(n1 - lo, np.complex128)
        v[max(lo, 0) - lo:] = xs * np.exp(-2j * np.pi * ph.astype(np.float64) / fs)
        ax = None
        if want_A:
            ax = np.zeros(n1 - lo)
            ax[max(lo, 0) - lo:] = np.abs(xs.real) + np.abs(xs.imag)
        j0, j1 = n0 * up // down, n1 * up // down
        y = np.zeros(j1 - j0, np.complex128)
        A = np.zeros(j1 - j0) if want_A else None
        for j_first in range(j0, min(j0 + up, j1)):           # one pass per filter phase: j = j_first + up k, i0 = i0_first + down k
            p = (j_first * down) % up
            i0 = (j_first * down) // up
            K = len(range(j_first, j1, up))
            start = i0 - (T - 1) - lo                         # v index of x[i0 - (T - 1)]
            W = np.lib.stride_tricks.as_strided(v[start:], shape=(K, T), strides=(down * v.strides[0], v.strides[0]))
            y[j_first - j0::up] = W @ self.g[p][::-1]
            if want_A:
                Wa = np.lib.stride_tricks.as_strided(ax[start:], shape=(K, T), strides=(down * ax.strides[0], ax.strides[0]))
                A[j_first - j0::up] = Wa @ np.abs(self.g[p][::-1])
        self.n_base = n1
        return (y, A) if want_A else y


# ---------------------------------------------------------------- a whole tracked receiver
def receiver_ref(x: np.ndarray, fs: int, vfos, n_sub: int, *, track: bool, taps=None, deadband_hz: float = DEADBAND_HZ,
                 max_step_hz: float = MAX_STEP_HZ, look_samples: int = 0):
    """vfos: [(offset_hz, rate R, bandwidth B), ...] over the stream x, in submits of n_sub samples.  The loop of SPEC 3.11: the rows of
    every submit are metered; at the start of the next submit the newest finished look of each VFO goes through step_ref(), and a
    VFO that moved is retuned continuously and its meter restarted.  Returns (rows: one complex128 row per VFO, log: per VFO a list of
    (first input sample of the submit the offset applies from, offset_hz, err_hz, level_db), retunes: per VFO the count)."""
    tun, met = [], []
    for f, r, b in vfos:
        g = taps(fs, r, b) if taps else R.taps64(fs, r, b)
        tun.append(Tuner(x, fs, r, g, f))
        met.append(Meter(r, look_samples))
    rows = [[] for _ in vfos]
    log = [[] for _ in vfos]
    retunes = [0] * len(vfos)
    for s in range(len(x) // n_sub):
        for k, (tu, me) in enumerate(zip(tun, met)):
            if track and s:
                lk = me.looks()
                if lk:
                    _, a, p = lk[-1]
                    new = step_ref(tu.f, vfos[k][2], fs, tu.r, me.d, a, deadband_hz, max_step_hz)
                    if new != tu.f:
                        tu.retune(new, continuous=True)
                        me.restart()
                        retunes[k] += 1
                    log[k].append((s * n_sub, new, err_hz(tu.r, me.d, a), level_db(p, me.L)))
            y = tu.process(n_sub)
            me.feed(y)
            rows[k].append(y)
    return [np.concatenate(r) for r in rows], log, retunes


def iq48_vfos(sondes):
    """the iq48 chain's VFOs for [(offset_hz, type), ...]: R = 48 kHz, B = the type's VFO rate (40 kHz at most)"""
    return [(int(f), 48000, min(VFO_RATE[int(t)], IQ48_MAX_BW)) for f, t in sondes]


def reference_vfos(sondes):
    """the reference chain's VFOs: R = B = the type's VFO rate"""
    return [(int(f), VFO_RATE[int(t)], VFO_RATE[int(t)]) for f, t in sondes]


def decode_rows(rows, types):
    """the CPU oracle over 48 kHz complex rows, one row per sonde: frames (FRAME_DTYPE) with channel = the sonde's index"""
    import oracle_lib
    out = []
    for i, (y, t) in enumerate(zip(rows, types)):
        n = len(y) // 2048 * 2048
        iq = np.stack([y.real[:n], y.imag[:n]], axis=1).astype(np.float32)[None]
        fr = oracle_lib.batch_run(int(t), iq)
        fr["channel"] = i
        out.append(fr)
    return np.concatenate(out)


def match(t: int, f, txs):
    """indices of the transmitted frames (symbol offset, bytes) a decoded frame equals, by payload"""
    if t == 0:
        return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx[8:], f["data"][8:f["len"]])]
    return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx, f["data"][:f["len"]])]


def tally(got, types, frames, symbols, tail_from: float = 0.0):
    """per sonde (frames sent whole, of those decoded, frames sent whole that start in the stream's part from `tail_from` on, of those
    decoded, decoded frames that match no transmitted one)"""
    out = []
    for i, t in enumerate(types):
        hit, stray = set(), 0
        for f in got[got["channel"] == i]:
            m = match(int(t), f, frames[i])
            stray += not m
            hit.update(m)
        starts = np.array([p for p, _ in frames[i]])
        period = int(np.median(np.diff(starts))) if len(starts) > 1 else symbols[i]
        whole = [k for k, p in enumerate(starts) if p + period <= symbols[i]]
        tail = [k for k in whole if starts[k] >= tail_from * symbols[i]]
        out.append((len(whole), len(set(whole) & hit), len(tail), len(set(tail) & hit), stray))
    return out
