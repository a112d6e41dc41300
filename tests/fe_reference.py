"""Float64 reference of the two front-ends, written from DESIGN.md section 3 (SPEC 3.1, 3.5, 3.5b, 3.5c, 3.7) and nothing else: it
imports neither the oracle nor the product and loads no table from either; every tap and twiddle is computed here from its
definition.  The product's and the oracle's float32 arithmetic is compared with it under error bounds that are formulas (the
float32 rounding of the stages the SPEC prescribes), not constants fitted to data, so a comparison keeps its meaning when a
kernel stops being bit-exact to the oracle.

Two layers:
  tight -- the SPEC's own atan2q (SPEC 3.1) evaluated in float64: what remains is float32 rounding;
  loose -- np.arctan2 with SPEC 3.1's documented approximation error on top: the approximant is the one SPEC 3.1 names.

Every `*_ref` function takes mutation keywords (a prototype shifted one tap, a history one sample short, a conjugated twist,
i0 - 1, p +- 1, ...) so that the tests can show that the bounds reject the bugs they exist for."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24                   # float32 unit roundoff

# ---------------------------------------------------------------- SPEC 3.5: the wideband filter bank
FS = 10e6                        # wideband rate
M = 512                          # bins (spacing 19 531.25 Hz)
D = 500                          # decimation: 20 kS/s per bin
T = 16                           # prototype taps per bin
L = M * T                        # 8192-tap prototype
HIST = L - D                     # 7692 wideband samples carried from block to block
STEPS = 2560                     # steps per block (1 280 000 wideband samples)
BIN_HZ = FS / M

# ---------------------------------------------------------------- SPEC 3.1: atan2q
# DESIGN.md section 3.1 (the atan2q paragraph): the seed constant, the floor F and the three coefficients of the odd minimax polynomial of (2/pi) atan
# (float32 values; they are used exactly as float32 holds them).
SEED = 0x7EF311C7
F_FLOOR = float(np.float32(6.9721523e-31))
AT_C1 = float(np.float32(0.6332877278327942))
AT_C3 = float(np.float32(-0.18171308934688568))
AT_C5 = float(np.float32(0.04842534288764))
# |atan2q pi/2 - atan2| <= 2e-3 rad, in quadrants
ATAN2Q_MAX_ERR = 2e-3 * 2.0 / math.pi

# ---------------------------------------------------------------- SPEC 3.7: VFO rates
VFO_RATES = (10000, 15000, 20000, 40000, 50000)


def blackman_sinc(n: int, fc: float) -> np.ndarray:
    """Blackman-windowed sinc of n taps, cutoff fc (cycles per sample), centred at (n - 1) / 2; not normalised."""
    t = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    return 2.0 * fc * np.sinc(2.0 * fc * t) * np.blackman(n)


def proto(shift: int = 0) -> np.ndarray:
    """SPEC 3.5: the filter bank's prototype, 8192 taps, 8 kHz cutoff at 10 MS/s, unit DC gain.
    shift (mutation): the taps moved by that many places."""
    h = blackman_sinc(L, 8000.0 / FS)
    h /= h.sum()
    if shift:
        h = np.roll(h, shift)
        if shift > 0:
            h[:shift] = 0.0
        else:
            h[shift:] = 0.0
    return h


def twiddles() -> np.ndarray:
    """exp(-2 pi i k / 512), k < 256 (complex128)."""
    return np.exp(-2j * np.pi * np.arange(M // 2) / M)


def vfo_ratio(rate: int):
    """SPEC 3.7: up / down = 48000 / R in lowest terms, cutoff 0.45 min(R, 48000) Hz."""
    g = math.gcd(48000, rate)
    return 48000 // g, rate // g, 0.45 * min(rate, 48000)


def resamp_taps(rate: int, cutoff_hz: float | None = None) -> np.ndarray:
    """SPEC 3.7 (and 3.5's 12/5 stage = rate 20000): g[p][t] = proto[up t + p], prototype of 16 up taps at R up, every phase
    normalised to unit DC gain.  [up, 16] float64.  cutoff_hz (mutation): another cutoff."""
    up, _, fc = vfo_ratio(rate)
    if cutoff_hz is not None:
        fc = cutoff_hz
    h = blackman_sinc(16 * up, fc / (rate * up))
    g = h.reshape(16, up).T.copy()                 # g[p][t] = h[up t + p]
    return g / g.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------- atan2q (SPEC 3.1) in float64
def atan2q_ref(y, x) -> np.ndarray:
    """SPEC 3.1 evaluated in float64: s = max(|x| + |y|, F), d = s - 2|y|, rc = the integer seed 0x7EF311C7 - bits(s) on the
    float32 bits of s, one Newton step, r = d rc, q = 1/2 - r (C1 + C3 r^2 + C5 r^4), x negative (sign bit): 2 - q, the sign
    bit of y.  Signed zeros count: atan2q(+-0, -0) = +-2, atan2q(0, 0) = 0."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    ax, ay = np.abs(x), np.abs(y)
    s = np.maximum(ax + ay, F_FLOOR)
    d = s - 2.0 * ay
    seed = (np.uint32(SEED) - s.astype(np.float32).view(np.uint32)).view(np.float32).astype(np.float64)
    rc = seed + seed * (1.0 - s * seed)
    r = d * rc
    t = r * r
    q = 0.5 - ((AT_C5 * t + AT_C3) * t + AT_C1) * r
    q = np.where(np.signbit(x), 2.0 - q, q)
    return np.where(np.signbit(y), -q, q)


def _slope_bound() -> float:
    """Largest d atan2q / d angle (quadrants per quadrant) over the first quadrant: the polynomial's slope against (2/pi) atan's
    along r = (cos - sin) / (cos + sin), times the Newton step's at most 1 + 0.26 %."""
    r = np.linspace(-1.0, 1.0, 200001)
    dp = AT_C1 + 3.0 * AT_C3 * r * r + 5.0 * AT_C5 * r ** 4
    return float(np.max(dp / (2.0 / math.pi / (1.0 + r * r)))) * 1.0026


KAPPA = _slope_bound()
# float32 evaluation of atan2q (s, d, the Newton step, r, r^2, two polynomial fmaf, q, 2 - q: about 8 roundings, each at most
# one unit of 2^-24 of a quantity <= 1 quadrant times a slope <= 1) against the float64 one on the same operands
ATAN2Q_EVAL_ERR = 8.0 * U * 2.0


# ---------------------------------------------------------------- the filter bank in closed form
def bank(x: np.ndarray, odd: bool = False, *, h: np.ndarray | None = None, hist: int = HIST, twist: int = -1, chunk: int = 256):
    """SPEC 3.5 / 3.5c in closed form.  x: the whole stream (complex, from its first sample).  Step m reads
    x[500 m - hist ... 500 m - hist + 8192) (zeros before the stream) and
        Y_k[m] = sum_i h[i] x[n0 + i] exp(-j 2 pi k (i + 500 m) / 512),   n0 = 500 m - hist
    (the fold, the rotation by 500 m and the FFT of the SPEC in closed form).  odd: the same bank on x[n] exp(-j pi n / 512),
    times exp(-j pi 7692 / 512), times the step's exp(+j (125 / 64) (pi / 2) m) -- the value whose atan2q the SPEC rounds
    BEFORE it takes 32000 m off in integers (see phases_ref).
    Returns (Y [512, n_steps] complex128, A [n_steps] = sum_i |h_i| |x[n0 + i]|, the scale of every float32 rounding).
    Mutations: h (another prototype), hist (another history length), twist = +1 (the odd bank's shift conjugated)."""
    h = proto() if h is None else h
    x = np.asarray(x, dtype=np.complex128)
    n_steps = x.shape[0] // D
    if odd:
        x = x * np.exp(twist * 1j * np.pi * (np.arange(x.shape[0]) % (2 * M)) / M)
    xp = np.concatenate([np.zeros(hist, np.complex128), x, np.zeros(L, np.complex128)])
    ah = np.abs(h).reshape(T, M)
    hf = h.reshape(T, M)
    k = np.arange(M)
    Y = np.empty((M, n_steps), np.complex128)
    A = np.empty(n_steps)
    for m0 in range(0, n_steps, chunk):
        m1 = min(n_steps, m0 + chunk)
        w = np.lib.stride_tricks.as_strided(xp[m0 * D:], shape=(m1 - m0, T, M), strides=(D * 16, M * 16, 16))
        v = np.einsum("mtr,tr->mr", w, hf)
        A[m0:m1] = np.einsum("mtr,tr->m", np.abs(w), ah)
        m = np.arange(m0, m1)
        rot = np.exp(-2j * np.pi * (np.outer(m * D % M, k) % M) / M)            # exp(-j 2 pi k 500 m / 512)
        Y[:, m0:m1] = (np.fft.fft(v, axis=1) * rot).T
    if odd:
        m = np.arange(n_steps)
        Y *= np.exp(twist * 1j * np.pi * (HIST - D * (m % (4 * M))) / M)[None, :]    # exp(-j pi (7692 - 500 m) / 512)
    return Y, A


# error of the float32 bank (SPEC 3.5) against Y, in units of 2^-24 A.  Per component, an n-term fmaf chain is off by at most
# n u times the sum of the magnitudes of its terms; a complex value's two components together by sqrt 2 times that.
#   fold: 16-term chains over h x, I and Q separately                    16 sqrt 2
#   odd twist: one product + one fmaf per component, W rounded (u / 2)   2 sqrt 2 + 1
#   FFT: 9 radix-2 stages; each butterfly's t = b w (2 roundings per component, w rounded: 2 sqrt 2 + 1) and a +- t (1
#        rounding: sqrt 2) act on values whose magnitudes sum to at most sum |v_r| <= A; twiddles have unit modulus
#   prototype taps rounded to float32 (u / 2)                            1 / 2
C_BANK = 16 * math.sqrt(2) + (2 * math.sqrt(2) + 1) + 9 * (3 * math.sqrt(2) + 1) + 0.5

COUNTS_PER_RAD = 65536 / (2 * math.pi)


def _q16(a: np.ndarray) -> np.ndarray:
    """quadrants -> the SPEC's 16-bit phase, rint(16384 a) mod 2^16"""
    return np.rint(a * 16384.0).astype(np.int64) & 0xFFFF


def wrap16(d: np.ndarray) -> np.ndarray:
    return ((np.asarray(d, np.int64) + 32768) & 0xFFFF) - 32768


def phases_ref(Y: np.ndarray, odd: bool, m, *, deramp_first: bool = False, loose: bool = False) -> np.ndarray:
    """The SPEC's 16-bit phases q[k][m] = rint(16384 atan2q(Y)) mod 2^16, the odd bank's minus 32000 m (mod 2^16) after the
    rounding (trap: atan2q is not rotation-invariant; deramp_first = True is the mutation that evaluates it on the de-ramped
    value).  m: the step index of every sample (broadcast against Y).  loose: (2 / pi) arctan2 instead of atan2q.
    int64 in [0, 65536)."""
    m = np.asarray(m, np.int64)
    if odd and deramp_first:
        Y = Y * np.exp(-1j * np.pi * D * (m % (4 * M)) / M)
    f = (lambda z: np.arctan2(z.imag, z.real) * (2 / np.pi)) if loose else (lambda z: atan2q_ref(z.imag, z.real))
    q = _q16(f(Y))
    if odd and not deramp_first:
        q = (q - 32000 * (m % 256)) & 0xFFFF
    return q


def phase_errors(q_got: np.ndarray, Y: np.ndarray, A: np.ndarray, odd: bool, m_first: int = 0, *, loose: bool = False, **mut):
    """|q_got - reference| in counts over the bound, per sample ([512, n] floats; <= 1 passes).  q_got: the 16-bit phases
    (any integer type, or quadrants as floats); Y, A: bank() of the steps m_first ...
    Bound (counts) = 1 (rint) + the float32 evaluation of atan2q + KAPPA C_BANK 2^-24 A / |Y| radians (the bank's rounding
    turns the value by at most that angle), plus, loose, SPEC 3.1's approximation error.
    Trap: atan2q jumps by about 27 counts across each axis (one Newton step leaves r c < 1 there); where min(|Re Y|, |Im Y|) is
    within the bank's rounding of zero, the branch on the other side of the axis is accepted too."""
    q_got = np.asarray(q_got)
    if q_got.dtype.kind == "f":
        q_got = np.rint(q_got.astype(np.float64) * 16384.0).astype(np.int64)
    q_got = q_got.astype(np.int64)
    m = np.arange(m_first, m_first + Y.shape[1])[None, :]
    eb = C_BANK * U * A[None, :]
    mag = np.abs(Y)
    with np.errstate(divide="ignore", invalid="ignore"):
        ang = np.where(mag > eb, np.arcsin(np.minimum(eb / np.maximum(mag, 1e-300), 1.0)), np.pi)
    bound = 1.0 + 16384 * ATAN2Q_EVAL_ERR + KAPPA * ang * COUNTS_PER_RAD
    if loose:
        bound = bound + 16384 * ATAN2Q_MAX_ERR
    err = np.abs(wrap16(q_got - phases_ref(Y, odd, m, loose=loose, **mut))).astype(np.float64)
    mb = np.broadcast_to(m, Y.shape)
    ebb = np.broadcast_to(eb, Y.shape)
    for flip in (np.array(-1 + 1j), np.array(1 - 1j)):             # the other side of the imaginary / the real axis
        comp = Y.real if flip.real < 0 else Y.imag
        near = np.abs(comp) <= ebb
        if near.any():
            Yf = Y[near].real * flip.real + 1j * Y[near].imag * flip.imag
            ea = np.abs(wrap16(q_got[near] - phases_ref(Yf, odd, mb[near], loose=loose, **mut))).astype(np.float64)
            err[near] = np.minimum(err[near], ea)
    return err / bound


# ---------------------------------------------------------------- discriminators
def chan_disc(q: np.ndarray) -> np.ndarray:
    """SPEC 3.5: d[m] = (int16)(q[m] - q[m-1]) / 16384 quadrants, q[-1] = 0; q: [bins, n] 16-bit phases of a whole stream."""
    q = np.asarray(q, np.int64)
    prev = np.concatenate([np.zeros((q.shape[0], 1), np.int64), q[:, :-1]], axis=1)
    return wrap16(q - prev) / 16384.0


def vfo_disc(iq: np.ndarray):
    """SPEC 3.1 on one stream of float32 I/Q [n, 2] (x[-1] = 0).  cross = -I[n] Q[n-1] + Q[n] I[n-1] and
    dot = Q[n] Q[n-1] + I[n] I[n-1] from exact float64 products in the SPEC's operand order, rounded to float32 (IEEE
    signed zeros kept), then atan2q_ref.
    Returns (d, amb, loose_ok, d_loose): amb = how far the kernel's d may legitimately jump (cross or dot within the
    float32 rounding of zero: the other side of an axis -- or of +-pi, where +2 and -2 are both right -- is as correct;
    0 elsewhere); loose_ok = where (2 / pi) arctan2 is a fair reference (|z[n]| |z[n-1]| well above F, no such jump);
    d_loose = that arctan2."""
    iq = np.asarray(iq, np.float32)
    x1, y1 = iq[:, 0].astype(np.float64), iq[:, 1].astype(np.float64)
    x0, y0 = np.concatenate([[0.0], x1[:-1]]), np.concatenate([[0.0], y1[:-1]])
    cross64 = (-x1) * y0 + y1 * x0
    dot64 = y1 * y0 + x1 * x0
    cross, dot = cross64.astype(np.float32), dot64.astype(np.float32)
    d = atan2q_ref(cross, dot)
    # the kernel's fmaf(-I, Q', Q I') rounds Q I' and then the sum: it may miss the exact value by 2u (|I Q'| + |Q I'|)
    ec = 2 * U * (np.abs(x1 * y0) + np.abs(y1 * x0))
    ed = 2 * U * (np.abs(y1 * y0) + np.abs(x1 * x0))
    amb = np.zeros_like(d)
    for flip_c, flip_d, near in ((True, False, np.abs(cross64) < ec), (False, True, np.abs(dot64) < ed)):
        if near.any():
            c2 = np.where(near & flip_c, -cross, cross)
            d2 = np.where(near & flip_d, -dot, dot)
            amb = np.maximum(amb, np.where(near, np.abs(atan2q_ref(c2, d2) - d), 0.0))
    zz = np.hypot(x1, y1) * np.hypot(x0, y0)
    loose_ok = (zz > 1e-24) & (amb == 0.0) & ~(np.abs(cross64) < ec) & ~(np.abs(dot64) < ed)
    return d, amb, loose_ok, np.arctan2(cross64, dot64) * (2 / np.pi)


# ---------------------------------------------------------------- resamplers
def resample(d: np.ndarray, g: np.ndarray, up: int, down: int, *, i0_off: int = 0, p_off: int = 0, extra=None):
    """SPEC 3.5 / 3.7: o[j] = sum_{t<16} g[p][t] d[i0 - t], p = (j down) mod up, i0 = floor(j down / up), history zeros
    before the stream.  d: [..., n] float64 over the whole stream.  Returns (o, S1, S2, Sx) with S1 = sum_t |g_t|,
    S2 = sum_t |g_t| |d_t| and Sx = sum_t |g_t| extra_t (extra: a per-input-sample slack, e.g. vfo_disc's amb).
    Mutations: i0_off (i0 - 1), p_off (p +- 1, mod up)."""
    d = np.asarray(d, np.float64)
    n = d.shape[-1]
    n_out = n * up // down
    na = n_out // up                                   # n is a multiple of down: outputs j = up a + b, b < up
    pad = 17
    dp = np.concatenate([np.zeros(d.shape[:-1] + (pad,)), d], axis=-1)
    ep = None if extra is None else np.concatenate([np.zeros(d.shape[:-1] + (pad,)), np.asarray(extra, np.float64)], axis=-1)
    ad = np.abs(dp)
    os_, s1s, s2s, sxs = [], [], [], []
    for b in range(up):
        c = b * down // up + i0_off                    # i0 = down a + c
        p = (b * down % up + p_off) % up
        o = np.zeros(d.shape[:-1] + (na,))
        s2 = np.zeros_like(o)
        sx = None if ep is None else np.zeros_like(o)
        for t in range(16):
            sl = slice(pad + c - t, pad + c - t + down * (na - 1) + 1, down)     # d[i0 - t] for a = 0, 1, ...
            gt = g[p, t]
            o += gt * dp[..., sl]
            s2 += abs(gt) * ad[..., sl]
            if ep is not None:
                sx += abs(gt) * ep[..., sl]
        os_.append(o)
        s2s.append(s2)
        sxs.append(sx)
        s1s.append(np.full(na, np.abs(g[p]).sum()))
    flat = lambda v: np.stack(v, axis=-1).reshape(v[0].shape[:-1] + (n_out,))
    o, S1, S2 = flat(os_), flat(s1s), flat(s2s)
    Sx = None if ep is None else flat(sxs)
    return o, S1, S2, Sx


def row_bound(S1, S2, d_err: float = 0.0, Sx=None):
    """Tight bound of a float32 row against resample(): the 16-term fmaf chain (16 u sum |g d|) and the taps' float32
    rounding (u / 2 sum |g d|), plus d's own float32 error d_err through sum |g|, plus the slack Sx."""
    b = 16.5 * U * S2 + S1 * d_err
    return b + Sx if Sx is not None else b


def vfo_rows_ref(iq: np.ndarray, rate: int, *, loose: bool = False, g: np.ndarray | None = None, **mut):
    """The SPEC 3.7 chain on one stream: (rows, bound, valid).  tight: atan2q_ref discriminator, rows within row_bound of
    the float32 ones.  loose: arctan2 discriminator with SPEC 3.1's error through sum |g|; valid marks the rows whose 16
    inputs all have loose_ok."""
    up, down, _ = vfo_ratio(rate)
    g = resamp_taps(rate) if g is None else g
    d, amb, lok, dl = vfo_disc(iq)
    if loose:
        o, S1, S2, Sx = resample(dl, g, up, down, extra=(~lok).astype(np.float64), **mut)
        return o, row_bound(S1, S2, ATAN2Q_EVAL_ERR + ATAN2Q_MAX_ERR), Sx == 0.0
    o, S1, S2, Sx = resample(d, g, up, down, extra=amb, **mut)
    return o, row_bound(S1, S2, ATAN2Q_EVAL_ERR, Sx), np.ones(o.shape, bool)


# ---------------------------------------------------------------- SPEC 3.5b: the composite resampler + decimator
DEC_PER_BLOCK = STEPS * 12 // 5 // 4     # 1536 decimated samples (3 tiles of 512) per block of 2560 steps

# every mutation keyword of composite_rows and a value that is a bug (the tests assert that each is rejected)
COMPOSITE_MUTATIONS = {
    "b_plus_1": dict(b_off=1),
    "b_minus_1": dict(b_off=-1),
    "row_rotated": dict(row_rot=1),
    "difference_in_32_bits": dict(wrap=False),
    "carried_phases_zero": dict(carry_zero=True),
    "quarter_missing": dict(quarter=False),
    "group_one_late": dict(group_off=1),
}


def _newest_input(n):
    """b(n) = floor(5 (4 n + 3) / 12): the newest discriminator sample decimated sample n reads (used to place the mutations only)"""
    return (5 * (4 * np.asarray(n, np.int64) + 3)) // 12


def _resample_then_average(d: np.ndarray, g: np.ndarray, group_off: int = 0):
    """z[n] = 1/4 sum_{i<4} o[4n + i + group_off] and A[n] = 1/4 sum_i sum_t |g_t| |d_t| of the same outputs; d: [n] with n % 5 == 0"""
    n = d.shape[-1]
    dd = np.concatenate([d, np.zeros(5)])                         # room for one more output group
    o, _, S2, _ = resample(dd, g, 12, 5)
    nz = n * 12 // 5 // 4
    o, S2 = o[group_off:group_off + 4 * nz], S2[group_off:group_off + 4 * nz]
    return o.reshape(nz, 4).sum(1) * 0.25, S2.reshape(nz, 4).sum(1) * 0.25


def composite_rows(q: np.ndarray, *, loose: bool = False, b_off: int = 0, row_rot: int = 0, wrap: bool = True, carry_zero: bool = False,
                   quarter: bool = True, group_off: int = 0):
    """SPEC 3.5b in float64 as "resample, then average": q: the 16-bit phases of ONE bin's whole stream (int64, q[-1] = 0 before
    the stream, a multiple of 5 steps).  d[m] = wrap16(q[m] - q[m-1]) / 16384 (exact: chan_disc), the 12/5 resampler
    o[j] = sum_{t<16} g*[5j mod 12][t] d[floor(5j / 12) - t] with the closed-form double taps g* = resamp_taps(20000), and
    z[n] = 1/4 sum_{i<4} o[4n + i].  Neither b(n) nor the rows G of DESIGN.md's formula are used: if that formula or its
    implementation is wrong, the two differ.  Returns (z, bound), 12 decimated samples per 20 steps.

    Bound of the float32 row z32[n] = sum_{k<17} fmaf(G[n mod 3][k], d[b(n) - k], acc) against z[n].  In exact arithmetic
    z[n] = sum_k G*_k d[b(n) - k] with G*_k = 1/4 sum_i g*_i (the taps of the four outputs that meet input b(n) - k).
      d is exact (a multiple of 2^-14 in [-2, 2)).
      The taps: the product uses G = fl32(1/4 sum_i fl32(g*_i)), summed in double: |fl32(g*_i) - g*_i| <= u |g*_i|, the final
      rounding u |G*| (1 + u), so per term |G_k - G*_k| <= u |G*_k| + 1/4 sum_i u |g*_i| <= 2 u a_k, a_k = 1/4 sum_i |g*_i|.
      The 17-term fmaf chain: at most 17 u sum_k |G_k d_k| <= 17 u (1 + 2 u) sum_k a_k |d_k|.
    With A[n] = sum_k a_k |d_k| = 1/4 sum_{i<4} sum_t |g*[p_i][t]| |d[i0_i - t]| (resample()'s S2 averaged over the group):
      bound[n] = 19 u (1 + 2^-20) A[n]           (2 u A for the taps, 17 u (1 + 2 u) A for the chain, second order terms rounded up)
    -- a formula of the inputs alone.  loose = True has nothing to add (there is no approximant in this stage); it is accepted so that
    the callers can pass their layer through.
    Mutations: b_off (b(n) +- 1: every read one sample later / earlier), row_rot (row (n + 1) mod 3 at b(n)), wrap = False (the
    difference taken in 32 bits), carry_zero (the 16 carried phases at the head of every block of 2560 steps replaced by zeros),
    quarter = False (the 1/4 missing), group_off = 1 (the averaging group starts one resampler output late)."""
    q = np.asarray(q, np.int64)
    assert q.ndim == 1 and q.shape[0] % 5 == 0
    g = resamp_taps(20000)
    prev = np.concatenate([[0], q[:-1]])
    d = (wrap16(q - prev) if wrap else (q - prev)) / 16384.0
    if b_off > 0:
        d = np.concatenate([d[b_off:], np.zeros(b_off)])
    elif b_off < 0:
        d = np.concatenate([np.zeros(-b_off), d[:b_off]])
    z, A = _resample_then_average(d, g, group_off=group_off)
    n = np.arange(z.shape[0])
    if row_rot:
        # row (n + 1) mod 3 applied at b(n): sample n + 1 of the stream delayed by b(n + 1) - b(n) (1 or 2) steps
        delta = _newest_input(n + 1) - _newest_input(n)
        z0, A0 = z, A
        z, A = z0.copy(), A0.copy()
        for dl in (1, 2):
            zs, As = _resample_then_average(np.concatenate([np.zeros(dl), d, np.zeros(5 - dl)]), g)
            sel = delta == dl
            z[sel], A[sel] = zs[n[sel] + 1], As[n[sel] + 1]
    if carry_zero:
        # what a block sees of the stream before it is zeros: its first difference is q[first] - 0, the 16 before it vanish
        edge = np.arange(STEPS, q.shape[0], STEPS)
        dz = d.copy()
        for e in edge:
            dz[e - 16:e] = 0.0
            dz[e] = (wrap16(q[e]) if wrap else q[e]) / 16384.0
        zz, Az = _resample_then_average(dz, g)
        head = (_newest_input(n % DEC_PER_BLOCK) <= 16) & (n >= DEC_PER_BLOCK)
        z, A = np.where(head, zz, z), np.where(head, Az, A)
    if not quarter:
        z, A = 4.0 * z, 4.0 * A
    return z, 19.0 * U * (1.0 + 2.0 ** -20) * A


# ---------------------------------------------------------------- test signals (complex128 streams at 10 MS/s)
def tones(n: int, spec, seed: int = 0) -> np.ndarray:
    """sum of exp(j (2 pi f n / FS + phi)) a over spec = [(bin, offset_hz, amplitude), ...], random phases"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n, np.complex128)
    for k, df, a in spec:
        f = (k * BIN_HZ + df) / FS
        th = (2 * np.pi * ((f * t) % 1.0) + rng.uniform(0, 2 * np.pi)).astype(np.float32)
        x.real += a * np.cos(th)
        x.imag += a * np.sin(th)
    return x


def chirp(n: int, bin0: float, bin1: float, a: float = 1.0) -> np.ndarray:
    """a linear sweep from bin0 to bin1 (in bins) over the n samples"""
    t = np.arange(n, dtype=np.float64)
    f0, f1 = bin0 / M, bin1 / M
    ph = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / n * t * t)
    return a * np.exp(1j * ph)


def noise(n: int, sigma: float = 1.0, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)


def as_iq32(x: np.ndarray) -> np.ndarray:
    """complex stream -> float32 [n, 2] (what the bank reads; the reference then uses exactly these values)"""
    return np.stack([x.real, x.imag], axis=1).astype(np.float32)


def as_int_iq(x: np.ndarray, bits: int) -> np.ndarray:
    """complex stream scaled so that 1.0 is full scale, rounded and clipped to the integer range of bits (int16: -32767 ..
    32767 as a receiver's AGC clips; int8: -128 .. 127, the offset-binary corner included): integer-valued [n, 2] array"""
    top = (1 << (bits - 1)) - 1
    lo = -top if bits == 16 else -top - 1
    v = np.rint(np.stack([x.real, x.imag], axis=1) * top)
    return np.clip(v, lo, top).astype(np.int16 if bits == 16 else np.int8)
