"""Float64 / integer reference of the sonde type detector, written from DESIGN.md section 3.8 alone: it imports neither the product
nor oracle/.  The SPEC's atan2q model and the discriminator operand order come from tests/fe_reference.py (a test helper); every
detector constant is written out here.

Layers:
  front-end  -- float64 model of the two branches (GFSK 24 kS/s, AFSK 6 kS/s) and the quantiser; `atan="exact"` uses
                (2/pi) arctan2, `atan="spec"` the SPEC's atan2q evaluated in float64;
  scores     -- integer Pearson correlation of each template with every complete window, one IEEE double division per lag:
                bit-for-bit what the kernel must report on the same quantised streams;
  decision   -- thresholds and the argmax of best / theta.

Mutation keywords (`chip_off`, `ceil_mode`, `short`, `ed_no_s1`, `phase_reset`) exist so that the tests can show that the
checks reject the mistakes they exist for."""
from __future__ import annotations

import math

import numpy as np

from fe_reference import ATAN2Q_MAX_ERR, U, atan2q_ref

RS41, DFM09, IMS100, M10, IMET4, C50, MRZN1 = range(7)
NTYPES = 7
FS = 48000
QSTEP = 4096            # quantiser: 2^-12 quadrant per count
QCLAMP = 4.0
GFSK_TYPES = (RS41, DFM09, IMS100, M10, MRZN1)     # 24 kS/s branch, stream D
LMAX24, LMAX6 = 320, 60                           # longest template per branch (the history a submit carries)

# SPEC 3.6: mixer tables (cycles per table period at 48 kS/s) and boxcar lengths in 8-sample blocks
AF_IMET = (17, 480, 5)       # 1700 Hz
AF_C50 = (19, 240, 2)        # 3800 Hz


def _bits_msb(v: int, n: int):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def _manchester(bits):
    out = []
    for b in bits:
        out += [b, 1 - b]          # 1 -> 10, 0 -> 01
    return out


def _biphase_s(bits):
    """first chip +1 (level 1); a transition at every bit boundary, a second one mid-bit for a 0"""
    out, lvl = [], 0
    for i, b in enumerate(bits):
        lvl = 1 if i == 0 else 1 - lvl
        out.append(lvl)
        if not b:
            lvl = 1 - lvl
        out.append(lvl)
    return out


def sync_chips(t: int):
    """on-air sync of type t as chips 0/1, in air order"""
    if t == RS41:
        return [(byte >> k) & 1 for byte in (0x10, 0xB6, 0xCA, 0x11, 0x22, 0x96, 0x12, 0xF8) for k in range(8)]
    if t == DFM09:
        return _manchester(_bits_msb(0x45CF, 16))
    if t == M10:
        return [int(c) for c in "10011001100110010100110010011001"]
    if t == IMS100:
        return _biphase_s(_bits_msb(0x049DCE, 24))
    if t == MRZN1:
        return _manchester(sum((_bits_msb(b, 8) for b in (0xAA, 0xBF, 0x35)), []))
    if t == IMET4:
        return [int(c) for c in "101000000010"]
    if t == C50:
        return [int(c) for c in "1" + "0" + "00000000" + "1" + "0" + "11111111" + "1"]
    raise ValueError(t)


# chip rate and stream rate of each type's template
BAUD = {RS41: 4800, DFM09: 5000, IMS100: 4800, M10: 9600, IMET4: 1200, C50: 2400, MRZN1: 4800}
RATE = {t: (6000 if t in (IMET4, C50) else 24000) for t in range(NTYPES)}
DEC = {t: FS // RATE[t] for t in range(NTYPES)}         # input samples per stream sample: 2 or 8
# +1: chip 1 scores positive when upright.  GFSK: a 1 is the upper frequency.  AFSK: iMet's mark (1200 Hz) lies below the
# 1700 Hz mixer, so a 1 reads negative; SRS-C50's mark (4700 Hz) lies above the 3800 Hz mixer, so a 1 reads positive.
SIGN = {RS41: 1, DFM09: 1, IMS100: 1, M10: 1, MRZN1: 1, IMET4: -1, C50: 1}


def template(t: int, *, chip_off: int = 0, ceil_mode: str = "ceil"):
    """s[n] = c[floor(n baud / fs')], n < L = ceil(Nchips fs' / baud), c = +-1 (SIGN applied).  Mutations: chip_off shifts the
    chips by one (a template off by one chip); ceil_mode = "floor" renders L and the chip boundaries with floor instead."""
    c = np.array(sync_chips(t), np.int64) * 2 - 1
    if chip_off:
        c = np.roll(c, chip_off)
    c = c * SIGN[t]
    fs, baud, nc = RATE[t], BAUD[t], len(c)
    if ceil_mode == "ceil":
        L = -(-nc * fs // baud)
        n = np.arange(L)
        return c[n * baud // fs]
    L = nc * fs // baud
    b = [j * fs // baud for j in range(nc + 1)]
    s = np.zeros(L, np.int64)
    for j in range(nc):
        s[b[j]:b[j + 1]] = c[j]
    return s


# ---------------------------------------------------------------- front-ends
def _atan(cross, dot, atan):
    if atan == "exact":
        return np.arctan2(cross, dot) * (2.0 / math.pi)
    return atan2q_ref(cross, dot)


def disc(z: np.ndarray, zprev0: complex = 0.0, atan: str = "exact"):
    """SPEC 3.1 on a complex stream: arg(z[m] conj(z[m-1])) in quadrants, z[-1] = zprev0"""
    zp = np.concatenate([[zprev0], z[:-1]])
    p = z * np.conj(zp)
    return _atan(p.imag, p.real, atan)


def quantise(v: np.ndarray) -> np.ndarray:
    """Qz(v) = rint(clamp(v, -4, 4) 4096)"""
    return np.rint(np.clip(v, -QCLAMP, QCLAMP) * QSTEP).astype(np.int64)


def as_complex(x: np.ndarray) -> np.ndarray:
    """[n, 2] rows of any input kind (float32, int16, int8) -> complex128, exactly"""
    x = np.asarray(x)
    return x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)


def mixer(cycles: int, per: int) -> np.ndarray:
    """SPEC 3.6's table W[k] = (cos, -sin)(2 pi cycles k / per), stored as float32"""
    a = 2.0 * math.pi * cycles * np.arange(per) / per
    return (np.cos(a).astype(np.float32).astype(np.float64) + 1j * np.sin(-a).astype(np.float32).astype(np.float64))


def front_end(rows, real: bool, *, atan: str = "exact", submits=None, phase_reset: bool = False):
    """The whole stream of one channel since create / reset -> (d2, q_imet, q_c50) in quadrants (float64, unquantised) and, for
    the error bounds, per-sample input noise |dz| of the AFSK boxcar outputs (see afsk_bound).
    rows: [n] float (real) or [n, 2] (IQ kinds).  submits: the submit lengths (only used by the phase_reset mutation)."""
    if real:
        d48 = np.asarray(rows, np.float64)
        d2 = d48[0::2] + d48[1::2]
    else:
        x = as_complex(rows)
        d2 = disc(x[0::2] + x[1::2], atan=atan)
        d48 = disc(x, atan=atan)
    n = len(d48)
    idx = np.arange(n)
    if phase_reset:                                    # mutation: the mixer phase restarts at every submit
        idx = np.concatenate([np.arange(k) for k in submits])
    out = []
    for cyc, per, nw in (AF_IMET, AF_C50):
        W = mixer(cyc, per)
        b = (d48 * W[idx % per]).reshape(-1, 8).sum(axis=1)
        bp = np.concatenate([np.zeros(nw, complex), b])
        z = sum(bp[nw - k: nw - k + len(b)] for k in range(nw))
        out.append(disc(z, atan=atan))
    return d2, out[0], out[1]


def quantised_streams(rows, real: bool, **kw):
    d2, qi, qc = front_end(rows, real, **kw)
    return quantise(d2), quantise(qi), quantise(qc)


# ---------------------------------------------------------------- error bounds of the product's front-end
E_ATAN = ATAN2Q_MAX_ERR + 16 * U         # SPEC atan2q error (quadrants) + float32 evaluation of atan2q and of cross / dot


def wrap_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a - b in quantiser counts, modulo the 4-quadrant turn (+2 and -2 quadrants are the same angle)"""
    d = np.asarray(a, np.int64) - np.asarray(b, np.float64)
    return d - 4 * QSTEP * np.round(d / (4 * QSTEP))


def gfsk_bound() -> float:
    """|D - 4096 d2_ref| (counts) on IQ input whose boxcar sums are exact: atan2q's SPEC error + half a quantiser step"""
    return QSTEP * E_ATAN + 0.5


def afsk_bound(rows, real: bool):
    """Per-sample bound (counts) of |A - 4096 q_ref| for both tone sets, and where it is meaningful.  The mixer's input d
    is exact for real rows and within E_ATAN per sample for IQ rows; a boxcar output z built from 8 nw such samples moves by at
    most dz = nw 8 e_in + 24 U sum |d| (float32 products and sums of the mixer and the boxcar), which turns the arctangent by
    asin(dz / |z|); q is the angle between two such z.  Samples with dz >= |z| / 2 carry no bound (flagged False)."""
    if real:
        d48 = np.asarray(rows, np.float64)
        e_in = 0.0
    else:
        d48 = disc(as_complex(rows))
        e_in = E_ATAN
    res = []
    for cyc, per, nw in (AF_IMET, AF_C50):
        W = mixer(cyc, per)
        n = len(d48)
        b = (d48 * W[np.arange(n) % per]).reshape(-1, 8).sum(axis=1)
        a = np.abs(d48).reshape(-1, 8).sum(axis=1)
        bp, ap = np.concatenate([np.zeros(nw, complex), b]), np.concatenate([np.zeros(nw), a])
        z = sum(bp[nw - k: nw - k + len(b)] for k in range(nw))
        az = sum(ap[nw - k: nw - k + len(b)] for k in range(nw))
        dz = nw * 8 * e_in + 24 * U * az
        mz = np.abs(z)
        ratio = dz / np.maximum(mz, 1e-300)
        rp = np.concatenate([[0.0], ratio[:-1]])
        ok = (ratio < 0.5) & (rp < 0.5)
        ok[0] = False
        ang = (np.arcsin(np.minimum(ratio, 1.0)) + np.arcsin(np.minimum(rp, 1.0))) * (2.0 / math.pi)
        res.append((QSTEP * (E_ATAN + ang) + 0.5, ok))
    return res


# ---------------------------------------------------------------- scores
def scores(Dstream: np.ndarray, s: np.ndarray, *, short: bool = False, ed_no_s1: bool = False):
    """r[t] for every complete window of the integer stream (t = 0 .. len - L): the SPEC's exact integers, then
    r = double(N) / sqrt(double(Et) * double(Ed)), 0 where Ed == 0.  Mutations: `short` sums one sample less than L,
    `ed_no_s1` leaves S1^2 out of Ed."""
    D = np.asarray(Dstream, np.int64)
    L = len(s)
    Lw = L - 1 if short else L
    nt = len(D) - L + 1
    if nt <= 0:
        return np.zeros(0)
    P = np.concatenate([[0], np.cumsum(D)])
    P2 = np.concatenate([[0], np.cumsum(D * D)])
    t = np.arange(nt)
    S1 = P[t + Lw] - P[t]
    S2 = P2[t + Lw] - P2[t]
    # SD = sum_j c_j (P[t + b_(j+1)] - P[t + b_j]) over the constant runs of s
    SD = np.zeros(nt, np.int64)
    edges = np.flatnonzero(np.diff(s)) + 1
    starts = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [Lw]])
    for a, e in zip(starts, ends):
        if a < Lw:
            SD += s[a] * (P[t + min(e, Lw)] - P[t + a])
    T1 = int(s[:Lw].sum())
    N = Lw * SD - T1 * S1
    Et = Lw * Lw - T1 * T1
    Ed = Lw * S2 - (0 if ed_no_s1 else S1 * S1)
    den = np.sqrt(float(Et) * Ed.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(Ed == 0, 0.0, N.astype(np.float64) / np.where(Ed == 0, 1.0, den))
    return r


def best_of(r: np.ndarray):
    """(best |r|, sign < 0, t): max |r|, earliest t on ties; (0, False, 0) with no window"""
    if len(r) == 0:
        return 0.0, False, 0
    a = np.abs(r)
    t = int(np.argmax(a))
    if a[t] == 0.0:
        return 0.0, False, 0
    return float(a[t]), bool(r[t] < 0), t


def detect_streams(D, Ai, Ac, *, types=range(NTYPES), tmpl=None, **mut):
    """best [7], inverted [7] (bool), pos [7] (input samples) from the whole quantised streams of one channel"""
    best = np.zeros(NTYPES)
    inv = np.zeros(NTYPES, bool)
    pos = np.zeros(NTYPES, np.uint64)
    for k in types:
        st = D if k in GFSK_TYPES else (Ai if k == IMET4 else Ac)
        s = template(k) if tmpl is None else tmpl[k]
        b, neg, t = best_of(scores(st, s, **mut))
        best[k], inv[k], pos[k] = b, (neg and k != IMS100), DEC[k] * t
    return best, inv, pos


# ---------------------------------------------------------------- decision
# theta_k: 1.1 x the largest best_k seen on AWGN and on 30 dB signals of the other six types (threshold table);
# float32 values, used as doubles
THETA = np.array([0.52, 0.79, 0.85, 0.82, 0.83, 0.91, 0.86], np.float32)


def decide(best, mask: int = 0x7F, theta=None) -> int:
    th = (THETA if theta is None else np.asarray(theta, np.float32)).astype(np.float64)
    kbest, vbest = -1, 0.0
    for k in range(NTYPES):
        if not (mask >> k) & 1 or best[k] < th[k]:
            continue
        v = best[k] / th[k]
        if v > vbest:
            kbest, vbest = k, v
    return kbest


def detect_rows(rows, real: bool, mask: int = 0x7F, **kw):
    """front-end (exact arctangent) + scores + decision on one channel's whole stream"""
    D, Ai, Ac = quantised_streams(rows, real, **kw)
    best, inv, pos = detect_streams(D, Ai, Ac)
    return decide(best, mask), best, inv, pos
