"""Float64 reference of the demodulator core, written from DESIGN.md section 3 (SPEC 3.0-3.0e, 3.2, 3.2b, 3.6, 3.6b) and nothing
else: it imports neither the oracle nor the product and loads no table from either.  The modem constants are written below, the tap
rows are computed in closed form, and every discrete rule of the SPEC is taken literally.

The timing loop is not run closed here.  rint ties and decisions at the threshold would make two closed runs drift apart, so the
reference checks ONE step of the recurrence at a time, from the product's own observable state after every tile (t_next, period,
bias, amp, the newest AFC state u, the bits): replay() predicts what the next tile must do and bounds every prediction by a
formula (float32 rounding of the chains the SPEC prescribes, the SPEC's approximation errors, +-1 of each rint that can tie).

Two layers, as in fe_reference.py:
  tight -- the SPEC's atan2q evaluated in float64: what remains is float32 rounding;
  loose -- np.arctan2 plus SPEC 3.1's documented approximation error.

Every function takes mutation keywords (see MUTATIONS) so that the tests can show that the bounds reject the bugs they exist for."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from fe_reference import ATAN2Q_EVAL_ERR, ATAN2Q_MAX_ERR, KAPPA, U, atan2q_ref

FS = 48000                       # decoder input rate
TILE = 2048                      # input samples per tile (behind the tone front-end for the AFSK streams)
NPHASE = 32                      # polyphase branches
ROUND = 256                      # symbols per round; the Gardner detector and m_k only for k < 256
SLACK = 4                        # samples of look-ahead slack in `limit`
AFC_GAIN = math.pi / 16          # SPEC 3.0b: 0.19634954 = a quarter of pi / 4
AFC_LEAK = 1.0 / 128
AFC_MAX = 0.8
CUTOFF = float(np.float32(0.65))  # SPEC 3.2: the low-pass cutoff in baud, the float32 0.65 (0.64999998) as the host's double formula reads it
ROT_FIT_ERR = 2.3e-5             # SPEC 3.0e: max error of the odd polynomial rot(u) against (4 / pi) atan u, quadrants
# SPEC 3.2 recip(x): integer-subtract seed (relative error < 5.1 %) and three Newton steps, each in fmaf: 0.051^2 -> 2.6e-3 -> 6.8e-6
# (+ 2u of rounding) -> (6.9e-6)^2 + u (1 + 6.9e-6): the last step's own rounding dominates
RECIP_ERR = U * (1.0 + 7e-6) + 4.8e-11


@dataclass(frozen=True)
class Modem:
    name: str
    baud: float
    decim: int          # input samples per internal sample in front of the discriminator (1 behind the tone front-end)
    pre: int            # 8: the AFSK tone front-end of SPEC 3.6 in front (48 kS/s -> 6 kS/s)
    itile: int          # internal samples per tile
    period0: int        # Q16 samples per symbol
    T: int              # taps in use per row
    rmax: int           # symbols per round at most
    rounds: int         # rounds per tile


# SPEC 3.0 / 3.2 / 3.6: written out, not derived from the library.  period0 = rint(65536 fs_int / baud); T = 8 below 3.5 samples per
# symbol (16 for the AFSK streams); rmax = 512 where a tile holds more than 256 symbols (M10 at either rate, the 6 kS/s streams);
# rounds = ceil((itile 65536 / pmin + 2) / rmax).
MODEMS = {
    # type: (default, SONDE_FLAG_WIDE)
    0: (Modem("RS41", 4800.0, 4, 1, 512, 163840, 8, 256, 1), Modem("RS41", 4800.0, 2, 1, 1024, 327680, 16, 256, 1)),
    1: (Modem("DFM", 5000.0, 4, 1, 512, 157286, 8, 256, 1), Modem("DFM", 5000.0, 2, 1, 1024, 314573, 16, 256, 1)),
    2: (Modem("iMS-100", 4800.0, 4, 1, 512, 163840, 8, 256, 1), Modem("iMS-100", 4800.0, 2, 1, 1024, 327680, 16, 256, 1)),
    3: (Modem("M10", 9600.0, 2, 1, 1024, 163840, 8, 512, 1), Modem("M10", 9600.0, 1, 1, 2048, 327680, 16, 512, 1)),
    4: (Modem("iMet-4", 1200.0, 1, 8, 2048, 327680, 16, 512, 1),) * 2,
    5: (Modem("C50", 2400.0, 1, 8, 2048, 163840, 16, 512, 2),) * 2,
    6: (Modem("MRZ-N1", 4800.0, 4, 1, 512, 163840, 8, 256, 1), Modem("MRZ-N1", 4800.0, 2, 1, 1024, 327680, 16, 256, 1)),
}
WIDE_AUTO_TYPES = (2, 3, 6)      # SPEC 3.0: SONDE_FLAG_WIDE_AUTO widens iMS-100, MRZ-N1 and M10 only

# SPEC 3.6: the tone front-end of the AFSK streams: (mixer cycles, table period, boxcar blocks)
AFSK = {4: (17, 480, 5), 5: (19, 240, 2)}
AF_DEC = 8

# every mutation keyword and a value that is a bug (the tests assert that each is rejected)
MUTATIONS = {
    "cutoff_060": dict(cutoff=0.60),
    "rows_not_normalised": dict(normalise=False),
    "phase_plus_1": dict(p_off=1),
    "phase_minus_1": dict(p_off=-1),
    "fir_history_short": dict(n_off=-1),
    "mid_after": dict(mid_sign=+1),
    "gardner_k0": dict(gardner_k0=True),
    "gardner_k256": dict(gardner_k256=True),
    "e_over_k": dict(e_over_k=True),
    "slack_3": dict(slack=3),
    "pclamp_128": dict(pclamp=7),
    "no_acquisition": dict(acq_tiles=0),
    "acquisition_2": dict(acq_tiles=2),
    "afc_lag_2": dict(afc_lag=2),
    "afc_gain_quarter": dict(afc_gain=0.25),
    "afc_leak_64": dict(afc_leak=1.0 / 64),
    "box_plus_u": dict(r_sign=+1),
    "box_front_current_u": dict(front_cur=True),
    "shift_30e_flipped": dict(shift_sign=+1),
    "shift_30e_missing": dict(shift_sign=0),
    "group_shifted": dict(group_off=1),
    "imet_mixer_1800": dict(mix_hz=1800.0),
    "boxcar_4_blocks": dict(box_blocks=4),
    "jump_16_16": dict(jump_ratio=16),
}


def modem(stype: int, wide: bool = False) -> Modem:
    return MODEMS[stype][1 if wide else 0]


# ---------------------------------------------------------------- SPEC 3.2: the tap rows in closed form
def taps(m: Modem, *, cutoff: float = CUTOFF, normalise: bool = True, **_) -> np.ndarray:
    """[32, T] float64: Blackman-windowed sinc, cutoff `cutoff` baud, H[p][j] = f(j - T/2 + p/32), f(t) = 2 fc sinc(2 fc t) times the
    Blackman window over t in [-T/2, T/2]; each row normalised to unit DC gain."""
    fc = cutoff * m.baud / (FS / (m.decim * m.pre))
    t = np.arange(m.T)[None, :] - m.T // 2 + np.arange(NPHASE)[:, None] / NPHASE
    w = 0.42 + 0.5 * np.cos(2 * np.pi * t / m.T) + 0.08 * np.cos(4 * np.pi * t / m.T)
    h = 2 * fc * np.sinc(2 * fc * t) * w
    return h / h.sum(axis=1, keepdims=True) if normalise else h


# ---------------------------------------------------------------- SPEC 3.1 on a float64 phasor, with its error bound
def _disc(W: np.ndarray, eW: np.ndarray, loose: bool):
    """d = atan2q(W) quadrants and its bound, W the (complex128) value the float32 chain approximates within eW (|.|_1).
    Bound: the angle eW / |W| can turn W by (times KAPPA), the float32 evaluation of atan2q, and the other branch where a
    component of W lies within eW of zero (atan2q jumps across the axes; at +-2 both signs are right)."""
    mag = np.abs(W)
    with np.errstate(divide="ignore", invalid="ignore"):
        ang = np.where(eW == 0.0, 0.0, np.where(mag > eW, np.arcsin(np.minimum(eW / np.maximum(mag, 1e-300), 1.0)), np.pi))
    if loose:
        d = np.arctan2(W.imag, W.real) * (2 / np.pi)
        b = ATAN2Q_MAX_ERR + ATAN2Q_EVAL_ERR + KAPPA * ang * (2 / np.pi)
    else:
        d = atan2q_ref(W.imag, W.real)
        b = ATAN2Q_EVAL_ERR + KAPPA * ang * (2 / np.pi)
    amb = np.zeros_like(d)
    for near, flip in (((np.abs(W.imag) <= eW) & (eW > 0), np.conj), ((np.abs(W.real) <= eW) & (eW > 0), lambda z: -np.conj(z))):
        if near.any():
            Wf = flip(W[near])
            df = np.arctan2(Wf.imag, Wf.real) * (2 / np.pi) if loose else atan2q_ref(Wf.imag, Wf.real)
            amb[near] = np.maximum(amb[near], np.abs(df - d[near]))
    return d, np.minimum(b + amb, 4.0)


def rot(u):
    """SPEC 3.0e in float64: (4 / pi) atan u"""
    return (4 / np.pi) * np.arctan(u)


def _afc_fifo(u_after: np.ndarray, ntiles: int, lag: int) -> np.ndarray:
    """the AFC state each tile's discriminator uses: u after tile j - lag (0 before the stream)"""
    u = np.zeros(ntiles)
    if ntiles > lag:
        u[lag:] = u_after[:ntiles - lag]
    return u


# ---------------------------------------------------------------- SPEC 3.0, 3.0b, 3.0d: the discriminator stream of the GFSK classes
def disc_iq(x: np.ndarray, m: Modem, u_after: np.ndarray, *, loose: bool = False, afc_lag: int = 3, r_sign: int = -1,
            front_cur: bool = False, group_off: int = 0, **_):
    """x: [n, 2] input values (float32 IQ, or the integers of the 16- / 8-bit rows), n a multiple of 2048; u_after[j]: the AFC state
    u the product reported after tile j.  Returns (d, bound) per internal sample.
    Mutations: afc_lag (another FIFO depth), r_sign = +1 (R = (1 - u^2/2, +u)), front_cur (the sample in front of a tile turned with
    the current tile's u), group_off (the decimation groups shifted by that many samples)."""
    x = np.asarray(x, np.float64)
    if group_off:
        x = np.concatenate([np.zeros((group_off, 2)), x[:-group_off]])
    n = x.shape[0]
    ntiles = n // TILE
    D = m.decim
    ns = n // D
    ut = _afc_fifo(np.asarray(u_after, np.float64), ntiles, afc_lag)
    u = np.repeat(ut, m.itile)                                    # u of every internal sample's tile
    xc = (x[:, 0] + 1j * x[:, 1]).reshape(ns, D)
    xa = (np.abs(x[:, 0]) + np.abs(x[:, 1])).reshape(ns, D)
    h = D // 2
    if D == 1:
        P0, P1 = xc[:, 0], np.zeros(ns, complex)
        A0, A1 = xa[:, 0], np.zeros(ns)
    else:
        P0, P1 = xc[:, :h].sum(1), xc[:, h:].sum(1)
        A0, A1 = xa[:, :h].sum(1), xa[:, h:].sum(1)

    def z_of(uu):
        R = (1.0 - 0.5 * uu * uu) + 1j * r_sign * uu
        return P0 + R * P1

    z = z_of(u)
    # float32: the half-sums (one add per component), rr = fmaf(-u/2, u, 1), R P1 (product + fmaf), the final add: at most 8 u of the
    # magnitudes involved (|R|_1 <= 1 + |u| <= 2)
    ez = 8.0 * U * (A0 + 2.0 * A1) if D > 1 else np.zeros(ns)
    zprev = np.concatenate([[0.0], z[:-1]])
    ezprev = np.concatenate([[0.0], ez[:-1]])
    if front_cur and D > 1:
        first = np.arange(m.itile, ns, m.itile)
        zprev[first] = P0[first - 1] + ((1.0 - 0.5 * u[first] ** 2) + 1j * r_sign * u[first]) * P1[first - 1]
    P = z * np.conj(zprev)
    Zn = np.abs(z.real) + np.abs(z.imag)
    Zp = np.abs(zprev.real) + np.abs(zprev.imag)
    eP = 4.0 * U * Zn * Zp + 2.0 * (ez * Zp + Zn * ezprev + ez * ezprev)
    W = P * ((1.0 - u * u) - 2j * u)
    eW = (1.0 + np.abs(u)) ** 2 * (eP + 3.0 * U * Zn * Zp)
    return _disc(W, eW, loose)


def disc_real(x: np.ndarray, m: Modem, *, decimated: bool = False, group_off: int = 0, **_):
    """Real discriminator input (SPEC 3.0: averaged like IQ, ((x0 + x1) + (x2 + x3)) 0.25 / (x0 + x1) 0.5), or already decimated
    (the channelizer's 3.5b rows: the ring takes them as they are).  Returns (d, bound)."""
    x = np.asarray(x, np.float64)
    if decimated or m.decim == 1:
        return x.copy(), np.zeros(x.shape[0])
    if group_off:
        x = np.concatenate([np.zeros(group_off), x[:-group_off]])
    g = x.reshape(-1, m.decim)
    return g.mean(1), 2.0 * U * np.abs(g).sum(1) / m.decim


# ---------------------------------------------------------------- SPEC 3.6: the tone front-end of the AFSK streams
def disc_afsk(x: np.ndarray, stype: int, *, is_iq: bool = True, loose: bool = False, mix_hz: float | None = None,
              box_blocks: int | None = None, **_):
    """x: [n, 2] IQ (or [n] audio) at 48 kS/s from the stream's first sample.  Mixer (cos, -sin)(2 pi cyc k / per), block sums of 8,
    boxcar over the newest `win` block sums, the discriminator of 3.1 on z.  Returns (q, bound) at 6 kS/s.
    Mutations: mix_hz (another mixer frequency), box_blocks (another boxcar length)."""
    cyc, per, win = AFSK[stype]
    if box_blocks is not None:
        win = box_blocks
    if is_iq:
        x = np.asarray(x, np.float64)
        z1 = x[:, 0] + 1j * x[:, 1]
        zp = np.concatenate([[0.0], z1[:-1]])
        Za = (np.abs(z1.real) + np.abs(z1.imag)) * (np.abs(zp.real) + np.abs(zp.imag))
        d1, b1 = _disc(z1 * np.conj(zp), 4.0 * U * Za, loose)
    else:
        d1 = np.asarray(x, np.float64)
        b1 = np.zeros_like(d1)
    n = d1.shape[0]
    k = np.arange(n)
    f = (mix_hz / FS) if mix_hz is not None else cyc / per
    Wm = np.exp(-2j * np.pi * ((f * k) % 1.0 if mix_hz is not None else (cyc * (k % per) % per) / per))
    b = (d1 * Wm).reshape(-1, AF_DEC).sum(1)
    # per component: the 8-term fmaf chain (8 u sum |d W|), the table's float32 rounding (u), d's own bound through |W| <= 1
    eb = 2.0 * (b1.reshape(-1, AF_DEC).sum(1) + 9.0 * U * np.abs(d1).reshape(-1, AF_DEC).sum(1))
    nb = b.shape[0]
    bp = np.concatenate([np.zeros(win - 1, complex), b])
    ebp = np.concatenate([np.zeros(win - 1), eb])
    ba = np.abs(bp.real) + np.abs(bp.imag)
    z = sum(bp[i:i + nb] for i in range(win))
    ez = sum(ebp[i:i + nb] for i in range(win)) + (win - 1) * U * sum(ba[i:i + nb] for i in range(win))
    zprev = np.concatenate([[0.0], z[:-1]])
    ezprev = np.concatenate([[0.0], ez[:-1]])
    Zn = np.abs(z.real) + np.abs(z.imag)
    Zp = np.abs(zprev.real) + np.abs(zprev.imag)
    eP = 4.0 * U * Zn * Zp + 2.0 * (ez * Zp + Zn * ezprev + ez * ezprev)
    return _disc(z * np.conj(zprev), eP, loose)


# ---------------------------------------------------------------- SPEC 3.2: the filter at the loop's instants
def fir(d: np.ndarray, bd: np.ndarray, pos: np.ndarray, m: Modem, H: np.ndarray, *, p_off: int = 0, n_off: int = 0, **_):
    """y(pos) = sum_j H[p][j] d[n + T/2 - j], n = pos >> 16, p = (pos >> 11) & 31, and its bound: d's bounds through |H|, the two
    fmaf chains of T/2 terms and their sum ((T/2 + 1) u sum |H d|) and the taps' float32 rounding (u sum |H d|).
    Mutations: p_off (p +- 1), n_off (the history shifted)."""
    pos = np.asarray(pos, np.int64)
    n = (pos >> 16) + n_off
    p = ((pos >> 11) + p_off) & (NPHASE - 1)
    idx = np.clip(n[:, None] + m.T // 2 - np.arange(m.T)[None, :], 0, d.shape[0] - 1)
    Hp = H[p]
    dv, bv = d[idx], bd[idx]
    y = (Hp * dv).sum(1)
    aH = np.abs(Hp)
    by = (aH * bv).sum(1) + (m.T // 2 + 2) * U * (aH * (np.abs(dv) + bv)).sum(1)
    return y, by


def _rint_iv(v, e):
    """the integers rint(x) can be for |x - v| <= e: (rint(v), the largest distance from it)"""
    c = np.rint(v)
    return c, np.maximum(np.rint(v + e) - c, c - np.rint(v - e))


def _clamp_q(v, e, lim, scale):
    """rint(scale clamp(v, +-lim)) for |x - v| <= e: (centre, slack) arrays"""
    return _rint_iv(scale * np.clip(v, -lim, lim), scale * e)


@dataclass
class Check:
    """worst error of one scene as a fraction of each bound, and the ambiguous bits; with hidden states (replay's states[j] = None):
    the spans between observed states, those left unresolved (the candidate set outgrew its limit: counted, not asserted), and, where the
    caller gave the true hidden states, how many of them lay outside the carried set"""
    worst: dict
    amb: int = 0
    nbits: int = 0
    ntiles: int = 0
    spans: int = 0
    unresolved: int = 0
    hidden: int = 0
    outside: int = 0
    cands: int = 0

    def put(self, key, frac):
        self.worst[key] = max(self.worst.get(key, 0.0), float(frac))

    def line(self, name: str) -> str:
        w = " ".join(f"{k}={v:.3g}" for k, v in sorted(self.worst.items()))
        blk = f" spans={self.spans} unresolved={self.unresolved} candidates<={self.cands}" if self.spans != self.ntiles else ""
        return (f"DEMOD-REF {name}: tiles={self.ntiles}{blk} bits={self.nbits} ambiguous={self.amb} "
                f"({self.amb / max(self.nbits, 1):.2e}) {w}")

    def failures(self):
        return {k: v for k, v in self.worst.items() if not v <= 1.0}


def initial_state(m: Modem) -> dict:
    """SPEC 3.2: t_next = (32 << 16) + period0, amp = 0.25, everything else 0"""
    return dict(t_next=(32 << 16) + m.period0, period=m.period0, bias=0.0, amp=0.25, afc_u=0.0)


CAND_LIMIT = 256                 # candidate states carried through hidden tiles at most; a span that needs more is unresolved


@dataclass
class _Cand:
    """a state the product may be in: the integers exactly, the two floats as centre and error; the position in the span's bits and
    what the chain that led here has accumulated"""
    t: int
    period: int
    bias: float
    eb: float
    amp: float
    ea: float
    nstat: int
    off: int = 0
    amb: int = 0
    nbits: int = 0
    fr: dict | None = None


def replay(d: np.ndarray, bd: np.ndarray, m: Modem, states: list, bits: list, *, afc: bool, chk: Check | None = None,
           cutoff: float = CUTOFF, normalise: bool = True, mid_sign: int = -1, gardner_k0: bool = False,
           gardner_k256: bool = False, e_over_k: bool = False, slack: int = SLACK, pclamp: int = 8, acq_tiles: int = 3,
           afc_lag: int = 3, afc_gain: float = AFC_GAIN, afc_leak: float = AFC_LEAK, shift_sign: int = -1,
           jump_ratio: int = 17, cand_limit: int = CAND_LIMIT, truth: list | None = None, **mut) -> Check:
    """Check every tile of one channel against one step of the SPEC's recurrence.
    d, bd: the discriminator stream (disc_*) and its bound; states[j], bits[j]: the product's state and new bits after tile j;
    afc: the stream is IQ (the AFC, 3.0d and 3.0e act).  Returns a Check whose worst fractions must all be <= 1.
    Keys: count (exact), bit, dphase, dper, bias, amp, jump, afc.

    states[j] may be None: tile j's end state is not observable (a channelizer bin's smallest submit is a block of 3 tiles).  bits then
    has one entry per OBSERVED state: the bits of the span of tiles that ends there, concatenated.  A span is accepted if and only if
    there is a chain of per-tile steps of the recurrence from the observed state before it to the observed state after it whose every
    step lies within the bounds, whose counts add up to the span's count exactly, and which reproduces every bit that is not ambiguous.
    Mechanism: a set of candidate states after each hidden tile.  t_next and period are integers and every value their rint intervals
    allow is enumerated (candidates that agree in both are merged: the hull of their intervals); bias and amp are carried as a centre
    and the error this replay already computes, which widens the ambiguity
    test (gap <= by + e_bias), the Gardner term's bound and, twice, the relative error of err (amp squared).  A candidate's (t, period)
    fix its tile's bit count; one whose counts overrun the span's bits, or which an unambiguous bit contradicts, is dropped.  At the
    span's end the observed state is tested against every surviving candidate with the tests of the observed case and the candidate
    with the smallest worst fraction is reported.  More than cand_limit candidates: the span is unresolved (Check.unresolved).  Only
    the non-AFC path without the tone front-end supports hidden states.  With every state observed each span is one tile and the one
    candidate has zero error: the computation is the one-step check, term for term.
    truth (optional): the states the product really had after every tile; Check.outside counts the hidden ones that are not in the
    carried set (t_next and period among the candidates, bias and amp inside a matching candidate's intervals)."""
    chk = chk or Check({})
    H = taps(m, cutoff=cutoff, normalise=normalise)
    hidden_mode = any(s is None for s in states)
    assert not hidden_mode or (not afc and m.pre == 1 and m.rounds == 1), "hidden states: the non-AFC, pre == 1 path only"
    assert states[-1] is not None and len(bits) == sum(s is not None for s in states)
    u_after = np.array([s["afc_u"] for s in states], np.float64) if afc else None
    prev = initial_state(m)
    nstat = 0
    kp = m.period0 * (0.5 / math.pi)
    e_kp = 2.0 * U * kp
    pmin, pmax = m.period0 - (m.period0 >> pclamp), m.period0 + (m.period0 >> pclamp)
    cl = lambda q: min(max(q, pmin), pmax)

    def k_total(j, c):
        limit = (((m.itile * (j + 1)) - 1 - m.T // 2 - slack) << 16) | 0xFFFF
        return (limit - c.t) // c.period + 1 if c.t <= limit else 0

    def tile(j, c, b, st):
        """one tile from candidate c with the bits b (len(b) == k_total): st observed -> the fractions of every test (dict), or
        "skip" (SRS-C50's first round); st None -> the list of candidates after the tile ([] if a bit contradicts c)"""
        fr = {}
        n0 = m.itile * (j + 1)
        t, period, bias, amp, eb, ea = c.t, c.period, c.bias, c.amp, c.eb, c.ea
        K_total = b.shape[0]
        K = min(K_total, m.rmax)
        namb = 0
        if K:
            k = np.arange(K)
            pos = t + k * period
            y, by = fir(d, bd, pos, m, H, **mut)
            bb = b[:K]
            # (b) each bit
            gap = np.abs(y - bias)
            amb = gap <= by + eb
            wrong = (bb != (y > bias)) & ~amb
            namb = int(amb.sum())
            fr["bit"] = (gap[wrong] / np.maximum(by[wrong] + eb, 1e-300)).max() if wrong.any() else 0.0
            if st is None and wrong.any():
                c.fr = fr
                return []
        if m.rounds > 1 and K_total > m.rmax:
            # SRS-C50: only the end of the second round is observable; the first round's bits are checked above
            c.fr, c.amb, c.nbits = fr, c.amb + namb, c.nbits + K
            return "skip"
        ns = c.nstat
        if K:
            kg = k[(k % 64 != 0) | gardner_k0]
            kg = kg[(kg < ROUND) | gardner_k256]
            kg = kg[kg >= 1]
            nm = min(K, ROUND) if not gardner_k256 else K
            mm, bm = fir(d, bd, pos[:nm] + mid_sign * (period >> 1), m, H, **mut)
            # (c) integer sums from the product's decisions
            Yc, Ys = _clamp_q(y, by + U * np.abs(y), 8.0, 4096.0)
            one = bb == 1
            S1, eS1 = Yc[one].sum(), Ys[one].sum()
            S0, eS0 = Yc[~one].sum(), Ys[~one].sum()
            C1 = int(one.sum())
            C0 = K - C1
            a = y[kg - 1] - y[kg]
            ea_ = by[kg - 1] + by[kg] + U * np.abs(a)
            bmv = mm[kg] - bias
            ebm = bm[kg] + U * np.abs(bmv) + eb
            e = a * bmv
            ee = ea_ * np.abs(bmv) + np.abs(a) * ebm + ea_ * ebm + U * (np.abs(a) + ea_) * (np.abs(bmv) + ebm)
            Ec, Es = _clamp_q(e, ee, 1e6 / 1024.0, 1024.0)
            E, eE = Ec.sum(), Es.sum()
            if m.pre == 8:
                sy, esy = _clamp_q(np.clip(np.abs(y[kg] - bias), 0, 8), by[kg] + U * np.abs(y[kg] - bias), 8.0, 4096.0)
                sm, esm = _clamp_q(np.clip(np.abs(mm[kg] - bias), 0, 8), bm[kg] + U * np.abs(mm[kg] - bias), 8.0, 4096.0)
                SY, eSY, SM, eSM = sy.sum(), esy.sum(), sm.sum(), esm.sum()
            # slicer levels
            if C1 > 0 and C0 > 0:
                hi, ehi = S1 / C1 / 4096.0, eS1 / C1 / 4096.0 + abs(S1 / C1 / 4096.0) * (RECIP_ERR + U)
                lo, elo = S0 / C0 / 4096.0, eS0 / C0 / 4096.0 + abs(S0 / C0 / 4096.0) * (RECIP_ERR + U)
                cc, ec = 0.5 * (hi + lo), 0.5 * (ehi + elo) + U * abs(0.5 * (hi + lo))
                av, ev = 0.5 * (hi - lo), 0.5 * (ehi + elo) + U * abs(0.5 * (hi - lo))
                if ns == 0:
                    nb, enb, na, ena = cc, ec, av, ev
                else:
                    # (the carried errors: half of each goes through the average, a rounding's share of it on top)
                    nb = bias + 0.5 * (cc - bias)
                    enb = 0.5 * ec + 0.5 * U * abs(cc - bias) + U * abs(nb) + (0.5 + 2 * U) * eb
                    na = amp + 0.5 * (av - amp)
                    ena = 0.5 * ev + 0.5 * U * abs(av - amp) + U * abs(na) + (0.5 + 2 * U) * ea
                if na < 1e-3:
                    na, ena = float(np.float32(1e-3)), ena + 1e-10
                ns = 1
            else:
                nb = (S1 + S0) / K / 4096.0
                enb = (eS1 + eS0) / K / 4096.0 + abs(nb) * (RECIP_ERR + U)
                na, ena = amp, 0.0 + ea
            if m.pre == 1 and n0 <= acq_tiles * m.itile:
                nb = (S1 + S0) / K / 4096.0
                enb = (eS1 + eS0) / K / 4096.0 + abs(nb) * (RECIP_ERR + U)
            if st is not None:
                fr["amp"] = abs(st["amp"] - na) / max(ena, 1e-300) if st["amp"] != na else 0.0
            # loop filter, from the product's amplitude (observable after the tile: only the round changes it); hidden: from the
            # carried one, whose relative error r enters 1 / amp^2 as at most 1 / (1 - r)^2 - 1
            N = K if e_over_k else min(K, ROUND)
            if st is not None:
                ampp, rel = np.float64(np.float32(st["amp"])), 0.0
            else:
                r_ = ena / na
                ampp, rel = np.float64(na), (1.0 / (1.0 - r_) ** 2 - 1.0 if r_ < 0.5 else math.inf)
            a2 = ampp * ampp
            err = E / N / 1024.0 / a2
            eerr = (eE + U * abs(E)) / N / 1024.0 / a2 + abs(err) * (2 * RECIP_ERR + 4 * U)
            if rel:
                eerr = eerr * (1.0 + rel) + abs(err) * rel
            errc = min(max(err, -1.0), 1.0)
            v = errc * kp
            ev = eerr * kp + abs(errc) * e_kp + U * abs(v)
            if st is None:
                if not math.isfinite(ev):
                    return None
                out = []
                pers = sorted({cl(period + q) for q in range(int(np.rint((v - ev) / 4096.0)), int(np.rint((v + ev) / 4096.0)) + 1)})
                for q in range(int(np.rint(v - ev)), int(np.rint(v + ev)) + 1):
                    for p2 in pers:
                        out.append(_Cand(t + K * period + q, p2, nb, enb, na, ena, ns, c.off + K_total, c.amb + namb, c.nbits + K))
                return out
            dph_c, dph_s = _rint_iv(v, ev)
            dpr_c, dpr_s = _rint_iv(v / 4096.0, ev / 4096.0)
            dphase = st["t_next"] - t - K * period
            jumps = [0]
            if m.pre == 8 and ns:
                # 16 SM > 17 SY with SM, SY within their slack: the jump is certain, excluded or either
                lo_ = 16 * (SM - eSM) - jump_ratio * (SY + eSY)
                hi_ = 16 * (SM + eSM) - jump_ratio * (SY - eSY)
                jumps = [period >> 1] if lo_ > 0 else ([0] if hi_ <= 0 else [0, period >> 1])
            ok = [abs(dphase - jj - dph_c) <= dph_s for jj in jumps]
            fr["dphase"] = min(abs(dphase - jj - v) / (ev + 0.5) for jj in jumps) if any(ok) else math.inf
            if m.pre == 8:
                fr["jump"] = 0.0 if any(ok) else math.inf
            # period += rint(err ki), clamped to period0 (1 +- 1/256): the clamp is monotone, so the interval maps through it
            if cl(period + dpr_c - dpr_s) <= st["period"] <= cl(period + dpr_c + dpr_s):
                fr["dper"] = abs(st["period"] - cl(period + v / 4096.0)) / (ev / 4096.0 + 0.5)
            else:
                fr["dper"] = math.inf
        else:
            nb, enb = bias, 0.0 + eb
            if st is None:
                return [_Cand(t, period, bias, eb, amp, ea, ns, c.off, c.amb, c.nbits)]
            fr["dphase"] = 0.0 if st["t_next"] == t and st["period"] == period else math.inf
        # 3.0e and 3.0b
        if afc:
            uf = lambda i: u_after[i] if i >= 0 else 0.0
            u0, u1 = uf(j - afc_lag), uf(j - afc_lag + 1)
            shift = rot(u1) - rot(u0)
            bias_after = nb + shift_sign * shift
            eba = enb + 2 * (ROT_FIT_ERR + 6 * U) + U * abs(shift) + U * abs(bias_after)
            uprev = uf(j - 1)
            un = min(max(afc_gain * nb + (1.0 - afc_leak) * uprev, -AFC_MAX), AFC_MAX)
            eu = AFC_GAIN * enb + 1e-8 * abs(nb) + 2 * U * (abs(uprev) + abs(un))
            fr["afc"] = abs(st["afc_u"] - un) / max(eu, 1e-300) if st["afc_u"] != un else 0.0
        else:
            bias_after, eba = nb, enb
        fr["bias"] = abs(st["bias"] - bias_after) / max(eba, 1e-300) if st["bias"] != bias_after else 0.0
        c.fr, c.amb, c.nbits, c.nstat = fr, c.amb + namb, c.nbits + K, ns
        return fr

    def merge(cands):
        """candidates that agree in the integers (and in the position in the span's bits) are one: the hull of their intervals.  Chains
        that differ by a count in one tile meet again in the next, so the set grows with the sum of the slacks, not their product."""
        out = {}
        for c in cands:
            o = out.setdefault((c.t, c.period, c.off, c.nstat), c)
            if o is not c:
                for v, e in (("bias", "eb"), ("amp", "ea")):
                    lo = min(getattr(o, v) - getattr(o, e), getattr(c, v) - getattr(c, e))
                    hi = max(getattr(o, v) + getattr(o, e), getattr(c, v) + getattr(c, e))
                    setattr(o, v, 0.5 * (lo + hi))
                    setattr(o, e, 0.5 * (hi - lo) * (1.0 + 4 * U) + 4 * U * abs(0.5 * (lo + hi)))
                o.amb, o.nbits = max(o.amb, c.amb), max(o.nbits, c.nbits)
        return list(out.values())

    def inside(cands, tr):
        return any(c.t == tr["t_next"] and c.period == tr["period"] and abs(tr["bias"] - c.bias) <= c.eb
                   and abs(tr["amp"] - c.amp) <= c.ea for c in cands)

    j, si = 0, 0
    ntiles = len(states)
    while j < ntiles:
        j1 = j
        while states[j1] is None:
            j1 += 1
        st = states[j1]
        sb = np.asarray(bits[si], np.int64)
        si += 1
        chk.ntiles += j1 - j + 1
        chk.spans += 1
        cands = [_Cand(prev["t_next"], prev["period"], prev["bias"], 0.0, prev["amp"], 0.0, nstat)]
        resolved = True
        last_fr = {}
        for jj in range(j, j1):                                  # the hidden tiles
            nxt = []
            for c in cands:
                kt = k_total(jj, c)
                if c.off + kt > sb.shape[0]:
                    last_fr = {"count": math.inf}
                    continue
                out = tile(jj, c, sb[c.off:c.off + kt], None)
                if out is None:
                    resolved = False
                    break
                if not out:
                    last_fr = c.fr
                nxt += out
            nxt = merge(nxt)
            if not resolved or len(nxt) > cand_limit:
                resolved = False
                break
            cands = nxt
            chk.cands = max(chk.cands, len(cands))
            if truth is not None and cands:
                chk.hidden += 1
                chk.outside += 0 if inside(cands, truth[jj]) else 1
            if not cands:
                break
        if not resolved:
            chk.unresolved += 1
        elif not cands:
            # no chain reaches this span's end: what dropped the last candidate says why
            for k_, v_ in last_fr.items():
                if not v_ <= 1.0:
                    chk.put(k_, v_)
            chk.put("chain", math.inf)
        else:
            best = None
            for c in cands:
                kt = k_total(j1, c)
                if c.off + kt != sb.shape[0]:
                    continue
                fr = tile(j1, c, sb[c.off:], st)
                w = 0.0 if fr == "skip" else max(fr.values(), default=0.0)
                if best is None or w < best[0]:
                    best = (w, c, fr)
            chk.put("count", 0.0 if best is not None else math.inf)
            if best is None:
                return chk
            _, c, fr = best
            chk.amb += c.amb
            chk.nbits += c.nbits
            if fr == "skip":
                chk.put("bit", c.fr.get("bit", 0.0))
            else:
                for k_, v_ in fr.items():
                    chk.put(k_, v_)
                nstat = c.nstat
        prev = st
        if not resolved or not cands:
            nstat = 1 if hidden_mode else nstat
        j = j1 + 1
    return chk
