"""The oracle's wideband and VFO front-ends (oracle/or_chan.c) against the float64 reference of tests/fe_reference.py, which is
written from DESIGN.md section 3 alone: tables, filter-bank phases (even and odd stacking, several consecutive blocks),
discriminator + resampler rows, under error bounds that are formulas.  The mutation checks at the end perturb the REFERENCE
the way the bugs these bounds exist for would perturb a kernel (a tap off by one, a history one sample short, ...) and assert
that the comparison then fails.  The GPU half (test_gpu_frontend_reference.py) applies the same to the HIP kernels."""
import math

import numpy as np
import pytest

import fe_reference as R
from sdrpp_radiosonde_amd import _lib, synth

HALF = R.BIN_HZ / 2
TONE_BINS = (0, 1, 255, 256, 257, 511)
OFFSETS = (0.0, 5000.0, -5000.0, 9500.0, -9500.0, HALF)
NBLK = 3                      # the carried 7692 samples are used twice


def tone_scene(rot: int, n: int) -> np.ndarray:
    """the six edge bins, bin i at offset OFFSETS[(i + rot) % 6]"""
    return R.tones(n, [(k, OFFSETS[(i + rot) % 6], 1.0) for i, k in enumerate(TONE_BINS)], seed=rot)


def scenes():
    """{name: float32 IQ [n, 2]} generators; NBLK consecutive blocks, the rotated tone scenes one block each"""
    n = NBLK * R.STEPS * R.D
    n1 = R.STEPS * R.D
    return {
        "tones0": lambda: R.as_iq32(tone_scene(0, n)),
        "tones2": lambda: R.as_iq32(tone_scene(2, n1)),
        "tones4": lambda: R.as_iq32(tone_scene(4, n1)),
        # a weak tone in bin 100 beside one 40 dB stronger in bin 101 (the stop band); a tone at the 20 kS/s alias of bin 300's;
        # a chirp across bins 380 .. 384 and both block boundaries
        "stopband_alias_chirp": lambda: R.as_iq32(R.tones(n, [(100, 1000.0, 0.01), (101, 0.0, 1.0), (300, 1000.0, 0.3), (300, 21000.0, 0.3)], seed=5)
                                                  + R.chirp(n, 379.6, 384.4)),
        "noise": lambda: R.as_iq32(R.noise(n, 1.0, seed=7)),
        "rs41": lambda: synth.make_wideband_rs41([3, 256, 400], n, seed=12, ebn0_db=25.0)[0].numpy(),
        # integer receivers at full scale (clipped): the values +-32767 and -128 occur
        "int16": lambda: R.as_int_iq(0.45 * tone_scene(1, n) / 3 + 0.2 * R.noise(n, 1.0, seed=9), 16).astype(np.float32),
        "int8": lambda: R.as_int_iq(0.5 * tone_scene(3, n) / 3 + 0.3 * R.noise(n, 1.0, seed=10), 8).astype(np.float32),
    }


def oracle_chan(oracle, iq32: np.ndarray, odd: bool, rows: bool = True):
    """the oracle's bank block by block: (16-bit phases [512, n] int64, 48 kS/s rows [512, n * 12 / 5] or None)"""
    L = oracle.lib()
    ch = L.or_chan_new_odd() if odd else L.or_chan_new()
    nblk = iq32.shape[0] // (R.STEPS * R.D)
    ph, o48 = [], []
    for b in range(nblk):
        blk = np.ascontiguousarray(iq32[b * R.STEPS * R.D:(b + 1) * R.STEPS * R.D]).reshape(-1)
        bins = np.zeros((512, R.STEPS), np.float32)
        out48 = np.zeros((512, R.STEPS * 12 // 5), np.float32) if rows else None
        L.or_chan_block(ch, oracle.fptr(blk), R.STEPS, oracle.fptr(bins.reshape(-1)), oracle.fptr(out48.reshape(-1)) if rows else None)
        ph.append(np.rint(bins.astype(np.float64) * 16384).astype(np.int64) & 0xFFFF)
        o48.append(out48)
    L.or_chan_free(ch)
    return np.concatenate(ph, axis=1), (np.concatenate(o48, axis=1) if rows else None)


# the bins whose rows are checked (the resampler is the same for every bin): every 8th and the edges and signals of the scenes
ROW_BINS = np.unique(np.r_[np.arange(0, 512, 8), TONE_BINS, 100, 101, 300, 301, 380, 381, 382, 383, 384, 3, 256, 400])


def chan_rows_ratio(q, rows, **mut):
    """float32 48 kS/s rows against the 12/5 resampler (float64, taps from their definition) applied to the same phases q:
    worst |difference| / bound per bin (q, rows: the same bins)"""
    g = R.resamp_taps(20000)
    d = R.chan_disc(q)
    o, S1, S2, _ = R.resample(d, g, 12, 5, **mut)
    return ratio(np.abs(rows.astype(np.float64) - o), R.row_bound(S1, S2)).max(axis=1)


def ratio(err, bound):
    """err / bound, where a zero bound (all-zero inputs) admits exactly zero"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))


_cache = {}


def scene_result(oracle, name):
    """(iq32, {odd: (oracle phases, oracle rows, Y, A)}) for a scene, computed once per session"""
    if name not in _cache:
        iq = scenes()[name]()
        x = iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)
        res = {}
        for odd in (False, True):
            q, rows = oracle_chan(oracle, iq, odd)
            Y, A = R.bank(x, odd)
            res[odd] = (q, rows, Y, A)
        _cache[name] = (iq, res)
    return _cache[name]


# ================================================================ tables
def test_tables_are_the_definitions():
    """The product's tables (host code) are float32 of the float64 definitions within 1 ulp; twiddles 0 and 128 exact (SPEC 3.5,
    round 6); the VFO taps at every rate the same."""
    L = _lib.load()
    h = np.zeros(8192, np.float32)
    tw = np.zeros(512, np.float32)
    g = np.zeros(192, np.float32)
    assert L.sonde_chan_tables(h.ctypes.data, tw.ctypes.data, g.ctypes.data) == 0

    def within_ulp(got, want, floor=0.0):
        want = np.asarray(want, np.float64)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        return np.all(np.abs(got.astype(np.float64) - want) <= np.maximum(ulp, floor))
    assert within_ulp(h, R.proto())
    w = R.twiddles()
    # components of a unit-modulus value: one ulp of 1/2 where the component itself rounds near zero
    assert within_ulp(tw[0::2], w.real, 2.0 ** -25) and within_ulp(tw[1::2], w.imag, 2.0 ** -25)
    assert tw[0] == 1.0 and tw[1] == 0.0 and tw[256] == 0.0 and tw[257] == -1.0
    assert within_ulp(g.reshape(12, 16), R.resamp_taps(20000))
    for rate in R.VFO_RATES:
        up, down, _ = R.vfo_ratio(rate)
        gv = np.zeros((up, 16), np.float32)
        assert L.sonde_vfo_taps(rate, gv.ctypes.data) == 0
        assert within_ulp(gv, R.resamp_taps(rate)), rate
        a, b = _lib.C.c_int(), _lib.C.c_int()
        assert L.sonde_vfo_ratio(rate, _lib.C.byref(a), _lib.C.byref(b)) == 0 and (a.value, b.value) == (up, down)


def test_atan2q_reference_is_the_spec(oracle):
    """atan2q_ref against the oracle's float32 atan2q (SPEC 3.1) within the float32 evaluation error, signed zeros exactly, and
    against arctan2 within SPEC 3.1's documented error"""
    L = oracle.lib()
    rng = np.random.default_rng(3)
    th = rng.uniform(-np.pi, np.pi, 4000)
    mag = 10.0 ** rng.uniform(-36, 36, th.size)
    y = (mag * np.sin(th)).astype(np.float32)
    x = (mag * np.cos(th)).astype(np.float32)
    got = np.array([L.or_atan2(float(a), float(b)) for a, b in zip(y, x)])
    assert np.abs(got - R.atan2q_ref(y, x)).max() <= R.ATAN2Q_EVAL_ERR
    for yy, xx, want in ((0.0, -0.0, 2.0), (-0.0, -0.0, -2.0), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
        assert abs(R.atan2q_ref(yy, xx) - want) <= R.ATAN2Q_EVAL_ERR and math.copysign(1, R.atan2q_ref(yy, xx)) == math.copysign(1, want)
    th = np.linspace(-np.pi, np.pi, 400001)
    e = np.abs(R.atan2q_ref(np.sin(th), np.cos(th)) - th * 2 / np.pi)
    assert np.minimum(e, 4 - e).max() <= R.ATAN2Q_MAX_ERR


# ================================================================ the oracle's filter bank
@pytest.mark.parametrize("name", list(scenes()))
def test_oracle_bank_phases_and_rows(oracle, name):
    """even and odd stacking, NBLK consecutive blocks: every phase within the tight bound of atan2q_ref(Y) and the loose one of
    arctan2(Y); the unfused 48 kS/s rows within the row bound of the 12/5 resampler applied to the oracle's own phases"""
    iq, res = scene_result(oracle, name)
    if name in ("int16", "int8"):
        top = 32767 if name == "int16" else 127
        assert iq.max() == top and iq.min() == (-32767 if name == "int16" else -128)
    for odd in (False, True):
        q, rows, Y, A = res[odd]
        r = R.phase_errors(q, Y, A, odd)
        assert r.max() <= 1.0, (odd, r.max(), np.unravel_index(r.argmax(), r.shape))
    q, rows, Y, A = res[False]                       # the loose layer (the approximant) and the resampler: one bank is enough
    rl = R.phase_errors(q, Y, A, False, loose=True)
    assert rl.max() <= 1.0, rl.max()
    assert chan_rows_ratio(q[ROW_BINS], rows[ROW_BINS]).max() <= 1.0


# ================================================================ the oracle's VFO front-end
def vfo_signals(rate: int, n: int):
    """[(name, float32 IQ [n, 2], tight_only)]: a tone sweep over +-R/2 (every quadrant of the phase step, the +-2 wrap),
    FM near the resampler's cutoff, phase noise, levels over 36 decades, exact-zero dropouts"""
    up, down, fc = R.vfo_ratio(rate)
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(rate)
    f = np.linspace(-0.5, 0.5, n) * rate                                   # sweep -R/2 .. R/2
    sweep = np.exp(1j * 2 * np.pi * np.cumsum(f) / rate)
    fm = np.exp(1j * (0.9 * np.sin(2 * np.pi * 0.95 * fc * t / rate) + 0.6 * np.sin(2 * np.pi * 0.7 * fc * t / rate + 1.0)))
    pn = np.exp(1j * np.cumsum(rng.uniform(-1.3, 1.3, n)))
    out = [("sweep", sweep, False), ("fm", fm, False), ("phase_noise", pn, False)]
    lv = 10.0 ** np.repeat(np.arange(-18, 19, 3), -(-n // 13))[:n]         # 1e-18 .. 1e18 in steps of 1e3
    out.append(("levels", pn * lv, True))
    lv2 = 10.0 ** np.repeat(np.arange(-9, 10, 3), -(-n // 7))[:n]          # |z| > 1e-12: the loose layer holds
    out.append(("levels_loose", sweep * lv2, False))
    drop = fm * 0.7
    drop[200:260] = 0.0
    drop[n // 2: n // 2 + 3] = 0.0
    drop[0] = -0.5 - 0.25j                                                  # x[0] in the third quadrant: atan2q(+-0, -0) = +-2
    out.append(("dropouts", drop, False))
    return [(nm, R.as_iq32(s), tight) for nm, s, tight in out]


def vfo_ratio_of(got, iq, rate, loose=False, **mut):
    o, b, valid = R.vfo_rows_ref(iq, rate, loose=loose, **mut)
    r = ratio(np.abs(got.astype(np.float64) - o), b)
    return np.where(valid, r, 0.0).max(), valid


@pytest.mark.parametrize("rate", R.VFO_RATES)
def test_oracle_vfo_rows(oracle, rate):
    """or_vfo at every rate, fed in ragged pieces: rows within the tight bound of the atan2q_ref chain and the loose bound of
    the arctan2 chain (levels above 1e-12 only: below, the discriminator reads toward 0 by design)"""
    up, down, _ = R.vfo_ratio(rate)
    n = 600 * down
    for name, iq, tight_only in vfo_signals(rate, n):
        v = oracle.Vfo(rate)
        cuts = [0, down, 7 * down, 8 * down, 200 * down, n]
        got = np.concatenate([v.process(iq[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
        rt, _ = vfo_ratio_of(got, iq, rate)
        assert rt <= 1.0, (name, rt)
        if not tight_only:
            rl, valid = vfo_ratio_of(got, iq, rate, loose=True)
            assert rl <= 1.0 and valid.mean() > 0.9, (name, rl, valid.mean())


def test_vfo_signed_zero_first_sample(oracle):
    """trap: x[-1] = 0 and x[0] in the third quadrant: the first discriminator sample is atan2q(+-0, -0) = +-2 (SPEC 3.1) and the
    tight reference reproduces it"""
    iq = R.as_iq32(np.array([-0.5 - 0.25j, -0.4 - 0.3j, 0.2 + 0.1j, 0.0, 0.3 - 0.1j] * 5))
    d, amb, lok, _ = R.vfo_disc(iq)
    L = oracle.lib()
    want = np.zeros(iq.shape[0], np.float32)
    last = np.zeros(2, np.float32)
    L.or_discriminate(oracle.fptr(np.ascontiguousarray(iq).reshape(-1)), iq.shape[0], oracle.fptr(want), oracle.fptr(last))
    assert abs(abs(d[0]) - 2.0) < 1e-6 and want[0] == np.float32(d[0]) and not lok[0]
    assert np.abs(want - d).max() <= R.ATAN2Q_EVAL_ERR


# ================================================================ mutation self-checks
def test_mutations_of_the_bank_reference_are_caught(oracle):
    """Each perturbation of the REFERENCE the way a kernel bug would perturb the arithmetic makes the comparison with the
    (correct) oracle outputs fail: the bounds are tight enough to catch what they exist for."""
    iq, res = scene_result(oracle, "tones0")
    n1 = R.STEPS * R.D                                     # one block is enough to see each of them
    x = iq[:n1, 0].astype(np.float64) + 1j * iq[:n1, 1].astype(np.float64)
    for odd in (False, True):
        q = res[odd][0][:, :R.STEPS]
        for kw in ({"h": R.proto(1)}, {"h": R.proto(-1)}, {"hist": R.HIST - 1}) + (({"twist": +1},) if odd else ()):
            Y, A = R.bank(x, odd, **kw)
            assert R.phase_errors(q, Y, A, odd).max() > 1.0, (odd, kw)
        if odd:
            Y, A = res[odd][2][:, :R.STEPS], res[odd][3][:R.STEPS]
            assert R.phase_errors(q, Y, A, odd, deramp_first=True).max() > 1.0
    q, rows = res[False][0][ROW_BINS], res[False][1][ROW_BINS]
    nq = R.STEPS
    for kw in ({"i0_off": -1}, {"p_off": 1}, {"p_off": -1}):
        assert chan_rows_ratio(q[:, :nq], rows[:, :nq * 12 // 5], **kw).max() > 1.0, kw


@pytest.mark.parametrize("rate", R.VFO_RATES)
def test_mutations_of_the_vfo_reference_are_caught(oracle, rate):
    up, down, _ = R.vfo_ratio(rate)
    n = 600 * down
    other = {10000: 15000, 15000: 10000, 20000: 15000, 40000: 50000, 50000: 40000}[rate]
    for name, iq, _ in vfo_signals(rate, n):
        if name not in ("fm", "phase_noise"):
            continue
        got = oracle.Vfo(rate).process(iq)
        assert vfo_ratio_of(got, iq, rate)[0] <= 1.0
        for kw in ({"i0_off": -1}, {"p_off": 1}, {"p_off": -1}, {"g": R.resamp_taps(rate, R.vfo_ratio(other)[2])}):
            assert vfo_ratio_of(got, iq, rate, **kw)[0] > 1.0, (name, kw)
