"""The carrier meter, the continuous retune and the tracking receiver on the GPU (DESIGN SPEC 3.11, 3.9) against
tests/track_reference.py: looks within a formula bound on rows of the real tuner, bit-identical however the stream is cut and through
strided rows, restart, the ring, refusals; retuned rows within the tuner's bound of the theta reference, the row's phase across the
boundary; then whole scenes of drifting sondes through WidebandReceiver(track=True), both chains, against the reference receiver."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import track_reference as TR
import tuner_reference as R
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeError
from sdrpp_radiosonde_amd.track import SondeTracker
from sdrpp_radiosonde_amd.tuner import SondeTuner, WidebandReceiver, tuner_taps
from test_track_reference import DRIFT, FS, GRANULE, N_SUB, SONDES, _cplx, drifting_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scene():
    iq, frames, symbols = drifting_scene()              # made on the CPU: the very samples the reference receiver takes
    return iq, frames, symbols


@pytest.fixture(scope="module")
def rows(scene):
    """[3, 49152, 2]: RS41 / DFM / M10 VFOs at 48 kHz over the first 8 granules of the scene"""
    iq = scene[0][:8 * GRANULE].to(DEV).contiguous()
    tu = SondeTuner(FS, 48_000, [(f, b) for f, _, b in TR.iq48_vfos(SONDES)], 8 * GRANULE)
    y = tu.process(iq).clone()
    tu.close()
    return y


def _sorted(looks):
    return looks[np.lexsort((looks["look"], looks["row"]))]


def _feed(tr, rows, cuts, out=None, read_each=False):
    got, a = [], 0
    for k in cuts:
        part = rows[:, a:a + k]
        if out is not None:
            out[:, :k] = part
            part = out[:, :k]
        tr.submit(part)
        a += k
        if read_each:
            got.append(tr.results()[0])
    assert a == rows.shape[1]
    got.append(tr.results()[0])
    return _sorted(np.concatenate(got))


# ---------------------------------------------------------------- the meter
@pytest.mark.parametrize("L,d", [(0, 0), (1024, 1), (12_288, 5)])
def test_looks_within_the_bound(rows, L, d):
    n = rows.shape[1]
    tr = SondeTracker(3, 48_000, n, look_samples=L, lag=d)
    assert (tr.look_samples, tr.lag) == ((L, d) if L else TR.defaults(48_000))
    looks = _feed(tr, rows, [n])
    host = rows.cpu().numpy().astype(np.float64)
    assert len(looks) == 3 * (n // tr.look_samples)
    for r in range(3):
        x = host[r, :, 0] + 1j * host[r, :, 1]
        A, P, M = TR.meter_ref(x, tr.look_samples, tr.lag)
        bnd = TR.bound(M, tr.look_samples)
        lk = looks[looks["row"] == r]
        assert np.array_equal(lk["look"], np.arange(len(A)))
        dev = np.stack([np.abs(lk["a_re"] - A.real), np.abs(lk["a_im"] - A.imag), np.abs(lk["p"] - P)], axis=1)
        print(f"row {r} L {tr.look_samples} d {tr.lag}: worst deviation / bound {float(np.max(dev / bnd)):.3f}")
        assert np.all(dev <= bnd), (r, float(np.max(dev / bnd)))
        assert np.all(np.abs(A) > 1000.0 * bnd[:, :2].max(axis=1))              # the looks carry signal: the bound is not vacuous
        # the host conversions of the looks
        e = tr.err_hz(lk)
        assert np.allclose(e, [TR.err_hz(48_000, tr.lag, a) for a in A], rtol=0, atol=0.5)
        assert np.allclose(tr.level_db(lk), [TR.level_db(p, tr.look_samples) for p in P], rtol=0, atol=1e-4)
        assert np.all(tr.quality(lk) > 0.0) and np.all(tr.quality(lk) <= 1.0)
    tr.close()


def test_looks_bit_identical_however_the_stream_is_cut_and_through_strided_rows(rows):
    n = rows.shape[1]                       # 49152 = 192 blocks
    one = _feed(SondeTracker(3, 48_000, n), rows, [n])
    assert len(one) == 30
    cuttings = [[256, 4864, 10_240, 33_792], [6144] * 8, [2560] * 19 + [512], [256] * 40 + [38_912]]
    for i, cuts in enumerate(cuttings):
        got = _feed(SondeTracker(3, 48_000, max(cuts)), rows, cuts, read_each=bool(i & 1))
        assert got.tobytes() == one.tobytes(), cuts
    buf = torch.full((3, 50_001, 2), float("nan"), device=DEV)             # rows an odd number of samples apart, longer than any submit
    got = _feed(SondeTracker(3, 48_000, 33_792), rows, cuttings[0], out=buf)
    assert got.tobytes() == one.tobytes()


def test_restart_makes_the_looks_those_of_a_stream_that_began_there(rows):
    n, g = rows.shape[1], 6144
    one = _feed(SondeTracker(3, 48_000, n), rows, [n])
    tr = SondeTracker(3, 48_000, n)
    tr.submit(rows[:, :g])
    tr.submit(rows[:, g:2 * g])
    before = _sorted(tr.results()[0])
    tr.restart(1)
    tr.submit(rows[:, 2 * g:])
    after = _sorted(tr.results()[0])
    fresh = _feed(SondeTracker(1, 48_000, n), rows[1:2, 2 * g:], [n - 2 * g])
    a1 = after[after["row"] == 1]
    assert len(fresh) == (n - 2 * g) // 4864 and np.array_equal(a1["look"], np.arange(len(fresh)))
    for k in ("a_re", "a_im", "p"):
        assert a1[k].tobytes() == fresh[k].tobytes(), k
    both = _sorted(np.concatenate([before, after]))
    for r in (0, 2):
        assert both[both["row"] == r].tobytes() == one[one["row"] == r].tobytes()
    b1 = before[before["row"] == 1]
    assert b1.tobytes() == one[(one["row"] == 1) & (one["look"] < 2)].tobytes()
    with pytest.raises(SondeError, match="no such row"):
        tr.restart(3)


def test_ring_keeps_the_newest_looks_and_counts_the_dropped(rows):
    tr = SondeTracker(3, 48_000, 1024, look_samples=256)
    assert tr.ring == 16
    for a in range(0, 6 * 1024, 1024):
        tr.submit(rows[:, a:a + 1024])
    looks, dropped = tr.results()
    assert list(dropped) == [8, 8, 8] and len(looks) == 48
    ref = _feed(SondeTracker(3, 48_000, 6 * 1024, look_samples=256), rows[:, :6 * 1024], [6 * 1024])
    assert _sorted(looks).tobytes() == ref[ref["look"] >= 8].tobytes()
    looks, dropped = tr.results()
    assert len(looks) == 0 and list(dropped) == [0, 0, 0]


def test_refusals(rows):
    with pytest.raises(SondeError, match="input_kind"):
        SondeTracker(3, 48_000, 2048, input_kind=_lib.INPUT_REAL)
    with pytest.raises(SondeError, match="look_samples"):
        SondeTracker(3, 48_000, 2048, look_samples=1000)
    with pytest.raises(SondeError, match="lag"):
        SondeTracker(3, 48_000, 2048, lag=65)
    with pytest.raises(SondeError, match="max_samples"):
        SondeTracker(3, 48_000, 1000)
    with pytest.raises(SondeError, match="rate"):
        SondeTracker(3, 1000, 2048)
    with pytest.raises(SondeError, match="sonde_track_create: no such HIP device"):
        SondeTracker(3, 48_000, 2048, device=torch.cuda.device_count())
    tr = SondeTracker(3, 48_000, 2048)
    with pytest.raises(SondeError, match="multiple of 256"):
        tr.submit(rows[:, :1000])
    with pytest.raises(SondeError, match="max_samples"):
        tr.submit(rows[:, :4096])
    with pytest.raises(SondeError, match="3 rows"):
        tr.submit(rows[:2, :2048])
    with pytest.raises(SondeError, match="REAL"):
        tr.submit(rows[:, :2048, 0])
    with pytest.raises(SondeError, match="device"):
        tr.submit(rows[:, :2048].cpu())
    import ctypes as C
    L = _lib.load()
    assert L.sonde_track_submit(tr.h, C.c_void_p(rows.data_ptr()), 2048, 1024, None) != 0 and b"row_stride" in L.sonde_last_error()
    assert len(tr.results()[0]) == 0


# ---------------------------------------------------------------- the continuous retune
def _int_stream(fs, n, seed, tones):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 900.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for amp, f in tones:
        x = x + 3000.0 * amp * np.exp(2j * np.pi * (f * t / fs + rng.uniform()))
    x = np.round(x)
    return x, torch.from_numpy(np.stack([x.real, x.imag], axis=1)).to(torch.float32).to(DEV)


def test_retuned_rows_within_the_tuner_bound_of_the_theta_reference():
    fs, r = 2_400_000, 20_000
    up, down = R.ratio(fs, r)
    subs = [40, 40, 25, 40]
    # per VFO and submit: (offset, continuous) -- continuous twice in a row, then a plain retune (theta back to 0), and the other way round
    plan = [[(-500_000, None), (-499_700, True), (-499_150, True), (31_234, False)],
            [(100_003, None), (700_000, False), (700_450, True), (700_450, None)]]
    x, dev = _int_stream(fs, sum(subs) * down, 9, ((0.4, 31_234), (0.4, 700_000), (0.4, -499_500)))
    tu = SondeTuner(fs, r, [p[0][0] for p in plan], max(subs) * down)
    g = tuner_taps(fs, r).astype(np.float64)
    ref = [TR.Tuner(x, fs, r, g, p[0][0]) for p in plan]
    a = 0
    for s, k in enumerate(subs):
        for v in range(2):
            f, cont = plan[v][s]
            if s and cont is not None:
                tu.retune(v, f, continuous=cont)
                ref[v].retune(f, continuous=cont)
        got = tu.process(dev[a:a + k * down].contiguous()).cpu().numpy()
        a += k * down
        for v in range(2):
            y, A = ref[v].process(k * down, want_A=True)
            bnd = R.bound(A, g.shape[1])
            assert np.all(np.abs(got[v, :, 0] - y.real) <= bnd) and np.all(np.abs(got[v, :, 1] - y.imag) <= bnd), (s, v)
            assert np.max(np.abs(y)) > 100.0 * np.max(bnd)
    assert ref[0].theta == 0 and ref[1].theta != 0
    assert tu.offsets == [31_234, 700_450]
    with pytest.raises(SondeError, match="inside the band"):
        tu.retune(0, 1_195_000, continuous=True)
    with pytest.raises(SondeError, match="no such VFO"):
        tu.retune(2, 0, continuous=True)


def test_row_phase_runs_on_across_a_continuous_retune():
    """a tone 700 Hz above the VFO, the VFO moves up by 333 Hz: the phase step between the last output before and the first after the
    boundary is no larger than between ordinary neighbours of that row (the larger of the two rates); the plain retune jumps"""
    fs, r, f0, df = FS, 48_000, 100_000, 333
    up, down = R.ratio(fs, r)
    n = 200 * down
    t = torch.arange(2 * n, dtype=torch.float64, device=DEV)
    ph = 2 * np.pi * (f0 + 700) / fs * t
    blk = torch.stack([torch.cos(ph), torch.sin(ph)], 1).to(torch.float32).contiguous()
    step = {}
    for cont in (True, False):
        tu = SondeTuner(fs, r, [(f0, 10_000)], n)
        a = tu.process(blk[:n]).clone()
        tu.retune(0, f0 + df, continuous=cont)
        y = torch.cat([a, tu.process(blk[n:])], 1)[0].cpu().numpy().astype(np.float64)
        y = y[:, 0] + 1j * y[:, 1]
        step[cont] = np.angle(y[1:] * np.conj(y[:-1]))
        tu.close()
    m = n * up // down
    old, new = 2 * np.pi * 700 / r, 2 * np.pi * (700 - df) / r
    ordinary = max(np.max(np.abs(step[True][m - 60:m - 10])), np.max(np.abs(step[True][m + 300:m + 350])))
    assert abs(ordinary - old) < 1e-4
    assert abs(step[True][m - 1]) <= ordinary + 1e-5
    assert np.all(step[True][m - 3:m + 3] <= old + 1e-4) and np.all(step[True][m - 3:m + 3] >= new - 1e-4)
    assert abs(step[False][m - 1]) > 10 * old


def test_plain_retune_is_unchanged():
    """continuous=False: the rows from the retune on are those of a tuner created at the new offset (\"as if tuned there since
    create\"), bit for bit, also after a continuous retune came before"""
    fs, r = 2_400_000, 20_000
    up, down = R.ratio(fs, r)
    x, dev = _int_stream(fs, 120 * down, 4, ((0.4, 31_234),))
    cuts = [dev[:40 * down].contiguous(), dev[40 * down:80 * down].contiguous(), dev[80 * down:].contiguous()]
    born = SondeTuner(fs, r, [31_000, 31_000], 40 * down)
    want = [born.process(c).cpu().numpy() for c in cuts]
    tu = SondeTuner(fs, r, [-500_000, 5_000], 40 * down)
    tu.process(cuts[0])
    tu.retune(0, 31_000)                       # the default is the plain retune
    tu.retune(1, 17_000, continuous=True)
    got1 = tu.process(cuts[1]).cpu().numpy()
    tu.retune(1, 31_000, continuous=False)
    got2 = tu.process(cuts[2]).cpu().numpy()
    assert got1[0].tobytes() == want[1][0].tobytes() and got1[1].tobytes() != want[1][1].tobytes()
    assert got2.tobytes() == want[2].tobytes()


# ---------------------------------------------------------------- the tracked receiver
def _run(rx, iq, n_used):
    got = []
    for a in range(0, n_used, rx.max_in):
        rx.submit(iq[a:a + rx.max_in])
        got.append(rx.frames())
    return np.concatenate(got)


def _offsets_per_submit(log, first, n_sub, count):
    """the offset in force at every submit, from a log of (first input sample, offset, ..)"""
    out, cur = [], first
    at = {a: o for a, o, _, _ in log}
    for s in range(count):
        cur = at.get(s * n_sub, cur)
        out.append(cur)
    return np.array(out)


@pytest.mark.parametrize("chain", ["iq48", "reference"])
def test_tracked_receiver_keeps_the_drifting_sondes(scene, chain):
    iq, frames, symbols = scene
    dev = iq.to(DEV).contiguous()
    types = [t for _, t in SONDES]
    rx = WidebandReceiver(FS, SONDES, chain=chain, track=True)
    assert rx.granule == (GRANULE if chain == "iq48" else 2 * GRANULE) and rx.max_in == rx.granule
    count = N_SUB * GRANULE // rx.granule
    n_used = count * rx.granule
    got = _run(rx, dev, n_used)
    sym = [int(s * n_used / (N_SUB * GRANULE)) for s in symbols]
    tally = TR.tally(got, types, frames, sym, 2 / 3)
    print(chain, "tracked (sent, decoded, sent in the last third, decoded there, stray):", tally)
    vfos = TR.iq48_vfos(SONDES) if chain == "iq48" else TR.reference_vfos(SONDES)
    _, log, ret = TR.receiver_ref(_cplx(iq[:n_used]), FS, vfos, rx.granule, track=True)
    for i, (sent, hit, _, _, stray) in enumerate(tally):
        assert sent >= 5 and sent - hit <= 1 and stray == 0, (chain, i, tally[i])
        assert len(rx.track_log[i]) >= count // 2
        mine = _offsets_per_submit(rx.track_log[i], SONDES[i][0], rx.granule, count)
        theirs = _offsets_per_submit(log[i], SONDES[i][0], rx.granule, count)
        worst = int(np.max(np.abs(mine - theirs)))
        print(chain, "sonde", i, "retunes", ret[i], "worst offset difference to the reference receiver", worst, "Hz; last offset", mine[-1])
        assert worst <= TR.DEADBAND_HZ, (chain, i, worst)
        assert rx.sondes[i][0] == rx.track_log[i][-1][1]
        assert abs(mine[-1] - SONDES[i][0]) > 2000           # it moved with the carrier
    rx.close()


def test_untracked_receiver_is_unchanged_and_loses_the_rs41(scene):
    iq, frames, symbols = scene
    dev = iq.to(DEV).contiguous()
    types = [t for _, t in SONDES]
    n_used = N_SUB * GRANULE
    a = WidebandReceiver(FS, SONDES, chain="iq48")
    b = WidebandReceiver(FS, SONDES, chain="iq48", track=False)
    assert not b.trackers and b.granule == a.granule
    fa, fb = _run(a, dev, n_used), _run(b, dev, n_used)
    assert fa.tobytes() == fb.tobytes() and b.track_log == [[], [], []]
    tally = TR.tally(fa, types, frames, symbols, 2 / 3)
    print("untracked:", tally)
    assert 2 * tally[0][3] < tally[0][2]
    a.close(); b.close()


def test_drift_in_the_ten_megasample_scene():
    """the eight-type scene of test_gpu_tuner.py at 10 MS/s with two of its sondes drifting, iq48 chain (one look acted on per 1.024 s
    submit): at most one missed frame per sonde, and the two VFOs end nearer their carriers than where they began"""
    from test_gpu_tuner import FS as FS10, N_SCENE, SCENE, _check_frames
    drift = [0.0] * len(SCENE)
    drift[0], drift[3] = 900.0, -1100.0                   # the RS41 and the M10
    iq, frames, symbols = synth.make_wideband_scene(SCENE, N_SCENE, fs=FS10, ebn0_db=20.0, seed=21, device=DEV, drift_hz_per_s=drift)
    iq = iq.contiguous()
    rx = WidebandReceiver(FS10, [(f, t) for f, t, _ in SCENE], chain="iq48", max_in=N_SCENE // 3, track=True)
    got = []
    for a in range(0, N_SCENE, rx.max_in):
        rx.submit(iq[a:a + rx.max_in])
        got.append(rx.frames())
    _check_frames(np.concatenate(got), SCENE, frames, symbols)
    for i in (0, 3):
        at, off, _, _ = rx.track_log[i][-1]
        true = SCENE[i][0] + drift[i] * at / FS10
        print("sonde", i, "log", [(a, o, round(e)) for a, o, e, _ in rx.track_log[i]], "carrier at the last retune", round(true))
        # the estimate is at least 0.4 of the true offset (tests/test_track_reference.py), or the VFO holds inside deadband / 0.4;
        # 300 Hz: the scene's own carrier offsets (cfo_max_hz)
        start = abs(SCENE[i][0] - true)
        assert abs(off - true) <= max(0.6 * start, TR.DEADBAND_HZ / 0.4) + 300.0, (i, off, true)
        assert (off - SCENE[i][0]) * drift[i] > 0
    for i in (1, 2, 4, 5, 6, 7):                           # the others stay within the deadband's reach of where they were put
        assert abs(rx.sondes[i][0] - SCENE[i][0]) <= TR.DEADBAND_HZ / 0.4 + 300.0, (i, rx.sondes[i])
    rx.close()
