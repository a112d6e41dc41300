"""The tuner, the carrier meter and the combiner beyond one launch of rows, and at the edges of their summation loops (DESIGN SPEC 3.9,
3.11, 3.14), on the scenes of tests/launch_edge_scenes.py against the float64 references and their derived bounds.

The three objects pass per-row parameters to their kernels by value, a fixed number of rows per launch (512 meter rows, 512 combiner
sondes, 64 active tuner slots); an object with more rows loops over launches, and the kernel indexes the by-value tables with the
launch index and device memory with the row.  Here every object runs three launches with arithmetic in each, rows restarted, retuned
and idle on both sides of the launch boundaries.  tests/test_launch_edges_reference.py shows on the same scenes (CPU) that a row whose
parameters were taken from the row 512 rows (64 slots) away would leave its bound by a factor above 100, that every edge named here
is reached, and that the bounds lie far below the signal.  Measured ratios and times: profiles/launch_edges_notes.md."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import combine_reference as CR
import launch_edge_scenes as LS
import track_reference as TR
import tuner_reference as R
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd import combine as cb
from sdrpp_radiosonde_amd.combine import SondeCombiner
from sdrpp_radiosonde_amd.track import SondeTracker
from sdrpp_radiosonde_amd.tuner import SondeTuner, tuner_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATE = LS.RATE
LOOK_FIELDS = ("look", "a_re", "a_im", "p")


def _dev(x):
    """complex [rows, n] of float32 values -> [rows, n, 2] float32 on the device"""
    return torch.from_numpy(LS.as_iq(x)).to(DEV)


# ---------------------------------------------------------------- carrier meter
def _meter_run(tr, rows, submits, behind):
    """restart the rows of `behind` at their boundaries, submit piece by piece (views into the whole rows), read once at the end:
    (looks, rows ascending and oldest first within a row; dropped)"""
    a = 0
    for s, k in enumerate(submits):
        for r, bs in behind.items():
            if s in bs:
                tr.restart(r)
        tr.submit(rows[:, a:a + k])
        a += k
    assert a == rows.shape[1]
    looks, dropped = tr.results()
    assert np.all(np.diff(looks["row"].astype(np.int64)) >= 0)
    return looks, dropped


def _by_row(looks, n_rows):
    at = np.searchsorted(looks["row"], np.arange(n_rows + 1))
    return [looks[at[r]:at[r + 1]] for r in range(n_rows)]


def _same_looks(a, b):
    return len(a) == len(b) and all(a[k].tobytes() == b[k].tobytes() for k in LOOK_FIELDS)


def _within_meter_bound(lk, x, L, d, restarts, what):
    """one row's looks against meter_ref restarted at the same samples; returns the worst deviation / bound"""
    idx, A, P, M, _ = LS.meter_expected(x, L, d, restarts)
    assert np.array_equal(lk["look"], idx), (what, lk["look"], idx)
    bnd = TR.bound(M, L)
    dev = np.stack([np.abs(lk["a_re"] - A.real), np.abs(lk["a_im"] - A.imag), np.abs(lk["p"] - P)], axis=1)
    assert np.all(dev <= bnd), (what, float(np.max(dev / bnd)))
    assert np.all(np.abs(A) > 1000.0 * bnd[:, :2].max(axis=1))
    return float(np.max(dev / bnd))


def test_meter_three_launches():
    """1030 rows (512 + 512 + 6), looks of 512 samples, lag 3, five submits, seven rows restarted around the launch boundaries"""
    c = LS.METER_LAUNCHES
    n_rows, L, d, submits, behind = c["rows"], c["L"], c["lag"], c["submits"], c["behind"]
    x = LS.carriers(n_rows, sum(submits), c["seed"])
    rows = _dev(x)
    tr = SondeTracker(n_rows, RATE, max(submits), look_samples=L, lag=d)
    assert tr.ring == LS.meter_ring_len(max(submits), L)
    looks, dropped = _meter_run(tr, rows, submits, behind)
    assert not dropped.any()
    per_row = _by_row(looks, n_rows)
    worst = 0.0
    for r in range(n_rows):
        worst = max(worst, _within_meter_bound(per_row[r], x[r], L, d, LS.restart_samples(submits, behind.get(r, ())), r))
    print(f"meter, three launches: worst deviation / bound {worst:.3f} over {len(looks)} looks")
    # the look counters began again at 0: a look 0 for every stretch between restarts that holds a whole look (rows 0 and 513 restart
    # before their first look is finished)
    again = 0
    for r in behind:
        whole = sum(b - a >= L for a, b in LS.segments(sum(submits), LS.restart_samples(submits, behind[r])))
        assert int(np.sum(per_row[r]["look"] == 0)) == whole, r
        at = int(np.nonzero(per_row[r]["look"] == 0)[0][-1])
        assert np.array_equal(per_row[r]["look"][at:], np.arange(len(per_row[r]) - at)), r
        again += whole == 2
    assert again == 5 and int(np.sum(per_row[1]["look"] == 0)) == 1
    # the listed rows and their neighbours: bit for bit a 1-row tracker's fed that row with the same restarts
    for r in LS.meter_listed(c):
        t1 = SondeTracker(1, RATE, max(submits), look_samples=L, lag=d)
        lone, _ = _meter_run(t1, rows[r:r + 1], submits, {0: behind.get(r, ())})
        assert _same_looks(per_row[r], lone), r
        t1.close()
    tr.close()


def test_meter_ring_beyond_the_first_launch():
    """1030 rows, 24 looks per row into a ring of 16, nothing read in between, three rows restarted at boundaries of their own"""
    c = LS.METER_RING
    n_rows, L, d, submits, behind = c["rows"], c["L"], c["lag"], c["submits"], c["behind"]
    n = sum(submits)
    x = LS.carriers(n_rows, n, c["seed"])
    rows = _dev(x)
    tr = SondeTracker(n_rows, RATE, c["max_samples"], look_samples=L, lag=d)
    assert tr.ring == 16
    looks, dropped = _meter_run(tr, rows, submits, behind)
    assert list(dropped) == [8] * n_rows and len(looks) == 16 * n_rows
    per_row = _by_row(looks, n_rows)
    one = SondeTracker(n_rows, RATE, n, look_samples=L, lag=d)
    ref, ref_dropped = _meter_run(one, rows, [n], {})
    assert not ref_dropped.any() and len(ref) == 24 * n_rows
    ref_row = _by_row(ref, n_rows)
    for r in range(n_rows):
        want = ref_row[r]
        if r in behind:                                     # the looks from the restart on: a single submit that begins there
            at = LS.restart_samples(submits, behind[r])[0]
            t1 = SondeTracker(1, RATE, n - at, look_samples=L, lag=d)
            after, _ = _meter_run(t1, rows[r:r + 1, at:], [n - at], {})
            t1.close()
            assert np.array_equal(after["look"], np.arange((n - at) // L))
            want = np.concatenate([want[:at // L], after])
        assert _same_looks(per_row[r], want[-16:]), r
    worst = 0.0
    for r in list(behind) + [0, 511, 512, 1028]:            # and within the bound of the reference, restarts and all
        idx, A, P, M, _ = LS.meter_expected(x[r], L, d, LS.restart_samples(submits, behind.get(r, ())))
        lk, bnd = per_row[r], TR.bound(M, L)[-16:]
        assert np.array_equal(lk["look"], idx[-16:])
        dev = np.stack([np.abs(lk["a_re"] - A.real[-16:]), np.abs(lk["a_im"] - A.imag[-16:]), np.abs(lk["p"] - P[-16:])], axis=1)
        assert np.all(dev <= bnd), (r, float(np.max(dev / bnd)))
        worst = max(worst, float(np.max(dev / bnd)))
    print(f"meter, ring: worst deviation / bound {worst:.3f}")
    looks, dropped = tr.results()
    assert len(looks) == 0 and not dropped.any()
    tr.close(); one.close()


@pytest.mark.parametrize("L,d", LS.METER_EDGES)
def test_meter_chunk_and_lag_edges(L, d):
    """3, 31, 32, 33 and 65 blocks per look at lags 1, 63 and 64: one submit against 256-sample submits, whose first `lag` partners
    all come from the carried history"""
    n = 2 * L + 256
    x = LS.carriers(LS.METER_EDGE_ROWS, n, LS.METER_EDGE_SEED)
    rows = _dev(x)
    t_one = SondeTracker(LS.METER_EDGE_ROWS, RATE, n, look_samples=L, lag=d)
    one, _ = _meter_run(t_one, rows, [n], {})
    t_cut = SondeTracker(LS.METER_EDGE_ROWS, RATE, 256, look_samples=L, lag=d)
    cut, dropped = _meter_run(t_cut, rows, [256] * (n // 256), {})
    assert len(one) == 2 * LS.METER_EDGE_ROWS and not dropped.any()
    assert one.tobytes() == cut.tobytes()
    worst = 0.0
    for r, lk in enumerate(_by_row(one, LS.METER_EDGE_ROWS)):
        worst = max(worst, _within_meter_bound(lk, x[r], L, d, (), r))
    print(f"meter, L {L} ({L // 256} blocks) lag {d}: worst deviation / bound {worst:.3f}")
    t_one.close(); t_cut.close()


# ---------------------------------------------------------------- combiner
def _cplx(v):
    return v[..., 0::2] + 1j * v[..., 1::2]


def _combine_run(comb, rows, submits, behind):
    """(output [S, n, 2] on the host, the read-outs [S, blocks] oldest first)"""
    S = comb.n_sondes
    ys, reads, a = [], [], 0
    for s, k in enumerate(submits):
        for i, bs in behind.items():
            if s in bs:
                comb.restart(i)
        y = comb.process(rows[:, a:a + k])
        rd = comb.readout()
        assert len(rd) == S * (k // comb.block) and np.array_equal(rd["sonde"].reshape(S, -1), np.repeat(np.arange(S)[:, None], k // comb.block, 1))
        reads.append(rd.reshape(S, -1))
        ys.append(y.cpu().numpy().copy())
        a += k
    assert a == rows.shape[1]
    return np.concatenate(ys, axis=1), np.concatenate(reads, axis=1)


def _check_combiner(x, S, K, L, y, rd, submits, behind):
    """every sonde: M, the weights' chain, the norm, the float32 weights, the output and the block counter; returns the worst
    deviation / bound of M and of the output"""
    n = x.shape[1]
    worst_m = worst_y = 0.0
    for i in range(S):
        xi = LS.sonde_rows(x, S, K, i)
        ri = rd[i]
        idx = np.concatenate([np.arange((b - a) // L) for a, b in LS.segments(n, LS.restart_samples(submits, behind.get(i, ())))])
        assert np.array_equal(ri["block"], idx), (i, ri["block"], idx)
        M, A = CR.stats_ref(xi, L)
        bnd = CR.bound(A, L)
        dev = np.abs(ri["m"] - M)
        used = A > 0
        assert np.all(dev <= bnd), (i, float(np.max(dev[used] / bnd[used])))
        assert np.all(ri["m"][~used] == 0.0)
        worst_m = max(worst_m, float(np.max(dev[used] / bnd[used])))
        W = _cplx(ri["w"])[:, :K]
        prev = None
        for b in range(len(ri)):
            want = cb.weights(ri["m"][b], None if idx[b] == 0 else prev, antennas=K)
            assert np.max(np.abs(W[b].real - want.real)) <= 1e-12 and np.max(np.abs(W[b].imag - want.imag)) <= 1e-12, (i, b, W[b], want)
            prev = W[b]
        assert np.all(np.abs(np.linalg.norm(W, axis=1) - 1.0) <= 1e-12)
        assert np.array_equal(ri["wf"], ri["w"].astype(np.float32)) and np.all(ri["w"][:, 2 * K:] == 0.0)
        wf = _cplx(ri["wf"].astype(np.float64))[:, :K]
        ref, T = CR.apply_ref(xi, wf, L)
        ab = CR.apply_bound(T, K)
        got = y[i].astype(np.float64)
        er, ei = np.abs(got[:, 0] - ref.real), np.abs(got[:, 1] - ref.imag)
        assert np.all(er <= ab[:, 0]) and np.all(ei <= ab[:, 1]), i
        nz = ab.min(axis=1) > 0
        worst_y = max(worst_y, float(np.max(er[nz] / ab[nz, 0])), float(np.max(ei[nz] / ab[nz, 1])))
        assert np.median(np.abs(ref)) > 1e4 * np.median(ab)
    return worst_m, worst_y


@pytest.mark.parametrize("S,K", LS.COMBINE_LAUNCHES["cases"])
def test_combiner_three_weights_launches(S, K):
    """1030 sondes (512 + 512 + 6) with two and four antennas, 513 (512 + 1) with three; blocks of 256, three submits, the sondes at
    the launch boundaries and at the edges of the restart words restarted behind one submit or the other"""
    c = LS.COMBINE_LAUNCHES
    L, submits, behind = c["L"], c["submits"], LS.combine_behind(S)
    x = LS.antenna_rows(S, K, sum(submits), c["seed"])
    rows = _dev(x)
    comb = SondeCombiner(S, K, RATE, max(submits), L)
    y, rd = _combine_run(comb, rows, submits, behind)
    worst_m, worst_y = _check_combiner(x, S, K, L, y, rd, submits, behind)
    print(f"combiner S {S} K {K}: worst M deviation / bound {worst_m:.3f}, worst output deviation / bound {worst_y:.3f}")
    for i in behind:                                        # bit for bit an S = 1 combiner's fed the sonde's rows with the same restarts
        lone = rows[[a * S + i for a in range(K)]].contiguous()
        c1 = SondeCombiner(1, K, RATE, max(submits), L)
        y1, r1 = _combine_run(c1, lone, submits, {0: behind[i]})
        assert y[i].tobytes() == y1[0].tobytes(), i
        for k in ("block", "m", "w", "wf"):
            assert rd[i][k].tobytes() == r1[0][k].tobytes(), (i, k)
        c1.close()
    comb.close()


@pytest.mark.parametrize("L", LS.COMBINE_EDGES["Ls"])
def test_combiner_summation_block_edges(L):
    """3, 32, 33 and 40 summation blocks per block: one submit against submits of one block"""
    e = LS.COMBINE_EDGES
    S, K, n = e["S"], e["K"], 2 * L
    x = LS.antenna_rows(S, K, n, e["seed"])
    rows = _dev(x)
    c_one, c_cut = SondeCombiner(S, K, RATE, n, L), SondeCombiner(S, K, RATE, L, L)
    y, rd = _combine_run(c_one, rows, [n], {})
    y2, rd2 = _combine_run(c_cut, rows, [L, L], {})
    assert y.tobytes() == y2.tobytes() and rd.tobytes() == rd2.tobytes()
    worst_m, worst_y = _check_combiner(x, S, K, L, y, rd, [n], {})
    print(f"combiner L {L} ({L // 256} summation blocks): worst M deviation / bound {worst_m:.3f}, worst output deviation / bound {worst_y:.3f}")
    c_one.close(); c_cut.close()


# ---------------------------------------------------------------- tuner
KINDS = {"complex64": (_lib.INPUT_IQ, torch.float32), "iq16": (_lib.INPUT_IQ16, torch.int16)}
HAND = 50                        # slots per tuner of the split a caller would make by hand: 0-49, 50-99, 100-149
_ref_rows = {}


def _ref_row(k):
    """(y, bound) of slot k from the float64 reference with the library's taps (the same for both input kinds: the samples are integers)"""
    if k not in _ref_rows:
        _ref_rows[k] = LS.tuner_row_ref(k, taps=lambda fs, r, b: tuner_taps(fs, r, b).astype(np.float64))
    return _ref_rows[k]


def _move(tu, before, now, slot_of, glide=()):
    """the slot calls that turn one submit's plan into the next: an idle slot is tuned with slot_set (theta = 0, as the plain retune),
    an active one retuned (the slots of `glide` continuously), one that left is cleared"""
    for k in sorted(set(before) | set(now)):
        if k not in now:
            tu.slot_clear(slot_of(k))
        elif k not in before:
            tu.slot_set(slot_of(k), *now[k])
        elif now[k] != before[k]:
            tu.retune(slot_of(k), now[k][0], continuous=k in glide)


@pytest.fixture(scope="module", params=list(KINDS))
def tuner_run(request):
    """the 150-slot tuner and three tuners of 50 slots over the same five submits: per submit (plan, rows [150, n_out, 2], the hand
    tuners' rows stacked [150, n_out, 2])"""
    cfg = LS.TUNER
    kind, dt = KINDS[request.param]
    fs, r, n_slots = cfg["fs"], cfg["r"], cfg["slots"]
    up, down = R.ratio(fs, r)
    xs = LS.tuner_stream()
    dev = torch.from_numpy(np.stack([xs.real, xs.imag], axis=1)).to(dt).to(DEV)
    subs, plan = LS.tuner_all_submits(), LS.tuner_plan()
    big = SondeTuner.slots(fs, r, n_slots, cfg["bws"], max(subs) * down, input_kind=kind)
    hands = [SondeTuner.slots(fs, r, HAND, cfg["bws"], max(subs) * down, input_kind=kind) for _ in range(n_slots // HAND)]
    out = torch.full((n_slots, 251, 2), float("nan"), device=DEV)          # rows an odd number of samples apart, longer than any submit's
    runs, a, before = [], 0, {}
    for s, units in enumerate(subs):
        glide = cfg["glided"] if s == 1 else ()
        _move(big, before, plan[s], lambda k: k, glide)
        for h, tu in enumerate(hands):
            lo = h * HAND
            _move(tu, {k: v for k, v in before.items() if lo <= k < lo + HAND}, {k: v for k, v in plan[s].items() if lo <= k < lo + HAND},
                  lambda k: k - lo, glide)
        before = plan[s]
        assert [big.slot_active(k) for k in range(n_slots)] == [k in plan[s] for k in range(n_slots)]
        if s == len(subs) - 1:
            out = torch.full((n_slots, 251, 2), float("nan"), device=DEV)  # (the last submit is shorter than the one before)
        blk = dev[a:a + units * down].contiguous()
        y = big.process(blk, out=out)
        assert y.shape == (n_slots, units * up, 2)
        assert bool(torch.isnan(out[:, units * up:]).all())                # nothing written beyond the rows
        got = y.cpu().numpy().copy()
        want = np.concatenate([tu.process(blk).cpu().numpy() for tu in hands], axis=0)
        runs.append((plan[s], got, want))
        a += units * down
    assert a == len(xs)
    big.close()
    for tu in hands:
        tu.close()
    return request.param, runs


def _check_tuner(name, runs, first, count):
    cfg = LS.TUNER
    up, _ = R.ratio(cfg["fs"], cfg["r"])
    j = np.concatenate([[0], np.cumsum(LS.tuner_all_submits())]) * up
    for s in range(first, first + count):
        plan, got, want = runs[s]
        assert not np.any(np.isnan(got))
        idle = [k for k in range(cfg["slots"]) if k not in plan]
        act = sorted(plan)
        assert not np.any(got[idle].view(np.uint32)), f"submit {s}: an idle row is not exactly zero"
        same = [got[k].tobytes() == want[k].tobytes() for k in act]
        assert all(same), (s, [k for k, ok in zip(act, same) if not ok])
        held, worst = 0, 0.0
        for k in cfg["ref_rows"]:
            if k not in plan:
                continue
            y, bnd = _ref_row(k)
            y, bnd = y[j[s]:j[s + 1]], bnd[j[s]:j[s + 1]]
            dr, di = np.abs(got[k, :, 0] - y.real), np.abs(got[k, :, 1] - y.imag)
            assert np.all(dr <= bnd) and np.all(di <= bnd), (s, k, float(np.max(np.maximum(dr, di) / bnd)))
            assert np.max(np.abs(y)) > 100.0 * np.max(bnd)
            worst = max(worst, float(np.max(np.maximum(dr, di) / bnd)))
            held += 1
        assert held >= (25 if len(act) > LS.TN_VMAX else 8)
        print(f"tuner {name}, submit {s} ({len(act)} active, {got.shape[1]} outputs): worst deviation / bound {worst:.3f} over {held} rows")


def test_tuner_three_mixing_launches_with_holes(tuner_run):
    """150 slots, 134 active in launches of 64 + 64 + 6 with sixteen holes between them; submits whose last tiles hold 42, 2, 62 and 48
    outputs; one slot of each launch retuned continuously between submits 1 and 2 (a phase offset that is not zero from there on); slot
    64 tuned, slot 129 retuned and slot 3 cleared between submits 2 and 3"""
    name, runs = tuner_run
    assert [len(p) for p, _, _ in runs[:4]] == [134] * 4 and [g.shape[1] for _, g, _ in runs[:4]] == [42, 66, 126, 240]
    _check_tuner(name, runs, 0, 4)


def test_tuner_two_fill_launches(tuner_run):
    """70 slots cleared: 64 active, exactly one full mixing launch that is sent at the last active slot, and 86 idle slots in two fill
    launches; one more submit"""
    name, runs = tuner_run
    plan, got, _ = runs[4]
    assert len(plan) == LS.TN_VMAX and LS.TUNER["slots"] - len(plan) == 86 and got.shape[1] == 78
    _check_tuner(name, runs, 4, 1)
