"""The scenes of tests/launch_edge_scenes.py on the CPU, from the references alone: what tests/test_gpu_launch_edges.py checks on the
GPU could not pass if a row's launch parameters were taken from the row 512 rows (64 slots) away, every edge of the launch plan and of
the summation loops is reached by a case, the bounds are far below the signal on every row, and the expected results do not depend
on how the stream is cut (the scenes' own restart bookkeeping)."""
from __future__ import annotations

import numpy as np
import pytest

import combine_reference as CR
import launch_edge_scenes as LS
import track_reference as TR
import tuner_reference as R


# ---------------------------------------------------------------- carrier meter
def test_meter_schedules_are_what_the_issue_lists():
    c = LS.METER_LAUNCHES
    assert c["rows"] == 2 * LS.VMAX + 6 and sorted(c["behind"]) == [0, 511, 512, 513, 1023, 1024, 1029]
    assert {b for bs in c["behind"].values() for b in bs} == {1, 2, 3, 4}              # every boundary is used
    assert all(n % LS.BLK == 0 for n in c["submits"]) and len(c["submits"]) == 5
    r = LS.METER_RING
    assert r["rows"] == 1030 and LS.meter_ring_len(r["max_samples"], r["L"]) == 16 and sorted(r["behind"]) == [5, 517, 1029]
    assert len({bs for bs in r["behind"].values()}) == 3                                # at different boundaries
    assert [L // LS.BLK for L, _ in LS.METER_EDGES] == [3, 31, 32, 33, 65]


@pytest.mark.parametrize("cfg", [LS.METER_LAUNCHES, LS.METER_RING], ids=["launches", "ring"])
def test_meter_row_aliasing_would_be_caught(cfg):
    """phase within the look, fresh flag and ring slot of a listed row differ from those of the rows 512 and 1024 away in at least one
    submit; and where only they differ, the looks differ: the expected looks of the row are not those of the partner's schedule"""
    prm = LS.meter_params(cfg, cfg.get("max_samples"))
    n = sum(cfg["submits"])
    x = LS.carriers(cfg["rows"], n, cfg["seed"])
    seen = set()
    for r in cfg["behind"]:
        partners = LS.alias_partners(r, cfg["rows"])
        assert partners
        for p in partners:
            differs = np.any(prm[:, r, :3] != prm[:, p, :3], axis=1)
            assert differs.any(), (r, p)
            seen.update(q for q in range(3) if np.any(prm[:, r, q] != prm[:, p, q]))
            # row r's samples under the partner's restarts give other looks than under its own, by far more than the bound
            mine = LS.meter_expected(x[r], cfg["L"], cfg["lag"], LS.restart_samples(cfg["submits"], cfg["behind"][r]))
            theirs = LS.meter_expected(x[r], cfg["L"], cfg["lag"], LS.restart_samples(cfg["submits"], cfg["behind"].get(p, ())))
            same_shape = len(mine[0]) == len(theirs[0]) and np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[4], theirs[4])
            if same_shape:
                bnd = TR.bound(mine[3], cfg["L"])
                assert np.any(np.abs(mine[1] - theirs[1]) > 100.0 * bnd[:, :2].max(axis=1)), (r, p)
    if cfg is LS.METER_LAUNCHES:
        assert seen == {0, 1, 2}                           # each of phase, fresh flag and ring slot tells some pair apart
    # no two rows are alike: every row's first look differs from every other row's
    first = np.array([TR.meter_ref(x[r, :cfg["L"]], cfg["L"], cfg["lag"])[0][0] for r in range(cfg["rows"])])
    assert len(np.unique(first)) == cfg["rows"]


def test_meter_restarts_show_in_the_results():
    """a restarted row's look counters start again at 0, and its restart drops a look in progress or its lag history: both are seen"""
    c = LS.METER_LAUNCHES
    prm = LS.meter_params(c)
    for r, bs in c["behind"].items():
        for b in bs:
            assert prm[b, r, 1] == 1 and prm[b, r, 3] == 0 and prm[b, r, 0] == 0
    assert prm[:, 1, 1].tolist() == [1, 0, 0, 0, 0]
    assert {int(prm[b, 1, 0]) for bs in c["behind"].values() for b in bs} == {0, 1}      # (row 1 never restarts) restarts inside a look and between looks


def test_meter_edge_classes():
    got = set()
    for L, d in LS.METER_EDGES:
        got |= LS.sum_classes(L // LS.BLK) | LS.lag_classes(d)
        assert (2 * L + 256) % LS.BLK == 0 and (2 * L + 256) // L == 2           # two looks finished, the third in the carry
    assert got >= {"fewer blocks than waves", "one block short of a trip", "exactly one trip", "a second trip", "a third trip",
                   "a last trip of one block", "lag 1", "lag one below the largest", "the largest lag"}
    assert LS.DMAX == 64 and all(d <= LS.DMAX for _, d in LS.METER_EDGES)
    # the launches: full, full, six rows; the ring: 24 looks into 16 slots
    assert -(-LS.METER_LAUNCHES["rows"] // LS.VMAX) == 3 and LS.METER_LAUNCHES["rows"] % LS.VMAX == 6
    r = LS.METER_RING
    assert sum(r["submits"]) // r["L"] == 24


def _meter_cases():
    c, r = LS.METER_LAUNCHES, LS.METER_RING
    yield "launches", LS.carriers(c["rows"], sum(c["submits"]), c["seed"]), c["L"], c["lag"], c
    yield "ring", LS.carriers(r["rows"], sum(r["submits"]), r["seed"]), r["L"], r["lag"], r
    for L, d in LS.METER_EDGES:
        yield f"edges {L} {d}", LS.carriers(LS.METER_EDGE_ROWS, 2 * L + 256, LS.METER_EDGE_SEED), L, d, None


def test_meter_bounds_are_not_vacuous():
    for name, x, L, d, cfg in _meter_cases():
        worst = np.inf
        for r in range(x.shape[0]):
            rs = LS.restart_samples(cfg["submits"], cfg["behind"].get(r, ())) if cfg else ()
            _, A, _, M, _ = LS.meter_expected(x[r], L, d, rs)
            bnd = TR.bound(M, L)
            assert len(A) and np.all(np.abs(A) > 1000.0 * bnd[:, :2].max(axis=1)), (name, r)
            worst = min(worst, float(np.min(np.abs(A) / bnd[:, :2].max(axis=1))))
        print(f"meter {name}: smallest |A| / bound {worst:.3g}")


def test_meter_reference_is_independent_of_the_cutting():
    c = LS.METER_LAUNCHES
    x = LS.carriers(c["rows"], sum(c["submits"]), c["seed"])
    for r in LS.meter_listed(c):
        rs = LS.restart_samples(c["submits"], c["behind"].get(r, ()))
        idx, A, P, _, _ = LS.meter_expected(x[r], c["L"], c["lag"], rs)
        for cuts in (c["submits"], (256,) * (sum(c["submits"]) // 256), (768, 256, 512, 1536)):
            if not set(rs) <= set(np.cumsum(cuts).tolist()):
                continue
            i2, A2, P2 = LS.meter_streamed(x[r], c["L"], c["lag"], cuts, rs)
            assert np.array_equal(idx, i2) and np.array_equal(A, A2) and np.array_equal(P, P2), (r, cuts)
    for L, d in LS.METER_EDGES[:2]:
        x = LS.carriers(LS.METER_EDGE_ROWS, 2 * L + 256, LS.METER_EDGE_SEED)
        idx, A, P, _, _ = LS.meter_expected(x[1], L, d)
        i2, A2, P2 = LS.meter_streamed(x[1], L, d, (256,) * (len(x[1]) // 256))
        assert len(idx) == 2 and np.array_equal(idx, i2) and np.array_equal(A, A2) and np.array_equal(P, P2)


# ---------------------------------------------------------------- combiner
def test_combiner_schedule_is_what_the_issue_lists():
    assert sorted(LS.COMBINE_BEHIND) == sorted(LS.COMBINE_LISTED)
    assert {b for bs in LS.COMBINE_BEHIND.values() for b in bs} == {1, 2}
    # i and i + 512 never restart behind the same boundary -- but for 1024: with two boundaries and three sondes (0, 512, 1024) at one
    # launch index, one of them has to restart behind both for the three to differ pairwise; its set still differs from the others'
    for i, bs in LS.COMBINE_BEHIND.items():
        for p in (i + LS.VMAX, i + 2 * LS.VMAX):
            other = LS.COMBINE_BEHIND.get(p, ())
            assert set(bs) != set(other), (i, p)
            assert not set(bs) & set(other) or 1024 in (i, p), (i, p)
    assert LS.COMBINE_LAUNCHES["cases"] == ((1030, 2), (1030, 4), (513, 3)) and LS.COMBINE_LAUNCHES["submits"] == (256, 512, 256)
    # the restart bits travel as 32-bit words: the last bit of a word and the first of the next, in the first launch and the second
    assert {i % 32 for i in (31, 543)} == {31} and {i % 32 for i in (32, 544)} == {0}


@pytest.mark.parametrize("S,K", LS.COMBINE_LAUNCHES["cases"])
def test_combiner_row_aliasing_would_be_caught(S, K):
    """the restart bit of a listed sonde differs from that of the sondes 512 and 1024 away in at least one submit, and there the
    weights with and without previous weights differ by far more than the 1e-12 the weights are held to"""
    c = LS.COMBINE_LAUNCHES
    behind = LS.combine_behind(S)
    prm = LS.combine_params(S, c["submits"], behind)
    n = sum(c["submits"])
    x = LS.antenna_rows(S, K, n, c["seed"])
    at = [0] + LS.boundaries(c["submits"])
    for i in behind:
        partners = LS.alias_partners(i, S)
        assert partners or S < 2 * LS.VMAX                # (S = 513: sonde 512 alone has a launch of its own, 0 is its partner)
        xi = LS.sonde_rows(x, S, K, i)
        M, _ = CR.stats_ref(xi, c["L"])
        _, W, _, _ = LS.combine_expected(xi, c["L"])                                 # never restarted
        for p in partners:
            subs = np.nonzero(prm[:, i, 0] != prm[:, p, 0])[0]
            assert len(subs), (i, p)
            for s in subs:
                b = at[s] // c["L"]                                                   # the submit's first block
                fresh = CR.weights_ref(K, M[b], None)
                chained = CR.weights_ref(K, M[b], W[b - 1])
                assert np.max(np.abs(fresh - chained)) > 1e-6, (i, p, s)
    # the block counters restart with the sonde
    for i, bs in behind.items():
        for b in bs:
            assert prm[b, i, 1] == 0 and prm[b, 1, 1] > 0
    # no two sondes are alike
    first = np.array([CR.stats_ref(LS.sonde_rows(x, S, K, i)[:, :c["L"]], c["L"])[0][0, 4] for i in range(S)])
    assert len(np.unique(first)) == S


def test_combiner_edge_classes():
    e = LS.COMBINE_EDGES
    assert [L // LS.BLK for L in e["Ls"]] == [3, 32, 33, 40]
    got = set()
    for L in e["Ls"]:
        got |= LS.sum_classes(L // LS.BLK)
    assert got >= {"fewer blocks than waves", "exactly one trip", "a second trip", "a last trip of one block", "a last trip of whole strides"}
    for S, _ in LS.COMBINE_LAUNCHES["cases"]:
        assert -(-S // LS.VMAX) in (2, 3)
    assert {-(-S // LS.VMAX) for S, _ in LS.COMBINE_LAUNCHES["cases"]} == {2, 3}
    assert {S % LS.VMAX for S, _ in LS.COMBINE_LAUNCHES["cases"]} == {1, 6}          # a last launch of one sonde, and of six


def _combine_cases():
    c, e = LS.COMBINE_LAUNCHES, LS.COMBINE_EDGES
    for S, K in c["cases"]:
        yield S, K, c["L"], LS.antenna_rows(S, K, sum(c["submits"]), c["seed"]), LS.combine_behind(S), c["submits"]
    for L in e["Ls"]:
        yield e["S"], e["K"], L, LS.antenna_rows(e["S"], e["K"], 2 * L, e["seed"]), {}, (2 * L,)


def test_combiner_bounds_are_not_vacuous():
    for S, K, L, x, behind, submits in _combine_cases():
        cross, out = np.inf, []
        for i in range(S):
            xi = LS.sonde_rows(x, S, K, i)
            y, W, M, _ = LS.combine_expected(xi, L, LS.restart_samples(submits, behind.get(i, ())))
            _, A = CR.stats_ref(xi, L)
            bnd = CR.bound(A, L)
            c = np.hypot(M[:, 4], M[:, 5]) / np.maximum(bnd[:, 4], bnd[:, 5])
            assert np.all(c > 1000.0), (S, K, L, i)
            cross = min(cross, float(c.min()))
            wf = W.real.astype(np.float32).astype(np.float64) + 1j * W.imag.astype(np.float32).astype(np.float64)
            ref, T = CR.apply_ref(xi, wf, L)
            ab = CR.apply_bound(T, K)
            assert np.median(np.abs(ref)) > 1e4 * np.median(ab), (S, K, L, i)
            out.append(float(np.median(np.abs(ref)) / np.median(ab)))
            assert np.array_equal(ref, y)
        print(f"combiner S {S} K {K} L {L}: smallest cross term / bound {cross:.3g}, smallest median |y| / median bound {min(out):.3g}")


def test_combiner_reference_is_independent_of_the_cutting():
    c = LS.COMBINE_LAUNCHES
    S, K = 1030, 4
    x = LS.antenna_rows(S, K, sum(c["submits"]), c["seed"])
    for i in LS.COMBINE_LISTED:
        xi = LS.sonde_rows(x, S, K, i)
        rs = LS.restart_samples(c["submits"], LS.COMBINE_BEHIND[i])
        one = LS.combine_expected(xi, c["L"], rs)
        for cuts in (c["submits"], (256,) * 4):
            got = LS.combine_expected(xi, c["L"], rs, cuts)
            for a, b in zip(one, got):
                assert np.array_equal(a, b), (i, cuts)
        assert one[3][len(one[3]) - 1] < 4 - 1                                     # the counter began again somewhere


# ---------------------------------------------------------------- tuner
def test_tuner_schedule_is_what_the_issue_lists():
    cfg = LS.TUNER
    up, down = R.ratio(cfg["fs"], cfg["r"])
    assert (up, down) == (6, 125) and cfg["slots"] == 150
    plan = LS.tuner_plan()
    assert {5, 64, 70, 100} <= set(cfg["idle"]) and len(cfg["idle"]) == 16 and len(plan[0]) == 134
    offs = [LS.tuner_offset(k) for k in range(cfg["slots"])] + list(cfg["retuned"].values())
    assert len(set(offs)) == len(offs) and all(2 * abs(f) + max(cfg["bws"]) <= cfg["fs"] for f in offs)
    assert [LS.tuner_bw(k) for k in range(6)] == list(cfg["bws"]) * 2               # the tap sets cycle over the slots
    assert [s * up for s in cfg["submits"]] == [42, 66, 126, 240]
    assert [(s * up - 1) % LS.TN_JT + 1 for s in cfg["submits"]] == [42, 2, 62, 48]
    # three mixing launches, and no active slot at the launch index that equals its number once a hole lies in front of it
    for p in plan[:4]:
        launches = LS.tuner_launches(sorted(p))
        assert [len(v) for v in launches] == [64, 64, 6]
        hole = min(cfg["idle"])
        for v in launches:
            assert all(k != i for i, k in enumerate(v) if k > hole)
    assert set(plan[2]) == (set(plan[1]) | {64}) - {3} and plan[2][129] != plan[1][129] and plan[2][128] == plan[1][128]
    # the last submit: one full mixing launch, whose last entry is the last active slot, and two fill launches
    assert len(plan[4]) == LS.TN_VMAX and max(plan[4]) == max(plan[3]) and set(plan[4]) <= set(plan[3])
    idle = cfg["slots"] - len(plan[4])
    assert idle == 86 and -(-idle // LS.TN_VMAX) == 2
    assert len(plan[3]) - len(plan[4]) == 70
    # the rows held to the float64 reference are active somewhere, cover every launch, and enough of them stay for the last submit
    must = {0, 63, 65, 66, 127, 128, 129, 130, 149}
    assert must <= set(cfg["ref_rows"]) and len(set(cfg["ref_rows"]) - must) >= 16 and len(set(cfg["ref_rows"])) == len(cfg["ref_rows"])
    for p in plan[:4]:
        for v in LS.tuner_launches(sorted(p)):
            assert len(set(v) & set(cfg["ref_rows"])) >= 4 and {v[0], v[-1]} <= set(cfg["ref_rows"])
    assert len(set(plan[4]) & set(cfg["ref_rows"])) >= 8


def test_tuner_edge_classes():
    cfg = LS.TUNER
    up, _ = R.ratio(cfg["fs"], cfg["r"])
    got = set()
    for s in LS.tuner_all_submits():
        got |= LS.tuner_tile_classes(s * up)
    assert got == {"fewer outputs than waves", "a last stride in part", "whole strides short of a tile", "one tile in part", "several tiles"}


@pytest.fixture(scope="module")
def tuner_rows():
    """every slot's reference row and bound over the five submits (None for a slot that is never active)"""
    return [LS.tuner_row_ref(k) for k in range(LS.TUNER["slots"])]


def test_tuner_rows_carry_signal_and_slot_aliasing_would_be_caught(tuner_rows):
    """per submit: every active row lies more than 100 bounds above zero, and differs by more than 100 bounds from the rows of the
    slots 64 and 128 slots away and of the slots 64 and 128 places away in the list of active slots (what shares its launch index)"""
    cfg = LS.TUNER
    up, _ = R.ratio(cfg["fs"], cfg["r"])
    j = np.concatenate([[0], np.cumsum(LS.tuner_all_submits())]) * up
    worst_sig = worst_alias = np.inf
    for s, p in enumerate(LS.tuner_plan()):
        act = sorted(p)
        sl = slice(int(j[s]), int(j[s + 1]))
        for i, k in enumerate(act):
            y, bnd = tuner_rows[k]
            assert not np.any(np.isnan(y[sl]))
            sig = float(np.max(np.abs(y[sl])) / np.max(bnd[sl]))
            assert sig > 100.0, (s, k, sig)
            worst_sig = min(worst_sig, sig)
            partners = {q for q in LS.alias_partners(k, cfg["slots"], LS.TN_VMAX) if q in p}
            partners |= {act[q] for q in LS.alias_partners(i, len(act), LS.TN_VMAX)}
            assert partners or s == 4, (s, k)                  # (the last submit is one launch: nothing shares a launch index)
            for q in partners:
                yq, bq = tuner_rows[q]
                diff = np.abs(y[sl] - yq[sl])
                sep = float(np.max(np.maximum(np.abs(diff.real), np.abs(diff.imag))) / max(np.max(bnd[sl]), np.max(bq[sl])))
                assert sep > 100.0, (s, k, q, sep)
                worst_alias = min(worst_alias, sep)
    print(f"tuner: smallest max |y| / max bound {worst_sig:.3g}, smallest separation of rows a launch apart / bound {worst_alias:.3g}")
    # a phase offset taken from another slot is seen: each launch holds a slot whose theta is not zero from submit 1 on, and with theta
    # left at zero its rows differ by more than 100 bounds
    glided = sorted(cfg["glided"])
    assert [next(n for n, v in enumerate(LS.tuner_launches(sorted(LS.tuner_plan()[1]))) if k in v) for k in glided] == [0, 1, 2]
    assert len({LS.tuner_theta(k, 1) for k in glided} | {0}) == 4 and all(LS.tuner_theta(k, 0) == 0 for k in glided)
    for k in glided:
        y, bnd = tuner_rows[k]
        y0, _ = LS.tuner_row_ref(k, no_theta=True)
        assert np.array_equal(y0[:int(j[1])], y[:int(j[1])])
        for s in range(1, 5):
            if k in LS.tuner_plan()[s]:
                sl = slice(int(j[s]), int(j[s + 1]))
                assert np.max(np.abs(y0[sl] - y[sl])) > 100.0 * np.max(bnd[sl]), (k, s)
    # a retune is seen: the retuned rows differ from the rows at the old offset by more than 100 bounds
    for k in (129,):
        y, bnd = tuner_rows[k]
        g = R.taps64(cfg["fs"], cfg["r"], LS.tuner_bw(k))
        _, down = R.ratio(cfg["fs"], cfg["r"])
        old, _ = R.tuner_ref(LS.tuner_stream(), cfg["fs"], cfg["r"], g, [LS.tuner_offset(k)] * 5, [s * down for s in LS.tuner_all_submits()])
        sl = slice(int(j[2]), int(j[5]))
        assert np.array_equal(old[:int(j[2])], y[:int(j[2])]) and np.max(np.abs(old[sl] - y[sl])) > 100.0 * np.max(bnd[sl])


def test_tuner_reference_is_independent_of_the_cutting(tuner_rows):
    """a slot that is never retuned, over the same stream in other submits: the same outputs (the filter's window reaches back over the
    boundaries, the mixer runs on the absolute index)"""
    total = sum(LS.tuner_all_submits())
    for k in (0, 149):
        y, bnd = tuner_rows[k]
        assert not np.any(np.isnan(y))
        for subs in ((total,), (1,) * 10 + (total - 10,)):
            y2, _ = LS.tuner_row_ref(k, submits=subs)
            assert len(y2) == len(y) and np.max(np.abs(y2 - y)) <= 1e-9 * np.max(np.abs(y)), (k, subs)
