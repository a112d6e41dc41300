"""Scenes and schedules for the tests of the tuner, the carrier meter and the combiner beyond one launch of rows (DESIGN SPEC 3.9, 3.11,
3.14): plain numpy plus the reference modules; it imports neither torch nor the product.

The three objects pass per-row parameters to their kernels by value, a fixed number of rows per launch (512 meter rows, 512 combiner
sondes, 64 active tuner slots), and sum in trips of 32 blocks through LDS with 4 waves striding over the blocks.  Here are

    rows of a carrier each   every row its own frequency, amplitude and noise (float32 values, so the references see what the kernels see)
    the schedules            which row restarts behind which submit, which slot is idle, retuned or cleared where
    the launch parameters    what travels by value per row and submit, worked out from the schedule alone (no product code)
    the expected results     the references applied segment by segment between a row's restarts
    the edge classes         which boundary of the launch plan a case reaches

tests/test_launch_edges_reference.py (CPU) asserts on these that the GPU tests of tests/test_gpu_launch_edges.py cannot pass
vacuously; both read the same data."""
from __future__ import annotations

import functools

import numpy as np

import combine_reference as CR
import track_reference as TR
import tuner_reference as R

RATE = 48_000
BLK = 256                        # samples per summation block, meter and combiner
VMAX = 512                       # meter rows / combiner sondes per launch
CHUNK = 32                       # summation blocks per trip through LDS
WAVES = 4
DMAX = 64                        # the meter's largest lag


def _f32(x: np.ndarray) -> np.ndarray:
    """what a float32 row holds of x, as complex128"""
    return x.real.astype(np.float32).astype(np.float64) + 1j * x.imag.astype(np.float32).astype(np.float64)


def as_iq(x: np.ndarray) -> np.ndarray:
    """complex [.., n] -> float32 [.., n, 2]"""
    return np.stack([x.real, x.imag], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def carriers(n_rows: int, n: int, seed: int) -> np.ndarray:
    """[n_rows, n] complex128 of float32 values: row r a carrier at -9000 + 17.3 r Hz (mod the rate's half), amplitude 0.6 .. 1.4, under
    noise of its own at 0.1 per component.  No two rows are alike."""
    rng = np.random.default_rng(seed)
    r = np.arange(n_rows)[:, None]
    f = (-9000.0 + 17.3 * r) % 18_000.0 - 9000.0
    amp = 0.6 + 0.1 * (r % 9)
    t = np.arange(n)[None, :]
    x = amp * np.exp(2j * np.pi * (f * t / RATE + rng.uniform(size=(n_rows, 1))))
    x = x + 0.1 * (rng.standard_normal((n_rows, n)) + 1j * rng.standard_normal((n_rows, n)))
    x = _f32(x)
    x.setflags(write=False)
    return x


def boundaries(submits) -> list[int]:
    """boundary b (1 ..) lies behind submit b: the sample index at which it lies"""
    return [int(v) for v in np.cumsum(submits)[:-1]]


def restart_samples(submits, behind) -> list[int]:
    """the sample indices of a row's restarts, for the boundaries it restarts behind"""
    at = boundaries(submits)
    return [at[b - 1] for b in behind]


def segments(n: int, restarts) -> list[tuple[int, int]]:
    """[0, n) cut at the restarts: each piece is a stream that began there"""
    cuts = [0] + sorted(restarts) + [n]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def alias_partners(r: int, n_rows: int, step: int = VMAX) -> list[int]:
    """the rows whose by-value parameters sit at the same launch index as row r's: r +- step, r +- 2 step"""
    return [p for p in (r - 2 * step, r - step, r + step, r + 2 * step) if 0 <= p < n_rows]


# ---------------------------------------------------------------- carrier meter
# three launches (512 + 512 + 6 rows).  behind: row -> the boundaries it restarts behind.  Rows r and r +- 512, r +- 1024 never restart
# behind the same boundary; boundaries 1 and 4 fall inside a look (the phase of the restarted row then differs too), 2 and 3 between looks.
METER_LAUNCHES = dict(rows=1030, L=512, lag=3, submits=(256, 768, 512, 256, 1280), seed=11,
                      behind={0: (1,), 513: (1,), 511: (2,), 512: (3,), 1023: (4,), 1024: (4,), 1029: (4,)})
# the ring (16 looks) beyond the first launch: six submits of four looks each, nothing read in between
METER_RING = dict(rows=1030, L=256, lag=2, max_samples=1024, submits=(1024,) * 6, seed=12, behind={5: (1,), 517: (3,), 1029: (5,)})
# (look_samples, lag): 3, 31, 32, 33 and 65 blocks per look; n = 2 L + 256, so the last look stays in the carry
METER_EDGES = [(768, 64), (7936, 1), (8192, 63), (8448, 64), (16640, 2)]
METER_EDGE_ROWS, METER_EDGE_SEED = 3, 13


def meter_listed(cfg) -> list[int]:
    """the restarted rows and their direct neighbours"""
    out = set()
    for r in cfg["behind"]:
        out.update(p for p in (r - 1, r, r + 1) if 0 <= p < cfg["rows"])
    return sorted(out)


def meter_ring_len(max_samples: int, L: int) -> int:
    """SPEC 3.11: a row keeps its newest max(16, max_samples / L + 2) looks"""
    return max(16, max_samples // L + 2)


def meter_params(cfg, max_samples: int | None = None) -> np.ndarray:
    """[submits, rows, 4] int: what travels by value for each row at each submit, from the schedule alone: blocks into the row's
    current look, the fresh flag, the ring slot of its next look (looks finished since create mod ring), and the look counter its
    next look gets (host state, not by value: the tests read it back)"""
    n_rows, LB = cfg["rows"], cfg["L"] // BLK
    ring = meter_ring_len(max_samples or max(cfg["submits"]), cfg["L"])
    ph, fresh, seq, look = np.zeros(n_rows, int), np.ones(n_rows, int), np.zeros(n_rows, int), np.zeros(n_rows, int)
    out = np.zeros((len(cfg["submits"]), n_rows, 4), int)
    for s, n in enumerate(cfg["submits"]):
        for r, bs in cfg["behind"].items():
            if s in bs:                                     # boundary s lies behind submit s, in front of submit s + 1 (index s)
                ph[r], fresh[r], look[r] = 0, 1, 0
        out[s] = np.stack([ph, fresh, seq % ring, look], axis=1)
        fin = (ph + n // BLK) // LB
        seq, look, ph = seq + fin, look + fin, (ph + n // BLK) % LB
        fresh[:] = 0
    return out


def meter_expected(x: np.ndarray, L: int, d: int, restarts=()):
    """every look of one row x (complex, from create) that restarts at the sample indices `restarts`, oldest first:
    (look index [K], A [K], P [K], M [K, 3], first sample of the look [K]); an unfinished look in front of a restart is dropped"""
    idx, A, P, M, at = [], [], [], [], []
    for a, b in segments(len(x), restarts):
        sa, sp, sm = TR.meter_ref(x[a:b], L, d)
        idx.append(np.arange(len(sa)))
        A.append(sa); P.append(sp); M.append(sm.reshape(-1, 3))
        at.append(a + L * np.arange(len(sa)))
    return np.concatenate(idx), np.concatenate(A), np.concatenate(P), np.concatenate(M), np.concatenate(at)


def meter_streamed(x: np.ndarray, L: int, d: int, cuts, restarts=()):
    """the same looks from the reference's streaming form fed in pieces of `cuts` samples, restarted where a piece begins at a
    restart: (look index, A, P).  The restarts must lie on cut boundaries."""
    me = TR.Meter(RATE, L, d)
    out, a = [], 0
    for k in cuts:
        if a in restarts:
            out += me.looks()
            me.restart()
        me.feed(x[a:a + k])
        a += k
    out += me.looks()
    assert a == len(x)
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]))


def sum_classes(blocks: int) -> set[str]:
    """the edges of the summation loop (4 waves stride over the blocks of a trip, 32 blocks per trip through LDS) a look or block of
    this many 256-sample blocks reaches"""
    out = set()
    if 1 < blocks < WAVES:
        out.add("fewer blocks than waves")
    trips, last = -(-blocks // CHUNK), (blocks - 1) % CHUNK + 1
    if trips == 1 and last == CHUNK - 1:
        out.add("one block short of a trip")
    if blocks == CHUNK:
        out.add("exactly one trip")
    if trips == 2:
        out.add("a second trip")
    if trips >= 3:
        out.add("a third trip")
    if trips >= 2 and last == 1:
        out.add("a last trip of one block")
    if trips >= 2 and last % WAVES == 0 and last < CHUNK:
        out.add("a last trip of whole strides")
    return out


def lag_classes(d: int) -> set[str]:
    out = set()
    if d == 1:
        out.add("lag 1")
    if d == DMAX - 1:
        out.add("lag one below the largest")
    if d == DMAX:
        out.add("the largest lag")
    return out


# ---------------------------------------------------------------- combiner
COMBINE_LISTED = (0, 31, 32, 511, 512, 513, 543, 544, 1023, 1024, 1029)
# sonde -> the boundaries it restarts behind (two boundaries: behind submits 1 and 2).  i and i + 512 never restart behind the same
# boundary; of 0, 512 and 1024 the last restarts behind both, so that all three differ in a submit
COMBINE_BEHIND = {0: (1,), 512: (2,), 1024: (1, 2), 31: (1,), 543: (2,), 32: (2,), 544: (1,), 511: (1,), 1023: (2,), 513: (2,), 1029: (1,)}
COMBINE_LAUNCHES = dict(L=256, submits=(256, 512, 256), cases=((1030, 2), (1030, 4), (513, 3)), seed=21)
# summation blocks per block: 3, 32, 33, 40; n = 2 L
COMBINE_EDGES = dict(S=2, K=3, Ls=(768, 8192, 8448, 10240), seed=22)


def combine_behind(S: int) -> dict:
    return {i: b for i, b in COMBINE_BEHIND.items() if i < S}


@functools.lru_cache(maxsize=None)
def antenna_rows(S: int, K: int, n: int, seed: int) -> np.ndarray:
    """[K * S, n] complex128 of float32 values: row a * S + i = sonde i's carrier (carriers()) through antenna a's gain, which is the
    antenna's and the sonde's own (amplitude 0.5 .. 1, a phase of its own that turns by 20 (a + 1) + i mod 7 Hz: paths that move), under
    noise of its own at 0.05 per component"""
    rng = np.random.default_rng(seed)
    s = carriers(S, n, seed + 1000)
    t = np.arange(n)[None, :]
    i = np.arange(S)[:, None]
    rows = []
    for a in range(K):
        g = rng.uniform(0.5, 1.0, size=(S, 1)) * np.exp(2j * np.pi * (rng.uniform(size=(S, 1)) + (20.0 * (a + 1) + i % 7) * t / RATE))
        rows.append(g * s + 0.05 * (rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))))
    x = _f32(np.concatenate(rows, axis=0))
    x.setflags(write=False)
    return x


def sonde_rows(x: np.ndarray, S: int, K: int, i: int) -> np.ndarray:
    """sonde i's K rows [K, n]"""
    return x[[a * S + i for a in range(K)]]


def combine_params(S: int, submits, behind) -> np.ndarray:
    """[submits, S, 2] int: the restart bit that travels by value for each sonde at each submit, and the block counter its first
    block of the submit gets (host state)"""
    L = COMBINE_LAUNCHES["L"]
    fresh, block = np.ones(S, int), np.zeros(S, int)
    out = np.zeros((len(submits), S, 2), int)
    for s, n in enumerate(submits):
        for i, bs in behind.items():
            if s in bs:
                fresh[i], block[i] = 1, 0
        out[s] = np.stack([fresh, block], axis=1)
        block = block + n // L
        fresh[:] = 0
    return out


def combine_expected(x: np.ndarray, L: int, restarts=(), cuts=None):
    """one sonde's stream x [K, n] that restarts at the sample indices `restarts`: (y [n], W [blocks, K], M [blocks, 16], block index
    [blocks]) from combine_reference.combine_ref, segment by segment.  cuts: feed each segment in pieces of these lengths instead,
    the weights carried from piece to piece (the restarts must lie on cut boundaries)."""
    n = x.shape[1]
    ys, Ws, Ms, idx = [], [], [], []
    edges = {0, n} | set(restarts) if cuts is None else set(np.cumsum([0] + list(cuts)).tolist())
    for a, b in segments(n, restarts):
        assert a in edges and b in edges
        inner = sorted(e for e in edges if a <= e <= b)
        w_prev, k = None, 0
        for p, q in zip(inner[:-1], inner[1:]):
            y, W, M = CR.combine_ref(x[:, p:q], L, w_prev=w_prev)
            ys.append(y); Ws.append(W); Ms.append(M)
            idx.append(k + np.arange(len(M)))
            k += len(M)
            if len(W):
                w_prev = W[-1]
    return np.concatenate(ys), np.concatenate(Ws), np.concatenate(Ms), np.concatenate(idx)


# ---------------------------------------------------------------- tuner
TN_VMAX, TN_JT = 64, 64
TUNER = dict(fs=1_000_000, r=48_000, bws=(10_000, 20_000, 48_000), slots=150, submits=(7, 11, 21, 40), seed=31,
             idle=(5, 17, 33, 47, 58, 64, 70, 81, 93, 100, 111, 118, 125, 133, 140, 147),
             # between submits 2 and 3 (in front of submit index 2): slot -> new offset (theta = 0: "as if tuned there since create"), and the slot
             # cleared.  Slot 64 is idle until then (an idle slot is tuned with slot_set, which follows the plain retune's rule), 129 is active
             retuned={64: -123_456, 129: 377_001}, cleared=(3,),
             # between submits 1 and 2 (in front of submit index 1), one slot of each launch moves by a few hundred Hz with the mixer's phase
             # kept (SPEC 3.9 "continuous retune"): from there on its phase offset theta is not zero.  slot -> the step in Hz
             glided={7: 333, 80: -271, 146: 199},
             # rows held to the float64 reference: the launches' first and last rows, the retuned ones, and others spread over the launches
             ref_rows=(0, 63, 65, 66, 127, 128, 129, 130, 149, 4, 6, 7, 16, 18, 32, 46, 59, 64, 69, 71, 80, 94, 101, 110, 119, 126, 141, 142, 143, 146, 148),
             # two fill launches: 64 slots stay active, 86 are idle; one more submit
             last_submit=13)


def tuner_offset(k: int) -> int:
    """slot k's offset: distinct, off every raster, |f| + 24 000 <= 500 000"""
    return -470_000 + 6301 * k


def tuner_bw(k: int) -> int:
    return TUNER["bws"][k % 3]


def tuner_plan():
    """per submit (the four, then the one behind the clearing): {slot: (offset, bandwidth)} of the active slots"""
    cfg = TUNER
    act = {k: (tuner_offset(k), tuner_bw(k)) for k in range(cfg["slots"]) if k not in cfg["idle"]}
    plan = [dict(act)]
    for k, df in cfg["glided"].items():
        act[k] = (tuner_offset(k) + df, tuner_bw(k))
    plan.append(dict(act))
    for k, f in cfg["retuned"].items():
        act[k] = (f, tuner_bw(k))
    for k in cfg["cleared"]:
        del act[k]
    plan += [dict(act), dict(act)]
    keep = tuner_kept(sorted(act))
    plan.append({k: v for k, v in act.items() if k in keep})
    return plan


def tuner_theta(k: int, s: int) -> int:
    """slot k's mixer phase offset in submit s: SPEC 3.9's theta' = (theta + (f_old - f_new) (n0 - T / 2)) mod Fs at the continuous
    retune in front of submit 1, 0 before it and for every other slot"""
    cfg = TUNER
    if k not in cfg["glided"] or s == 0:
        return 0
    _, down = R.ratio(cfg["fs"], cfg["r"])
    n0 = cfg["submits"][0] * down
    T = R.taps_per_phase(cfg["fs"], tuner_bw(k))
    return ((-cfg["glided"][k]) % cfg["fs"]) * ((n0 - T // 2) % cfg["fs"]) % cfg["fs"]


def tuner_kept(active: list[int]) -> set[int]:
    """the 64 slots that stay active for the last submit: the first and the last, and every second one in between"""
    inner = active[1:-1][1::2]
    return set([active[0], active[-1]] + inner[:TN_VMAX - 2])


def tuner_all_submits() -> list[int]:
    return list(TUNER["submits"]) + [TUNER["last_submit"]]


def tuner_launches(active: list[int]) -> list[list[int]]:
    """the active slots, ascending, 64 per launch"""
    return [active[a:a + TN_VMAX] for a in range(0, len(active), TN_VMAX)]


@functools.lru_cache(maxsize=None)
def tuner_stream():
    """the wideband stream [n] complex128 of integer values (exact as float32 and as 16-bit IQ): noise at 900 per component and two tones"""
    cfg = TUNER
    _, down = R.ratio(cfg["fs"], cfg["r"])
    n = sum(tuner_all_submits()) * down
    rng = np.random.default_rng(cfg["seed"])
    t = np.arange(n)
    x = 900.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for amp, f in ((0.3, 31_234), (0.2, -234_000)):
        x = x + 3000.0 * amp * np.exp(2j * np.pi * (f * t / cfg["fs"] + rng.uniform()))
    x = np.round(x)
    x.setflags(write=False)
    return x


def tuner_row_ref(k: int, taps=None, submits=None, no_theta=False):
    """slot k over the whole stream: (y, bound) per output, its retune given to the reference as per-submit offsets; None where the
    slot is idle in every submit.  Outputs of submits in which the slot is idle are NaN.  taps(fs, r, b) -> [up, T] float64 (default:
    the reference's own).  submits: another cutting of the same stream (in units of `down`), for a slot that is active throughout and never retuned.  no_theta: the
    phase offsets left at zero (what a slot's row would be with another slot's theta)."""
    cfg = TUNER
    _, down = R.ratio(cfg["fs"], cfg["r"])
    plan = tuner_plan()
    own = tuner_all_submits()
    if not any(k in p for p in plan):
        return None
    bw = tuner_bw(k)
    g = (taps or R.taps64)(cfg["fs"], cfg["r"], bw)
    last = next(p[k][0] for p in reversed(plan) if k in p)
    if submits is None:
        subs = own
        offs = [p[k][0] if k in p else last for p in plan]
    else:
        subs = list(submits)
        assert all(k in p and p[k][0] == last for p in plan) and sum(subs) == sum(own)
        offs = [last] * len(subs)
    thetas = None if submits is not None or no_theta else [tuner_theta(k, s) for s in range(len(subs))]
    y, A = R.tuner_ref(tuner_stream(), cfg["fs"], cfg["r"], g, offs, [s * down for s in subs], thetas=thetas)
    bnd = R.bound(A, g.shape[1])
    if submits is None:
        up, _ = R.ratio(cfg["fs"], cfg["r"])
        j = np.concatenate([[0], np.cumsum(own)]) * up
        y = y.copy()
        for s, p in enumerate(plan):
            if k not in p:
                y[j[s]:j[s + 1]] = np.nan
    return y, bnd


def tuner_tile_classes(n_out: int) -> set[str]:
    """what a submit of n_out outputs reaches in the last tile of 64 outputs (4 waves, 16 outputs each, the clamp min(wave + 4 r, nj - 1))"""
    nj = (n_out - 1) % TN_JT + 1
    out = set()
    if nj < WAVES:
        out.add("fewer outputs than waves")
    if nj < TN_JT and nj % WAVES:
        out.add("a last stride in part")
    if nj < TN_JT and nj % WAVES == 0:
        out.add("whole strides short of a tile")
    if n_out < TN_JT:
        out.add("one tile in part")
    if n_out > TN_JT:
        out.add("several tiles")
    return out
