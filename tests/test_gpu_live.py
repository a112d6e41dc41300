"""The live receiver on the GPU (DESIGN SPEC 3.12): tuner slots against a tuner that held the VFO since create and against
tests/tuner_reference.py, the slot refusals, the restart of single batch channels and detector channels against fresh objects fed
only the later submits, then one scene in which sondes appear and vanish through LiveReceiver against WidebandReceiver(track=True)
with outside knowledge.  Measured figures: profiles/live_notes.md."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import tuner_reference as R
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import VFO_RATE, SondeBatch, SondeChannelizer, SondeError
from sdrpp_radiosonde_amd.detect import SondeDetector
from sdrpp_radiosonde_amd.tuner import SondeTuner, WidebandReceiver, tuner_taps
from test_track_reference import DRIFT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IQ = _lib.INPUT_IQ
FS = 1_000_000


def _stream(fs, n, seed, tones=((0.3, 31_234), (0.2, -234_000))):
    """integer-valued complex samples: noise plus tones (the stream of tests/test_gpu_tuner.py)"""
    rng = np.random.default_rng(seed)
    a = 3000.0
    t = np.arange(n)
    x = a * 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for amp, f in tones:
        x = x + a * amp * np.exp(2j * np.pi * (f * t / fs + rng.uniform()))
    x = np.round(x)
    return x, torch.from_numpy(np.stack([x.real, x.imag], axis=1)).to(torch.float32).to(DEV)


# ---------------------------------------------------------------- tuner slots
BWS = [10_000, 20_000, 40_000]
SUBS = [7, 40, 3, 25, 64, 11, 30]              # submit lengths in units of `down`: uneven
# slot -> [(first submit, end submit, offset, bandwidth)]: set and cleared at several boundaries, a slot used twice at another
# offset and bandwidth, one slot active from the first submit, one to the last, one never
PLAN = {
    0: [(0, 3, 31_000, 10_000), (4, 7, -233_500, 40_000)],
    1: [(1, 2, -480_000, 40_000), (3, 6, 123_457, 20_000)],
    2: [(2, 7, 495_000, 10_000)],
    3: [],
    4: [(5, 6, 30_001, 20_000)],
}


def _plan_at(slot, s):
    for a, b, f, bw in PLAN[slot]:
        if a <= s < b:
            return f, bw
    return None


@pytest.mark.parametrize("strided", [False, True])
def test_slot_rows_equal_a_tuner_that_held_the_vfo_since_create(strided):
    r = 48_000
    up, down = R.ratio(FS, r)
    n = sum(SUBS) * down
    x, dev = _stream(FS, n, seed=17)
    n_slots = len(PLAN)
    tu = SondeTuner.slots(FS, r, n_slots, BWS, max(SUBS) * down)
    assert not any(tu.slot_active(k) for k in range(n_slots))
    out = torch.full((n_slots, 700, 2), float("nan"), device=DEV) if strided else None      # rows 700 apart, longer than any submit's
    got, a = [], 0
    for s, k in enumerate(SUBS):
        for slot in PLAN:
            now, before = _plan_at(slot, s), _plan_at(slot, s - 1) if s else None
            if now != before:
                if now is None:
                    tu.slot_clear(slot)
                else:
                    tu.slot_set(slot, *now)
            assert tu.slot_active(slot) == (now is not None)
        got.append(tu.process(dev[a:a + k * down].contiguous(), out=out).cpu().numpy().copy())
        a += k * down
    got = np.concatenate(got, axis=1)
    assert got.shape == (n_slots, n * up // down, 2) and not np.any(np.isnan(got))
    j_of = np.concatenate([[0], np.cumsum(SUBS)]) * up
    seen_active = seen_idle = 0
    for slot, spans in PLAN.items():
        idle = np.ones(got.shape[1], bool)
        for s0, s1, f, bw in spans:
            j0, j1 = int(j_of[s0]), int(j_of[s1])
            idle[j0:j1] = False
            # a sonde_tuner_create tuner with the same bandwidth set (one VFO per listed bandwidth), this VFO from the start
            others = [(0, b) for b in BWS if b != bw]
            ref = SondeTuner(FS, r, [(f, bw)] + others, max(SUBS) * down)
            want, a = [], 0
            for k in SUBS:
                want.append(ref.process(dev[a:a + k * down].contiguous())[0].cpu().numpy().copy())
                a += k * down
            want = np.concatenate(want, axis=0)
            ref.close()
            assert np.array_equal(got[slot, j0:j1].view(np.uint32), want[j0:j1].view(np.uint32)), (slot, s0, s1)
            # and within the formula bound of the float64 reference
            g = tuner_taps(FS, r, bw).astype(np.float64)
            y, A = R.tuner_ref(x, FS, r, g, [f] * len(SUBS), [k * down for k in SUBS], j_range=(j0, j1))
            bnd = R.bound(A, g.shape[1])
            gk = got[slot, j0:j1, 0] + 1j * got[slot, j0:j1, 1]
            assert len(y) == j1 - j0
            assert np.all(np.abs(gk.real - y.real) <= bnd) and np.all(np.abs(gk.imag - y.imag) <= bnd), (slot, s0)
            seen_active += 1
        assert not np.any(got[slot, idle].view(np.uint32)), f"slot {slot}: an idle stretch is not exactly zero"
        seen_idle += int(idle.any())
    assert seen_active == 6 and seen_idle == 5
    tu.close()


def test_a_tuner_with_every_slot_idle_writes_zeros():
    up, down = R.ratio(FS, 48_000)
    _, dev = _stream(FS, 40 * down, seed=2)
    tu = SondeTuner.slots(FS, 48_000, 70, BWS, 40 * down)          # more than one launch's worth of slots
    out = torch.full((70, 300, 2), float("nan"), device=DEV)
    y = tu.process(dev, out=out)
    assert y.shape == (70, 40 * up, 2) and not np.any(y.cpu().numpy().view(np.uint32))
    assert bool(torch.isnan(out[:, 40 * up:]).all())               # nothing beyond the rows was written
    tu.slot_set(69, 1000, 10_000)
    y = tu.process(dev, out=out).cpu().numpy()
    assert np.any(y[69]) and not np.any(y[:69].view(np.uint32))
    tu.close()


def test_slot_refusals():
    up, down = R.ratio(FS, 48_000)
    tu = SondeTuner.slots(FS, 48_000, 3, BWS, 40 * down)
    with pytest.raises(SondeError, match="listed"):
        tu.slot_set(0, 0, 15_000)
    with pytest.raises(SondeError, match="inside the band"):
        tu.slot_set(0, 480_001, 40_000)
    tu.slot_set(0, 480_000, 40_000)
    with pytest.raises(SondeError, match="no such slot"):
        tu.slot_set(3, 0, 10_000)
    with pytest.raises(SondeError, match="no such slot"):
        tu.slot_clear(3)
    with pytest.raises(SondeError, match="idle"):
        tu.retune(1, 1000)
    with pytest.raises(SondeError, match="idle"):
        tu.retune(1, 1000, continuous=True)
    tu.retune(0, 1000)
    tu.slot_clear(0)
    with pytest.raises(SondeError, match="idle"):
        tu.retune(0, 2000)
    with pytest.raises(SondeError, match="bandwidth"):
        SondeTuner.slots(FS, 48_000, 3, [4000], 40 * down)
    with pytest.raises(SondeError, match="bad argument"):
        SondeTuner.slots(FS, 48_000, 3, [], 40 * down)
    tu.close()


# ---------------------------------------------------------------- restart of single batch channels
N_SUB = {False: 36 * 2048, True: 5 * 16384}            # samples per submit (AFSK batches: multiples of 16384)
SHAPES = {
    "rs41": ([0, 0, 0, 0], [1, 3]),
    "mixed": ([0, 3, 1, 0, 3, 1], [0, 1, 5]),
    "afsk": ([4, 5, 0, 4, 5], [0, 4, 2]),
}


def _batch_signal(types, n):
    rows = []
    for c, t in enumerate(types):
        rows.append(synth.make_batch(t, 1, n, seed=40 + c, ebn0_db=25.0, first_channel=c).iq[0])
    return torch.stack(rows).to(DEV).contiguous()


def _frag_bytes(frags, chans):
    """fragments field by field; floats by their bits (a NaN equals itself)"""
    def key(d):
        return tuple(np.float32(v).tobytes() if isinstance(v, float) else v for v in (getattr(d, n) for n, _ in d._fields_))
    return [(c, key(d)) for c, d in frags if c in chans]


def _feed_batch(b, iq, subs, restart_after=None, restart=()):
    """per submit: (frames, poll fragments); the restart is queued before the frames of the submit in front of it are read"""
    out = []
    for s in subs:
        b.submit(iq[:, s[0]:s[1]])
        if restart_after is not None and s == restart_after:
            b.restart_channels(restart)
        out.append((b.frames().copy(), b.poll()))
    return out


@pytest.mark.parametrize("flags,slices", [(0, 0), (_lib.FLAG_LATE_JOIN, 2), (_lib.FLAG_PIPELINE, 0)], ids=["default", "late_join_sliced", "pipeline"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_restart_equals_a_fresh_batch(shape, flags, slices):
    types, restart = SHAPES[shape]
    afsk = any(t in (4, 5) for t in types)
    ns, C_ = N_SUB[afsk], len(types)
    iq = _batch_signal(types, 4 * ns)
    subs = [(k * ns, (k + 1) * ns) for k in range(4)]
    kw = dict(types=np.array(types, np.uint8), flags=flags, time_slices=slices)
    live, never, fresh = (SondeBatch(C_, ns, **kw) for _ in range(3))
    got = _feed_batch(live, iq, subs, restart_after=subs[1], restart=restart)
    ref = _feed_batch(never, iq, subs)
    new = _feed_batch(fresh, iq, subs[2:])
    others = [c for c in range(C_) if c not in restart]
    # every channel had found frames before the restart
    before = np.concatenate([got[0][0], got[1][0]])
    assert all(np.any(before["channel"] == c) for c in range(C_)), np.bincount(before["channel"], minlength=C_)
    # the frames of the submit in front of the restart were read after it: all channels as if nothing had happened
    for k in (0, 1):
        assert got[k][0].tobytes() == ref[k][0].tobytes()
        assert _frag_bytes(got[k][1], range(C_)) == _frag_bytes(ref[k][1], range(C_))
    n_new = 0
    for k in (2, 3):
        f, fr = got[k][0], new[k - 2][0]
        assert f[np.isin(f["channel"], restart)].tobytes() == fr[np.isin(fr["channel"], restart)].tobytes(), (shape, k)
        assert f[np.isin(f["channel"], others)].tobytes() == ref[k][0][np.isin(ref[k][0]["channel"], others)].tobytes(), (shape, k)
        assert _frag_bytes(got[k][1], restart) == _frag_bytes(new[k - 2][1], restart)
        assert _frag_bytes(got[k][1], others) == _frag_bytes(ref[k][1], others)
        n_new += int(np.isin(f["channel"], restart).sum())
    assert n_new >= len(restart)                # the restarted channels decoded again, with bitpos counted from the restart
    for c in range(C_):
        want = fresh if c in restart else never
        assert live.nbits(c) == want.nbits(c), c
        assert live.state(c) == want.state(c), c
    assert all(live.nbits(c) < never.nbits(c) for c in restart)
    for b in (live, never, fresh):
        b.close()


def test_batch_restart_refusals():
    b = SondeBatch(2, 2048)
    with pytest.raises(SondeError, match="no such channel"):
        b.restart_channels([2])
    b.restart_channels([])
    b.restart_channels([1])                     # before the first submit: nothing to undo
    b.close()
    ch = SondeChannelizer()
    with pytest.raises(SondeError, match="channelizer"):
        ch.batch.restart_channels([0])
    ch.close()


# ---------------------------------------------------------------- restart of single detector channels
def test_detector_restart_equals_a_fresh_detector():
    types, restart = [0, 3, 1, 6, 2, 0], [1, 2, 5]
    ns = 24 * 2048
    iq = _batch_signal(types, 4 * ns)
    live, never, fresh = (SondeDetector(len(types), ns) for _ in range(3))
    for k in range(4):
        part = iq[:, k * ns:(k + 1) * ns]
        live.submit(part)
        never.submit(part)
        if k >= 2:
            fresh.submit(part)
        if k == 1:
            assert np.array_equal(never.results()["type"], types)           # decided before the restart
            live.restart_channels(restart)
    a, b, c = live.results(), never.results(), fresh.results()
    others = [i for i in range(len(types)) if i not in restart]
    for key in ("best", "pos", "type", "inverted"):
        assert np.array_equal(a[key][restart], c[key][restart]), key
        assert np.array_equal(a[key][others], b[key][others]), key
    assert np.array_equal(a["type"], types)
    assert np.all(a["pos"][restart] < 2 * ns) and not np.array_equal(a["pos"][restart], b["pos"][restart])
    with pytest.raises(SondeError, match="no such channel"):
        live.restart_channels([6])
    for d in (live, never, fresh):
        d.close()


# ---------------------------------------------------------------- end to end: sondes appear and vanish
GRANULE = 128_000                              # the iq48 chain's granule at 1 MS/s
N_LIVE = 104 * GRANULE                         # 13.3 s
SCAN_S, PROBE_S = 1.024, 2.048                 # 8 and 16 submits: scans and probe ends fall on submit boundaries exactly
LOSE_AFTER, MAX_PROBES = 3, 3
# (offset, type, first sample, end sample, drift Hz/s): carriers >= 60 kHz apart, less than half the band occupied
LIVE_SCENE = [
    (-400_000, 0, 0, N_LIVE, 0.0),                            # RS41, the whole time
    (-250_000, 1, 3_000_000, N_LIVE, 0.0),                    # DFM from 3 s
    (-100_000, 3, 0, 5_000_000, 0.0),                         # M10 until 5 s
    (250_000, 3, 8_000_000, N_LIVE, 0.0),                     # a second M10, elsewhere, from 8 s
    (100_000, 0, 4_000_000, N_LIVE, DRIFT[0]),                # RS41 from 4 s, drifting
]
NOISE_AT, NOISE_BW, NOISE_DB = 400_000, 12_000, 10.0          # the non-sonde: band-limited Gaussian noise
POOLS = {0: 2, 1: 1, 3: 1}


def _match(t, f, txs):
    if t == 0:
        return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx[8:], f["data"][8:f["len"]])]
    return [i for i, (_, tx) in enumerate(txs) if np.array_equal(tx, f["data"][:f["len"]])]


def _true_offset(k, n):
    f, _, _, _, r = LIVE_SCENE[k]
    return f + r * n / FS


@pytest.fixture(scope="module")
def live_run():
    sigma = 0.02
    iq, frames, symbols = synth.make_wideband_scene([(f, t) for f, t, _, _, _ in LIVE_SCENE], N_LIVE, fs=FS, seed=77, device=DEV, noise_sigma=sigma,
                                                    drift_hz_per_s=[r for *_, r in LIVE_SCENE], active=[(a, b) for _, _, a, b, _ in LIVE_SCENE])
    # the non-sonde: white noise NOISE_DB over the floor's density, cut to NOISE_BW by a brick wall, moved to NOISE_AT
    gen = torch.Generator(device=DEV)
    gen.manual_seed(991)
    w = torch.randn((N_LIVE, 2), generator=gen, device=DEV, dtype=torch.float32) * (sigma * 10.0 ** (NOISE_DB / 20.0))
    W = torch.fft.fft(torch.view_as_complex(w))
    fr = torch.fft.fftfreq(N_LIVE, d=1.0 / FS, device=DEV)
    W[fr.abs() > NOISE_BW / 2] = 0
    w = torch.fft.ifft(W) * torch.exp(2j * np.pi * NOISE_AT / FS * torch.arange(N_LIVE, device=DEV, dtype=torch.float64)).to(torch.complex64)
    iq = (iq + torch.view_as_real(w)).contiguous()
    del w, W, fr
    from sdrpp_radiosonde_amd import LiveReceiver
    rx = LiveReceiver(FS, POOLS, probes=4, scan_seconds=SCAN_S, probe_seconds=PROBE_S, lose_after=LOSE_AFTER, max_probes=MAX_PROBES)
    assert rx.granule == GRANULE and rx.sondes() == []
    got, when, probing, n_all, frags = [], [], [], 0, []
    for a in range(0, N_LIVE, GRANULE):
        rx.submit(iq[a:a + GRANULE])
        f = rx.frames()
        n_all += len(rx.frames(valid_only=False))
        got.append(f)
        when.append(np.full(len(f), a, np.int64))
        probing.append(sorted(q["offset"] for q in rx.policy.probes.values()))
        if (a // GRANULE) % 2:                                  # poll every second submit: two submits' fragments per call
            frags += [(a, sid, d.serial.decode(errors="replace"), round(float(d.lat), 4)) for sid, d in rx.poll()]
    got, when = np.concatenate(got), np.concatenate(when)
    events, final = list(rx.events), rx.sondes()
    log = {k: list(v) for k, v in rx.track_log.items()}
    rx.close()
    for e in events:
        print("event:", e)
    print(f"frames reported {len(got)}; recorded by the batch with a failed checksum or FEC and left out: {n_all - len(got)}")
    # what a sonde can leave: one frame while its slot acquires (the VFO starts where the scanner saw the carrier) and one when
    # its carrier ends in mid-frame; five slots acquire in this scene and one carrier ends
    assert n_all - len(got) <= len(LIVE_SCENE) + 1
    return iq, frames, symbols, (got, when), events, final, probing, log, frags


def _found_of(events, k):
    """the found events of true sonde k: right type, within 10 kHz of where the carrier was"""
    return [e for e in events if e[0] == "found" and e[4] == LIVE_SCENE[k][1] and abs(e[3] - _true_offset(k, e[1])) <= 10_000]


def test_live_found_lost_and_the_non_sonde(live_run):
    iq, frames, symbols, (got, when), events, final, probing, log, frags = live_run
    S, P = int(SCAN_S * FS), int(PROBE_S * FS)
    found = [e for e in events if e[0] == "found"]
    # (a) one found event per sonde, the right type, within 10 kHz, in time
    assert len(found) == len(LIVE_SCENE), found
    ids = []
    for k, (f, t, a, b, r) in enumerate(LIVE_SCENE):
        ev = _found_of(events, k)
        assert len(ev) == 1, (k, ev)
        assert ev[0][1] <= a + S + P + S, (k, ev[0], a)
        ids.append(ev[0][2])
    assert sorted(ids) == list(range(len(LIVE_SCENE)))                   # ids never repeat
    # (b) the first M10 is lost in time, and silent afterwards
    lost = [e for e in events if e[0] == "lost"]
    assert [e[2] for e in lost] == [ids[2]], lost
    assert lost[0][1] <= LIVE_SCENE[2][3] + (LOSE_AFTER + 1) * S
    assert np.any(got["channel"] == ids[2]) and not np.any((got["channel"] == ids[2]) & (when >= lost[0][1]))
    assert ids[2] not in [v[0] for v in final]
    # (c) the non-sonde never gets an id, and stops taking a probe slot
    near = [e for e in events if abs(e[3] - NOISE_AT) <= 10_000]
    assert [e[0] for e in near] == ["probe"] * MAX_PROBES + ["ignored"], near
    last_probe = max(i for i, p in enumerate(probing) if any(abs(f - NOISE_AT) <= 10_000 for f in p))
    assert last_probe < len(probing) - 16                                # free for the last two seconds and more
    # (f) the second M10 took the first one's slot with a new id
    assert ids[3] != ids[2] and [v[1] for v in final if v[0] == ids[3]] == [3]
    assert {v[0] for v in final} == {ids[0], ids[1], ids[3], ids[4]}
    # the drifting RS41 was followed
    assert len(log[ids[4]]) > 0 and abs(log[ids[4]][-1][1] - _true_offset(4, N_LIVE)) <= 1000


def test_live_poll_reports_each_fragment_under_the_id_it_was_decoded_for(live_run):
    """poll() every second submit: a call returns two submits' fragments, and the M10 slot changes hands between two polls"""
    events, frags = live_run[4], live_run[8]
    ids = [_found_of(events, k)[0][2] for k in range(len(LIVE_SCENE))]
    found_at = {e[2]: e[1] for e in events if e[0] == "found"}
    lost_at = {e[2]: e[1] for e in events if e[0] == "lost"}
    by_id = {}
    lats = {}
    for a, sid, serial, lat in frags:
        assert sid in found_at and a + GRANULE > found_at[sid], (a, sid)            # no fragment before its sonde was found
        assert sid not in lost_at or a - GRANULE < lost_at[sid], (a, sid)           # none from submits after it was lost
        by_id.setdefault(sid, set()).add(serial)
        if lat:
            lats.setdefault(sid, set()).add(lat)
    assert set(by_id) == set(ids), (sorted(by_id), ids)                             # every sonde's parser produced fragments
    serials = {sid: {s for s in v if s} for sid, v in by_id.items()}
    assert all(len(v) <= 1 for v in serials.values()), serials                      # one sonde, one serial number
    assert serials[ids[0]] and serials[ids[4]] and not serials[ids[0]] & serials[ids[4]]      # the two RS41s
    # M10 frames carry no serial number; the scene's M10 number k reports latitude 47 + k / 1000: the slot's second tenant is not the first
    assert lats[ids[2]] == {round(47.0 + 2e-3, 4)} and lats[ids[3]] == {round(47.0 + 3e-3, 4)}, (lats[ids[2]], lats[ids[3]])


def test_live_frames_against_a_receiver_with_outside_knowledge(live_run):
    iq, frames, symbols, (got, when), events, final, probing, log, frags = live_run
    lost_at = {e[2]: e[1] for e in events if e[0] == "lost"}
    hits = {}
    for k, (f, t, a, b, r) in enumerate(LIVE_SCENE):
        ev = _found_of(events, k)[0]
        n0, sid = ev[1], ev[2]
        mine = got[got["channel"] == sid]
        # (d) every frame reported is a transmitted frame of that sonde, byte for byte
        hit = set()
        for fr in mine:
            m = _match(t, fr, frames[k])
            assert m, f"sonde {k} (id {sid}): a reported frame matches no transmitted one"
            hit.update(m)
        hits[k] = hit
        # (e) the yardstick: existing code, the true offset and type, the same stream from the found sample on
        end = min(b, N_LIVE)
        rx = WidebandReceiver(FS, [(int(round(_true_offset(k, n0))), t)], chain="iq48", track=True)
        assert rx.granule == GRANULE and n0 % GRANULE == 0
        ref = []
        for s in range(n0, N_LIVE, GRANULE):
            rx.submit(iq[s:s + GRANULE])
            ref.append(rx.frames())
        rx.close()
        yard = set()
        for fr in np.concatenate(ref):
            yard.update(_match(t, fr, frames[k]))
        baud = synth.SCENE_BAUD[t]
        starts = np.array([p for p, _ in frames[k]]) * FS / baud
        period = float(np.median(np.diff(starts)))
        sent = {i for i, p in enumerate(starts) if p >= n0 and p + period <= end}
        print(f"sonde {k} type {t} id {sid}: found at {n0}, sent {len(sent)}, yardstick {len(yard & sent)}, live {len(hit & sent)}")
        assert len(sent) >= 2, (k, len(sent))
        assert len(sent - yard) <= 1, (k, sorted(sent - yard))             # the yardstick itself loses at most one: the scene hides nothing
        assert len((yard & sent) - hit) <= 1, (k, sorted((yard & sent) - hit))
        if sid in lost_at:                                                # (b) nothing under a lost sonde's id that was sent after it fell silent
            assert all(starts[i] < end for i in hit)
    # (f) the second M10's frames are none of the first one's
    a, b = [frames[2][i][1].tobytes() for i in hits[2]], [frames[3][i][1].tobytes() for i in hits[3]]
    assert hits[3] and not set(a) & set(b)
