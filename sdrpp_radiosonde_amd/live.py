"""Python face of the live receiver (include/sonde_abi.h, DESIGN SPEC 3.12): a wideband receiver that is left running while sondes
appear and vanish.

    match           the matching rule: which scan candidate belongs to which live VFO (sonde_live_match: pure host)
    LivePolicy      the rule book, no GPU: scan candidates and probe detections in, actions and events out
    LiveReceiver    wideband stream -> slot tuner -> decoders / carrier meter / type detector, a scanner beside them; executes the policy
                    (the "iq48" chain of _chain.py, which WidebandReceiver and DiversityReceiver share)

Nothing here computes on the samples: the tuner, the batch, the meter, the detector and the scanner are the library's HIP objects."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _chain, _lib
from ._chain import IQ48_MAX_BW as PROBE_BW          # the bandwidth of every probe VFO
from ._handle import chk, current_stream
from ._lib import INPUT_IQ, SondeError
from .batch import VFO_RATE

MATCH_HZ = 10000           # the scanner's min_sep_hz default: a candidate this close to a VFO is that VFO's carrier


def match(vfo_offsets, cand_offsets, match_hz: int = 0):
    """(cand_of_vfo, vfo_of_cand), int32 arrays, -1 = unmatched (sonde_live_match)"""
    v = np.ascontiguousarray(vfo_offsets, dtype=np.int32).reshape(-1)
    c = np.ascontiguousarray(cand_offsets, dtype=np.int32).reshape(-1)
    cv, vc = np.full(len(v), -1, np.int32), np.full(len(c), -1, np.int32)
    chk(_lib.load().sonde_live_match(v.ctypes.data_as(C.c_void_p), len(v), c.ctypes.data_as(C.c_void_p), len(c), int(match_hz),
                                     cv.ctypes.data_as(C.c_void_p), vc.ctypes.data_as(C.c_void_p)))
    return cv, vc


def frame_ok(frames) -> np.ndarray:
    """which frames passed their own check, by the rule parse.cpp applies per sonde type: RS41 both codewords corrected; DFM and
    iMS-100 no uncorrectable block (nerr[1] == 0); M10 / M20, iMet-4, SRS-C50 and MRZ-N1 the checksum (nerr[0] == 0).  The batch
    records frames that fail (a host may count them); a carrier that falls silent in mid-frame leaves one.  A frame with
    FRAME_DUPLICATE (set_diversity(mark_duplicates=True): another receiver of the group has delivered it) is left out like a failed
    one; without that mode no record carries the flag."""
    t, e0, e1 = frames["type"], frames["nerr"][:, 0], frames["nerr"][:, 1]
    ok = np.where(t == 0, (e0 >= 0) & (e1 >= 0), np.where((t == 1) | (t == 2), e1 == 0, e0 == 0))
    return ok & ((frames["flags"] & _lib.FRAME_DUPLICATE) == 0)


def _pools(capacity) -> dict:
    if isinstance(capacity, dict):
        pools = {int(t): int(n) for t, n in sorted(capacity.items()) if int(n) > 0}
    else:
        pools = {t: int(capacity) for t in sorted(VFO_RATE)} if int(capacity) > 0 else {}
    if not pools or any(t not in VFO_RATE for t in pools):
        raise SondeError("capacity must be {sonde type: slots} or one positive int for every type")
    return pools


class LivePolicy:
    """What the live receiver does with what it sees; no GPU, no samples.  Decode slots are numbered pool by pool in ascending sonde
    type (slot = batch channel = tuner slot), the probe slots follow them in the tuner.  Times are input-sample counts.

        scan(n_in, offsets, cn0=None)     the scanner's candidates of the last scan period -> actions
        probes_due(n_in)                  probe slots whose probe_samples have passed
        probe_result(n_in, probe, type)   the detector's decision for one of them (-1 = none) -> actions
        moved(slot, offset_hz)            the tracking loop retuned a decode slot

    Actions, in the order they must be executed before the next submit:
        ("clear", slot)                         idle the decode slot (its sonde is lost)
        ("decode", slot, offset_hz, type)       tune the decode slot, restart its batch channel and meter row
        ("probe", probe, offset_hz)             tune the probe slot at PROBE_BW, restart its detector channel
        ("release", probe)                      idle the probe slot
    `events`: ("found" | "lost", n_in, id, offset_hz, type), ("full", n_in, -1, offset_hz, type) once per candidate, and, for the
    curious, ("probe" | "ignored", n_in, -1, offset_hz, -1).  `vfos[slot]`: id, offset, type, found_at, misses, cn0.  hold(slot):
    the carrier was not seen in the last scan -- the tracking loop does not retune on looks of an empty frequency."""

    def __init__(self, rate_in: int, capacity, probes: int = 8, *, probe_samples: int, lose_after: int = 3, max_probes: int = 3,
                 match_hz: int = 0, matcher=None):
        self.rate_in = int(rate_in)
        self.pools = _pools(capacity)
        self.n_probes = int(probes)
        self.probe_samples, self.lose_after, self.max_probes = int(probe_samples), int(lose_after), int(max_probes)
        if self.n_probes < 1 or self.lose_after < 1 or self.max_probes < 1 or self.probe_samples < 1:
            raise SondeError("probes, lose_after, max_probes and the probe time must be positive")
        self.match_hz = int(match_hz) or MATCH_HZ
        self._match = matcher or match
        self.slot_type, self.free = [], {}
        for t, n in self.pools.items():
            self.free[t] = list(range(len(self.slot_type), len(self.slot_type) + n))
            self.slot_type += [t] * n
        self.n_slots = len(self.slot_type)
        self.vfos = {}             # decode slot -> {"id", "offset", "type", "found_at", "misses", "cn0"}
        self.probes = {}           # probe slot -> {"offset", "until", "rec"}
        self.known = []            # candidates that are no sonde of ours (yet): {"offset", "tries", "ignored", "type", "full", "probing"}
        self.events = []
        self.next_id = 0

    # ---- helpers
    def hold(self, slot: int) -> bool:
        return self.vfos[slot]["misses"] > 0

    def moved(self, slot: int, offset_hz: int):
        self.vfos[slot]["offset"] = int(offset_hz)

    def fits(self, offset_hz: int) -> bool:
        return 2 * abs(int(offset_hz)) + PROBE_BW <= self.rate_in

    def _take(self, n_in, offset, t, cn0):
        """a free decode slot of type t for a new sonde, or None"""
        if not self.free.get(t):
            return None
        slot = self.free[t].pop(0)
        self.vfos[slot] = {"id": self.next_id, "offset": int(offset), "type": int(t), "found_at": int(n_in), "misses": 0, "cn0": float(cn0)}
        self.events.append(("found", int(n_in), self.next_id, int(offset), int(t)))
        self.next_id += 1
        return ("decode", slot, int(offset), int(t))

    def add_initial(self, offset_hz: int, t: int):
        act = self._take(0, offset_hz, int(t), float("nan"))
        if act is None:
            raise SondeError(f"initial: no free slot for sonde type {t}")
        return act

    # ---- the scan
    def scan(self, n_in: int, offsets, cn0=None):
        offsets = [int(f) for f in offsets]
        cn0 = [float("nan")] * len(offsets) if cn0 is None else [float(x) for x in cn0]
        actions = []
        slots = sorted(self.vfos)
        cand_of_vfo, vfo_of_cand = self._match([self.vfos[s]["offset"] for s in slots], offsets, self.match_hz)
        for k, slot in enumerate(slots):
            v = self.vfos[slot]
            if cand_of_vfo[k] >= 0:
                v["misses"] = 0
                v["cn0"] = cn0[int(cand_of_vfo[k])]
                continue
            v["misses"] += 1
            if v["misses"] >= self.lose_after:
                del self.vfos[slot]
                self.free[v["type"]].append(slot)
                self.free[v["type"]].sort()
                self.events.append(("lost", int(n_in), v["id"], v["offset"], v["type"]))
                actions.append(("clear", slot))
        rest = [i for i in range(len(offsets)) if vfo_of_cand[i] < 0]
        # the candidates we already know: the nearest record within match_hz; a record not seen in this scan is forgotten
        _, rec_of = self._match([r["offset"] for r in self.known], [offsets[i] for i in rest], self.match_hz)
        seen = set(int(r) for r in rec_of if r >= 0)
        todo = []
        for j, i in enumerate(rest):
            if rec_of[j] >= 0:
                rec = self.known[int(rec_of[j])]
                rec["offset"] = offsets[i]                                  # the newest sighting: where a drifting carrier is now
                rec["cn0"] = cn0[i]
            else:
                rec = {"offset": offsets[i], "tries": 0, "ignored": False, "type": -1, "full": False, "probing": False}
                self.known.append(rec)
            todo.append((offsets[i], cn0[i], rec))
        self.known = [r for k, r in enumerate(self.known) if k in seen or r["probing"] or any(r is t[2] for t in todo)]
        for f, c, rec in sorted(todo, key=lambda t: t[0]):                 # ascending offset: who waits for a probe slot waits in this order
            if rec["probing"] or rec["ignored"]:
                continue
            if rec["type"] >= 0:                                            # typed before, its pool was full
                act = self._take(n_in, f, rec["type"], c)
                if act is not None:
                    self.known.remove(rec)
                    actions.append(act)
                continue
            if not self.fits(f):
                continue
            p = next((p for p in range(self.n_probes) if p not in self.probes), None)
            if p is None:
                continue
            rec["probing"] = True
            rec["cn0"] = c
            self.probes[p] = {"offset": f, "until": int(n_in) + self.probe_samples, "rec": rec}
            self.events.append(("probe", int(n_in), -1, f, -1))
            actions.append(("probe", p, f))
        return actions

    # ---- the probes
    def probes_due(self, n_in: int):
        return sorted(p for p, q in self.probes.items() if n_in >= q["until"])

    def probe_result(self, n_in: int, probe: int, t: int):
        q = self.probes.pop(int(probe))
        rec, t = q["rec"], int(t)
        rec["probing"] = False
        actions = [("release", int(probe))]
        if t >= 0 and t in self.pools:
            act = self._take(n_in, rec["offset"], t, rec.get("cn0", float("nan")))      # at the candidate's newest offset, not the probe's
            if act is not None:
                if rec in self.known:
                    self.known.remove(rec)
                actions.append(act)
            else:
                rec["type"] = t
                if not rec["full"]:
                    rec["full"] = True
                    self.events.append(("full", int(n_in), -1, rec["offset"], t))
            return actions
        rec["tries"] += 1
        if rec["tries"] >= self.max_probes:
            rec["ignored"] = True
            self.events.append(("ignored", int(n_in), -1, q["offset"], -1))
        return actions


class LiveReceiver:
    """Decode the sondes of one wideband stream as they appear and vanish (SPEC 3.12).  Only the iq48 chain: one slot tuner at
    48 kHz into one SondeBatch(INPUT_IQ); the reference chain needs one tuner per VFO rate and is left out.

    capacity: {sonde type: decode slots} or one int for every type -- the pools; a new sonde of a type takes a free slot of its
    pool.  probes: slots (40 kHz VFOs into one SondeDetector) that tell what an unknown carrier is.  initial: [(offset_hz, type)]
    decoded from the first submit on, no probing.  One SondeScanner sees every submit; every scan_seconds of input its candidates
    are matched against the live VFOs (match) and LivePolicy decides: a sonde not seen lose_after scans running is lost and its slot
    cleared; an unknown carrier is probed for probe_seconds, typed and given a slot and an id (ids never repeat), up to max_probes
    times.  Between a miss and the next sighting the tracking loop holds (track=True follows drifting carriers as
    WidebandReceiver does).  scan_seconds and probe_seconds take effect at submit boundaries.

    submit() takes a device block [n, 2], n a multiple of `granule` and <= max_in.  frames() / poll() report the sonde id as
    `channel` (frames(): only frames whose checksum or FEC passed, unless valid_only=False); sondes() lists (id, slot, offset_hz, type, found_at, cn0_dbhz); `events` is the policy's log, `track_log[id]` lists
    (first input sample the offset applies from, offset_hz, err_hz, level_db) per look acted on."""

    def __init__(self, rate_in: int, capacity, *, probes: int = 8, initial=(), input_kind: int = INPUT_IQ, device: int = 0, max_in: int | None = None,
                 scan_seconds: float = 1.0, probe_seconds: float = 2.0, lose_after: int = 3, max_probes: int = 3, track: bool = True,
                 track_params: dict | None = None, rescue: bool = False, manchester_rescue: bool = False,
                 dfm_rescue: bool = False, ims_rescue: bool = False, afsk_rescue: bool = False):
        from .detect import SondeDetector
        from .scan import SondeScanner
        from .tuner import SondeTuner
        self.rate_in, self.device, self.input_kind = int(rate_in), int(device), int(input_kind)
        fs = self.rate_in
        self.scan_samples = max(1, int(round(float(scan_seconds) * fs)))
        self.policy = LivePolicy(fs, capacity, probes, probe_samples=max(1, int(round(float(probe_seconds) * fs))), lose_after=lose_after,
                                 max_probes=max_probes)
        pol = self.policy
        p = _chain.plan(fs, pol.pools, max_in)
        self.granule, self.max_in, n48 = p.granule, p.max_in, p.n48
        self.n_dec, self.n_probes = pol.n_slots, pol.n_probes
        self._bw = {t: _chain.iq48_bandwidth(t) for t in pol.pools}
        self.tuner = SondeTuner.slots(fs, 48000, self.n_dec + self.n_probes, sorted(set(self._bw.values()) | {PROBE_BW}), self.max_in,
                                      input_kind=input_kind, device=device)
        self.batch = _chain.batch(self.n_dec, n48, pol.slot_type, device, (rescue, manchester_rescue, dfm_rescue, ims_rescue, afsk_rescue))
        self.detector = SondeDetector(self.n_probes, n48, device=device)
        self.scanner = SondeScanner(fs, self.max_in, input_kind=input_kind, device=device)
        self.track = bool(track)
        self.track_params = dict(track_params or {})
        self.tracker = None
        if self.track:
            from .track import SondeTracker
            self.tracker = SondeTracker(self.n_dec, 48000, n48, device=device, look_samples=int(self.track_params.get("look_samples", 0)))
        self._rows = _chain.rows(self.n_dec + self.n_probes, n48, device)
        self._n48 = 0
        self._n_in = 0
        self._next_scan = self.scan_samples
        self._id_of = np.full(self.n_dec, -1, np.int64)          # batch channel -> sonde id during the submits since the table last changed
        self._frags = []                                         # poll fragments of those submits, read before the table changed
        self.track_log = {}
        self.events = pol.events
        self._do([pol.add_initial(int(f), int(t)) for f, t in initial])

    # ---- the policy's actions
    def _drain_poll(self):
        """the batch's unpolled fragments (up to two submits) under the ids those submits ran with: called before a slot changes
        hands, so that every submit the batch still holds unpolled used the table as it stands"""
        try:
            got = self.batch.poll()
        except SondeError as e:
            if "overwritten" not in str(e):
                raise
            got = self.batch.poll()                              # the host does not poll: what is still resident
        self._frags += [(int(self._id_of[c]), d) for c, d in got if self._id_of[c] >= 0]

    def _do(self, actions):
        restart_dec, restart_det = [], []
        if self._n_in and any(a[0] in ("clear", "decode") for a in actions):
            self._drain_poll()
        for a in actions:
            if a[0] == "clear":
                self.tuner.slot_clear(a[1])
            elif a[0] == "decode":
                _, slot, f, t = a
                self.tuner.slot_set(slot, f, self._bw[t])
                restart_dec.append(slot)
                self.track_log[self.policy.vfos[slot]["id"]] = []
            elif a[0] == "probe":
                self.tuner.slot_set(self.n_dec + a[1], a[2], PROBE_BW)
                restart_det.append(a[1])
            elif a[0] == "release":
                self.tuner.slot_clear(self.n_dec + a[1])
        if restart_dec:
            self.batch.restart_channels(restart_dec)
            for slot in restart_dec:
                if self.tracker is not None:
                    self.tracker.restart(slot)
        if restart_det:
            self.detector.restart_channels(restart_det)

    def _track_update(self):
        """the loop of SPEC 3.11 over the live slots whose carrier the last scan saw"""
        tr, tu, pol = self.tracker, self.tuner, self.policy

        def skip(slot):          # unowned, held, or found in the submit the look was taken from
            return slot not in pol.vfos or pol.hold(slot) or pol.vfos[slot]["found_at"] >= self._n_in
        for slot, new, err, level in _chain.track_looks(tr, tu, self.rate_in, self.track_params, skip):
            if new != tu.offsets[slot]:
                tu.retune(slot, new, continuous=True)
                tr.restart(slot)
                pol.moved(slot, new)
            self.track_log[pol.vfos[slot]["id"]].append((self._n_in, new, err, level))

    def _housekeeping(self):
        """between two submits: probes whose time is up, then the scan if one is due, then the tracking loop"""
        pol, n = self.policy, self._n_in
        due = pol.probes_due(n)
        if due:
            kind = self.detector.results()["type"]
            for p in due:
                self._do(pol.probe_result(n, p, int(kind[p])))
        if n >= self._next_scan:
            while self._next_scan <= n:
                self._next_scan += self.scan_samples
            if self.scanner.segments > 0:                          # (a scan period shorter than one segment: the spectrum goes on averaging)
                cand = self.scanner.candidates()
                self.scanner.reset()
                self._do(pol.scan(n, cand["offset_hz"], cand["cn0_dbhz"]))
        if self.track:
            self._track_update()

    # ---- the stream
    def rows(self):
        """the 48 kHz rows of the last submit: decode slots, then probe slots (idle ones: zeros)"""
        return self._rows[:, :self._n48]

    def submit(self, block, stream: int | None = None):
        n = int(block.shape[0])
        _chain.check_block(n, self.granule, self.max_in)
        if stream is None:
            stream = current_stream(self.device)
        if self._n_in:
            self._housekeeping()
        n48 = _chain.out48(self.rate_in, n)
        self.scanner.submit(block, stream)
        self.tuner.process(block, out=self._rows, stream=stream)
        dec, prb = self._rows[:self.n_dec, :n48], self._rows[self.n_dec:, :n48]
        if self.tracker is not None:
            self.tracker.submit(dec, stream)
        self.detector.submit(prb, stream)
        self.batch.submit(dec, stream)
        self._id_of[:] = -1
        for slot, v in self.policy.vfos.items():
            self._id_of[slot] = v["id"]
        self._n48 = n48
        self._n_in += n

    def frames(self, valid_only: bool = True) -> np.ndarray:
        """the last submit's frames of the live sondes; `channel` is the sonde id.  valid_only leaves out the frames the batch
        records although their checksum or FEC failed (frame_ok): a receiver that is left running sees carriers cut off in mid-frame"""
        f = self.batch.frames()
        f = f[self._id_of[f["channel"]] >= 0]
        if valid_only:
            f = f[frame_ok(f)]
        f["channel"] = self._id_of[f["channel"]]
        return f

    def poll(self):
        """[(sonde id, SondeData), ...] of the submits since the last poll (SondeBatch.poll: poll at least every second submit).  A
        slot that changed hands in between reports each fragment under the id it was decoded for."""
        self._drain_poll()
        out, self._frags = self._frags, []
        return out

    def sondes(self):
        """[(id, slot, offset_hz, type, found_at, cn0_dbhz)] of the live sondes, by slot"""
        return [(v["id"], s, v["offset"], v["type"], v["found_at"], v["cn0"]) for s, v in sorted(self.policy.vfos.items())]

    def close(self):
        for o in (self.tuner, self.batch, self.detector, self.scanner, self.tracker):
            if o is not None:
                o.close()
        self.tracker = None
