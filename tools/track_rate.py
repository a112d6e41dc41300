"""Cost of the carrier meter: HIP-event times of the meter's launch over V rows of one granule at 48 kHz (6144 samples),
next to the tuner's time for the same rows in the same process (10 MS/s, one 1 280 000-sample block, B = 10 kHz), warm, on one
stream.  One JSON line per V: the median over --reps repetitions (each --inner calls between two events) of the ms per call, and
the time a plain device read of the rows takes at the read rate this repository measured (6.2 TB/s).  Then WidebandReceiver.submit
+ frames() with track on and off, interleaved, wall clock, over a scene of --sondes RS41 sondes: median and spread of each.

    python tools/track_rate.py [--rows 8,64,512] [--reps 10] [--inner 20] [--sondes 8] [--submits 12]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import synth                                   # noqa: E402
from sdrpp_radiosonde_amd.track import SondeTracker                      # noqa: E402
from sdrpp_radiosonde_amd.tuner import SondeTuner, WidebandReceiver      # noqa: E402

FS = 10_000_000
BLOCK = 1_280_000              # one granule of the iq48 chain (0.128 s)
N48 = 6144
READ_RATE = 6.2e12             # bytes / s: the device read rate measured for the headline


def timed(fn, reps, inner, warmup):
    s = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(inner):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8,64,512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="calls between the two events of one repetition")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sondes", type=int, default=8)
    ap.add_argument("--submits", type=int, default=12, help="submits per receiver in the on / off comparison")
    a = ap.parse_args()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    blk = torch.randn((BLOCK, 2), generator=g, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for V in [int(v) for v in a.rows.split(",")]:
        offs = [(-4_000_000 + (8_000_000 // V) * k + 137, 10_000) for k in range(V)]
        tu = SondeTuner(FS, 48_000, offs, BLOCK)
        rows = tu.process(blk, stream=st)
        t_med, t_min, t_max = timed(lambda: tu.process(blk, out=rows, stream=st), max(3, a.reps // 2), max(1, a.inner // 10), 1)
        tr = SondeTracker(V, 48_000, N48)
        m_med, m_min, m_max = timed(lambda: tr.submit(rows, stream=st), a.reps, a.inner, a.warmup)
        floor_ms = V * N48 * 8 / READ_RATE * 1e3
        print(json.dumps({"rows": V, "samples": N48, "meter_ms": round(m_med, 5), "meter_ms_min": round(m_min, 5), "meter_ms_max": round(m_max, 5),
                          "tuner_ms": round(t_med, 4), "tuner_ms_min": round(t_min, 4), "meter_over_tuner": round(m_med / t_med, 6),
                          "read_floor_ms": round(floor_ms, 6), "x_read_floor": round(m_med / floor_ms, 1)}), flush=True)
        tr.close()
        tu.close()
    # the receiver, track on / off interleaved
    n = a.submits * BLOCK
    sondes = [(-3_500_000 + 900_000 * k + 321, 0) for k in range(a.sondes)]
    iq, _, _ = synth.make_wideband_scene(sondes, n, fs=FS, ebn0_db=20.0, seed=2, device="cuda:0", drift_hz_per_s=700.0)
    iq = iq.contiguous()
    rx = {on: WidebandReceiver(FS, sondes, chain="iq48", track=on) for on in (False, True)}
    ms = {False: [], True: []}
    for s in range(a.submits):
        part = iq[s * BLOCK:(s + 1) * BLOCK]
        for on in ((False, True) if s % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rx[on].submit(part)
            rx[on].frames()
            ms[on].append((time.perf_counter() - t0) * 1e3)
    out = {"sondes": a.sondes, "submits": a.submits}
    for on in (False, True):
        v = ms[on][2:]                                       # the first two submits of each are warm-up
        out["track_on" if on else "track_off"] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    out["retunes"] = [len({o for _, o, _, _ in lg}) for lg in rx[True].track_log]
    print(json.dumps(out), flush=True)
    for r in rx.values():
        r.close()


if __name__ == "__main__":
    main()
