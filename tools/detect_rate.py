"""Throughput of the sonde type detector: C channels x n samples of complex IQ per submit, HIP-event timing over
repeated submits on one stream.  Prints ms per submit, ms per 1024 channel-seconds and G input samples/s as one JSON line.

    python tools/detect_rate.py [--channels 1024] [--samples 49152] [--reps 20] [--kind iq|iq16|iq8|real]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import _lib, synth                 # noqa: E402
from sdrpp_radiosonde_amd.detect import SondeDetector         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=49152)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kind", default="iq", choices=("iq", "iq16", "iq8", "real"))
    a = ap.parse_args()
    kind = {"iq": _lib.INPUT_IQ, "iq16": _lib.INPUT_IQ16, "iq8": _lib.INPUT_IQ8, "real": _lib.INPUT_REAL}[a.kind]
    C, n = a.channels, a.samples
    base = synth.make_batch(0, 64, n, seed=3, ebn0_db=20.0, cfo_max_hz=2000.0, device="cuda:0").iq
    iq = base.repeat((C + 63) // 64, 1, 1)[:C].contiguous()
    if kind == _lib.INPUT_IQ16:
        rows = torch.round(iq * 8000).to(torch.int16)
    elif kind == _lib.INPUT_IQ8:
        rows = torch.round(iq * 60).to(torch.int8)
    elif kind == _lib.INPUT_REAL:
        rows = torch.atan2(iq[..., 1], iq[..., 0]).contiguous()
    else:
        rows = iq
    det = SondeDetector(C, n, input_kind=kind)
    s = torch.cuda.current_stream()
    for _ in range(a.warmup):
        det.submit(rows, s.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.reps):
        det.submit(rows, s.cuda_stream)
    e1.record(s)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    ch_s = C * n / 48000.0
    print(json.dumps({"channels": C, "samples": n, "kind": a.kind, "reps": a.reps, "ms_per_submit": round(ms, 4),
                      "ms_per_1024_channel_seconds": round(ms * 1024.0 / ch_s, 4),
                      "gsamples_per_s": round(C * n / (ms * 1e-3) / 1e9, 2)}))
    det.close()


if __name__ == "__main__":
    main()
