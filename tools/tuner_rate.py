"""Throughput of the wideband tuner: V VFOs over one 10 MS/s complex stream, HIP-event timing over repeated submits
on one stream.  Both chains of WidebandReceiver: "iq48" (R = 48 kHz, B = 10 kHz: RS41) and "reference" (R = B = 10 kHz).  Prints one
JSON line per (chain, V): ms per submit, VFO-seconds of output per second of device time, and the fraction of the FP32 vector
peak by SPEC 3.9's count of useful work (4 T FLOP per output sample).

    python tools/tuner_rate.py [--vfos 16,64,256] [--blocks 1] [--reps 10] [--kind iq|iq16|iq8]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import _lib                         # noqa: E402
from sdrpp_radiosonde_amd.tuner import SondeTuner            # noqa: E402

FS = 10_000_000
BLOCK = 1_280_000              # one granule of the iq48 chain (0.128 s)
PEAK_FLOPS = 157.3e12          # MI355X FP32 vector peak (MI355X_MICROARCH.md)
CHAINS = {"iq48": (48_000, 10_000), "reference": (10_000, 10_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vfos", default="16,64,256")
    ap.add_argument("--blocks", type=int, default=1, help="granules of 1 280 000 samples per submit")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kind", default="iq", choices=("iq", "iq16", "iq8"))
    a = ap.parse_args()
    kind = {"iq": _lib.INPUT_IQ, "iq16": _lib.INPUT_IQ16, "iq8": _lib.INPUT_IQ8}[a.kind]
    n = a.blocks * BLOCK
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    blk = torch.randn((n, 2), generator=g, device="cuda:0")
    if kind == _lib.INPUT_IQ16:
        blk = torch.round(blk * 2000).to(torch.int16)
    elif kind == _lib.INPUT_IQ8:
        blk = torch.clamp(torch.round(blk * 30), -127, 127).to(torch.int8)
    s = torch.cuda.current_stream()
    for chain, (r, b) in CHAINS.items():
        for V in [int(v) for v in a.vfos.split(",")]:
            offs = [(int(-4_900_000 + k * (9_800_000 // V)) // 1000 * 1000 + 123, b) for k in range(V)]
            tu = SondeTuner(FS, r, offs, n, input_kind=kind)
            out = torch.empty((V, tu.out_samples(n), 2), device="cuda:0")
            for _ in range(a.warmup):
                tu.process(blk, out=out, stream=s.cuda_stream)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.reps):
                tu.process(blk, out=out, stream=s.cuda_stream)
            e1.record(s)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            T = 32 * -(-FS // b)
            flop = 4.0 * T * tu.out_samples(n) * V
            print(json.dumps({"chain": chain, "rate_out": r, "bandwidth": b, "vfos": V, "samples": n, "kind": a.kind, "reps": a.reps,
                              "ms_per_submit": round(ms, 4), "vfo_seconds_per_s": round(V * n / FS / (ms * 1e-3), 1),
                              "us_per_vfo_second": round(ms * 1e3 / (V * n / FS), 2),
                              "valu_peak_fraction": round(flop / (ms * 1e-3) / PEAK_FLOPS, 4)}), flush=True)
            tu.close()


if __name__ == "__main__":
    main()
