"""Cost of the band scanner: submits of 1 280 000-sample blocks of one 10 MS/s complex stream, HIP-event timing on one
stream, warm.  One JSON line per (fft_size, input kind, blocks per submit): the median over --reps repetitions (each --inner
submits between two events) of the ms per submit, and two yardsticks taken in the same run, neither of them the code under test:
(a) the same spectrum through torch on the GPU (unfold -> window -> torch.fft.fft -> abs()**2 -> sum), float input only, and
(b) the time a plain device read of the block takes at the read rate this repository measured (6.2 TB/s).

    python tools/scan_rate.py [--sizes 4096,8192,16384] [--kinds iq,iq16,iq8] [--blocks 1,8] [--reps 10] [--inner 20]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import _lib                        # noqa: E402
from sdrpp_radiosonde_amd.scan import SondeScanner, window   # noqa: E402

FS = 10_000_000
BLOCK = 1_280_000              # one granule of the iq48 chain (0.128 s)
READ_RATE = 6.2e12             # bytes / s: the device read rate measured for the headline
KINDS = {"iq": (_lib.INPUT_IQ, 8), "iq16": (_lib.INPUT_IQ16, 4), "iq8": (_lib.INPUT_IQ8, 2)}


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
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192,16384")
    ap.add_argument("--kinds", default="iq,iq16,iq8")
    ap.add_argument("--blocks", default="1,8", help="granules of 1 280 000 samples per submit")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="submits between the two events of one repetition")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip yardstick (a)")
    a = ap.parse_args()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    for blocks in [int(b) for b in a.blocks.split(",")]:
        n = blocks * BLOCK
        base = torch.randn((n, 2), generator=g, device="cuda:0")
        for kind in a.kinds.split(","):
            code, nbytes = KINDS[kind]
            blk = base
            if kind == "iq16":
                blk = torch.round(base * 2000).to(torch.int16)
            elif kind == "iq8":
                blk = torch.clamp(torch.round(base * 30), -127, 127).to(torch.int8)
            for N in [int(v) for v in a.sizes.split(",")]:
                sc = SondeScanner(FS, n, fft_size=N, input_kind=code)
                st = torch.cuda.current_stream().cuda_stream
                med, best = timed(lambda: sc.submit(blk, stream=st), a.reps, a.inner, a.warmup)
                segs = sc.segments
                sc.close()
                row = {"fft_size": N, "kind": kind, "blocks": blocks, "samples": n, "reps": a.reps, "inner": a.inner,
                       "ms_per_submit": round(med, 4), "ms_min": round(best, 4), "segments_total": segs,
                       "ms_per_signal_second": round(med / (n / FS), 4)}
                floor_ms = n * nbytes / READ_RATE * 1e3
                row["read_floor_ms"] = round(floor_ms, 5)
                row["x_read_floor"] = round(med / floor_ms, 1)
                if kind == "iq" and not a.no_torch:
                    try:
                        w = torch.from_numpy(window(N)).to("cuda:0")
                        xc = torch.view_as_complex(blk)

                        def ref():
                            X = torch.fft.fft(xc.unfold(0, N, N // 2) * w)
                            return (X.abs() ** 2).sum(0)
                        tmed, tbest = timed(ref, a.reps, a.inner, a.warmup)
                        row["torch_ms"] = round(tmed, 4)
                        row["torch_ms_min"] = round(tbest, 4)
                        row["torch_over_scanner"] = round(tmed / med, 2)
                    except Exception as e:              # torch's FFT not usable on this build: the yardstick is dropped, and said so
                        row["torch_ms"] = None
                        row["torch_error"] = str(e)[:200]
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
