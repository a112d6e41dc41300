"""Cost and gain of the coherent antenna combiner.

Cost: HIP-event time of one SondeCombiner.process (its three launches) over S sondes x K antennas x one second of 48 kHz rows
(48 128 samples, 47 blocks of 1024), warm, on one stream, interleaved with a plain streamed read (sonde_hbm_read_probe) of as many
bytes as the (K + 1) * S rows the combiner must at least move once: one JSON line with the median, minimum and maximum of each over
--reps repetitions.

Gain: frames the GPU decoder delivers per GFSK sonde type over an Eb/N0 sweep, --channels sondes x --seconds each, from (a) one
antenna, (b) the better of two (per sonde), (c) the combiner with K = 2, (d) with K = 4; equal antennas at gains of their own under
noise of their own.  One JSON line per type and Eb/N0.

    python tools/combine_measure.py [--sondes 512] [--antennas 2] [--reps 15] [--ebn0 6,8,10,12,14] [--types 0,1,2,3,6] [--skip-gain]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import _lib, synth                              # noqa: E402
from sdrpp_radiosonde_amd.batch import SondeBatch                         # noqa: E402
from sdrpp_radiosonde_amd.combine import SondeCombiner                    # noqa: E402

DEV = "cuda:0"
N_SECOND = 48_128              # one second of rows in whole blocks of 1024


def cost(S, K, reps, warmup):
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    rows = torch.randn((K * S, N_SECOND, 2), generator=g, device=DEV)
    out = torch.empty((S, N_SECOND, 2), device=DEV)
    comb = SondeCombiner(S, K, 48_000, N_SECOND)
    st = torch.cuda.current_stream()
    nbytes = (K + 1) * S * N_SECOND * 8
    probe = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV).normal_()
    L = _lib.load()
    for _ in range(warmup):
        comb.process(rows, out=out)
    torch.cuda.synchronize()
    us, read_us = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        comb.process(rows, out=out)
        e1.record(st)
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
        gbs = C.c_float()
        if L.sonde_hbm_read_probe(C.c_void_p(probe.data_ptr()), nbytes, 3, C.byref(gbs)) != 0:
            raise RuntimeError(_lib.last_error())
        read_us.append(nbytes / (gbs.value * 1e9) * 1e6)
    print(json.dumps({"sondes": S, "antennas": K, "samples": N_SECOND, "block": comb.block, "reps": reps,
                      "submit_us": {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)},
                      "plain_read_us": {"median": round(statistics.median(read_us), 1), "min": round(min(read_us), 1), "max": round(max(read_us), 1)},
                      "bytes_moved_at_least": nbytes}), flush=True)
    comb.close()


def _count(fr, t, frames):
    """transmitted frames (whole ones) of each channel found among the records"""
    hit = np.zeros(len(frames), dtype=np.int64)
    for c, lst in enumerate(frames):
        mine = fr[fr["channel"] == c]
        have = {bytes(f["data"][8 if t == 0 else 0:f["len"]]) for f in mine}
        hit[c] = sum(bytes(tx[8:] if t == 0 else tx) in have for _, tx in lst)
    return hit


def gain(types, ebn0s, channels, seconds):
    n = seconds * 48_000 // 2048 * 2048
    for t in types:
        sb = synth.make_batch(t, channels, n, seed=8, ebn0_db=60.0, amp_range=(1.0, 1.0), device=DEV)
        s = torch.view_as_complex(sb.iq.contiguous())
        sent = sum(len(f) for f in sb.frames)
        stride = int(_lib.load().sonde_row_stride(n, _lib.INPUT_IQ))
        buf = torch.empty((channels, stride, 2), dtype=torch.float32, device=DEV)
        rng = np.random.default_rng(3)
        ph = torch.from_numpy(np.exp(2j * np.pi * rng.uniform(size=4))).to(DEV)
        for e in ebn0s:
            sig = math.sqrt((48_000 / synth.SCENE_BAUD[t]) / (2.0 * 10.0 ** (e / 10.0)))
            gen = torch.Generator(device=DEV)
            gen.manual_seed(100 + int(10 * e))
            ant = torch.empty((4 * channels, n, 2), dtype=torch.float32, device=DEV)
            for a in range(4):
                ant[a * channels:(a + 1) * channels] = torch.view_as_real((s * ph[a]).to(torch.complex64)) + \
                    sig * torch.randn((channels, n, 2), generator=gen, device=DEV)

            def decode(rows):
                buf[:, :n] = rows
                b = SondeBatch(channels, n, types=np.full(channels, t, dtype=np.uint8), input_kind=_lib.INPUT_IQ)
                b.submit(buf[:, :n], torch.cuda.current_stream().cuda_stream)
                f = b.frames()
                b.close()
                return _count(f, t, sb.frames)
            one, two = decode(ant[:channels]), decode(ant[channels:2 * channels])
            res = {"type": t, "ebn0_db": e, "sent": sent, "one_antenna": int(one.sum()), "better_of_two": int(np.maximum(one, two).sum())}
            for K in (2, 4):
                comb = SondeCombiner(channels, K, 48_000, n)
                res[f"coherent_{K}"] = int(decode(comb.process(ant[:K * channels])).sum())
                comb.close()
            print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sondes", type=int, default=512)
    ap.add_argument("--antennas", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ebn0", default="6,8,10,12,14")
    ap.add_argument("--types", default="0,1,2,3,6")
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=4)
    ap.add_argument("--skip-gain", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    a = ap.parse_args()
    if not a.skip_cost:
        cost(a.sondes, a.antennas, a.reps, a.warmup)
    if not a.skip_gain:
        gain([int(t) for t in a.types.split(",")], [float(e) for e in a.ebn0.split(",")], a.channels, a.seconds)


if __name__ == "__main__":
    main()
