#!/usr/bin/env python3
"""What SONDE_FLAG_MANCHESTER_RESCUE (DESIGN SPEC 3.3f) gains on noisy M10, M20 and MRZ-N1 signals, and what it costs:

    python tools/manchester_rescue_measure.py [--ebn0 9 10 11 12 13] [--channels 16] [--tiles 120] [--seed 700]
    python tools/manchester_rescue_measure.py --cost [--channels 1024] [--tiles 24] [--ebn0 10 25] [--steps 40] [--reps 7]

Gain: synth.make_batch channels of each type at each Eb/N0; the same samples go through a batch without and with the flag; per
(type, Eb/N0) one JSON line: frames sent, records, records whose check passes without the flag (`clean`) and with it, the frames the
second pass rescued, and the rescued frames that are not the transmitted bytes (`rescued_wrong`: false accepts, listed with their
nerr[1] = marked bits and flips; the SPEC expects a few at low Eb/N0).

Cost: one M10 batch per Eb/N0, submit time (host clock around `steps` submits that end in a synchronise) with the flag off and on,
the two batches alternating `reps` times on the same samples; per Eb/N0 one JSON line with both medians and their ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import _lib, synth                    # noqa: E402
from sdrpp_radiosonde_amd.batch import SondeBatch               # noqa: E402

TILE = 2048
KINDS = {"M10": (3, False, 101), "M20": (3, True, 70), "MRZ-N1": (6, False, 45)}


def gain(args, name, ebn0):
    typ, m20, ln = KINDS[name]
    C, n = args.channels, TILE * args.tiles
    sb = synth.make_batch(typ, C, n, seed=args.seed, ebn0_db=ebn0, m20=m20, device="cuda:0")
    types = np.full(C, typ, dtype=np.uint8)
    res = {}
    for key, flags in (("off", 0), ("on", _lib.FLAG_MANCHESTER_RESCUE)):
        b = SondeBatch(C, n, types=types, flags=flags)
        b.submit(sb.iq)
        fr = b.frames()
        tried = sum(b.manchester_rescue_info(c)["tried"] for c in range(C)) if flags else 0
        b.close()
        good = rescued = 0
        wrong = []
        for f in fr:
            c = int(f["channel"])
            d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in sb.frames[c]), key=lambda t: t[0])
            sent = d < 64 and int(f["len"]) == ln and np.array_equal(f["data"][:ln], tx[:ln])
            if int(f["flags"]) & _lib.FRAME_RESCUED:
                rescued += 1
                if not sent:
                    wrong.append((c, int(f["bitpos"]), int(f["nerr"][1]), int(_lib.frame_flips(int(f["flags"])))))
            good += int(f["nerr"][0]) == 0 and sent
        res[key] = dict(records=int(len(fr)), check_passes=int((fr["nerr"][:, 0] == 0).sum()), delivered_right=int(good), tried=int(tried),
                        rescued=int(rescued), rescued_wrong=wrong)
    sent = sum(len(f) for f in sb.frames)
    return dict(type=name, ebn0_db=ebn0, channels=C, tiles=args.tiles, seed=args.seed, frames_sent=sent, **res)


def cost(args, ebn0):
    C, n = args.channels, TILE * args.tiles
    sb = synth.make_batch(3, C, n, seed=args.seed, ebn0_db=ebn0, device="cuda:0")
    types = np.full(C, 3, dtype=np.uint8)
    batches = {key: SondeBatch(C, n, types=types, flags=flags) for key, flags in (("off", 0), ("on", _lib.FLAG_MANCHESTER_RESCUE))}
    ms = {"off": [], "on": []}
    for b in batches.values():
        b.set_timing(0)
        for _ in range(10):
            b.submit(sb.iq)
        b.sync()
    for _ in range(args.reps):
        for key, b in batches.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.submit(sb.iq)
            b.sync()
            ms[key].append((time.perf_counter() - t0) * 1e3 / args.steps)
    fr = batches["on"].frames()
    out = dict(cost="M10", ebn0_db=ebn0, channels=C, tiles=args.tiles, steps=args.steps, reps=args.reps,
               records_last_submit=int(len(fr)), check_fails_last_submit=int((fr["nerr"][:, 0] != 0).sum()),
               rescued_last_submit=int((fr["flags"] & _lib.FRAME_RESCUED != 0).sum()),
               ms_off=[round(v, 4) for v in ms["off"]], ms_on=[round(v, 4) for v in ms["on"]],
               median_off=round(statistics.median(ms["off"]), 4), median_on=round(statistics.median(ms["on"]), 4))
    out["on_over_off"] = round(out["median_on"] / out["median_off"], 4)
    for b in batches.values():
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--channels", type=int, default=None)
    ap.add_argument("--tiles", type=int, default=None)
    ap.add_argument("--ebn0", type=float, nargs="+", default=None)
    ap.add_argument("--seed", type=int, default=700)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", nargs="+", default=list(KINDS), choices=list(KINDS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("manchester_rescue_measure: no GPU (there is no CPU path)")
    if args.cost:
        args.channels, args.tiles = args.channels or 1024, args.tiles or 24
        for e in args.ebn0 or [10.0, 25.0]:
            print(json.dumps(cost(args, e)), flush=True)
        return
    args.channels, args.tiles = args.channels or 16, args.tiles or 120
    for name in args.types:
        for e in args.ebn0 or [9.0, 10.0, 11.0, 12.0, 13.0]:
            print(json.dumps(gain(args, name, e)), flush=True)


if __name__ == "__main__":
    main()
