#!/usr/bin/env python3
"""What SONDE_FLAG_DFM_RESCUE (DESIGN SPEC 3.3g) gains on noisy DFM signals, and what it costs:

    python tools/dfm_rescue_measure.py [--ebn0 7 8 9 10 11 12] [--channels 8] [--tiles 100] [--seed 5] [--gpu]
    python tools/dfm_rescue_measure.py --cost [--steps 40] [--reps 7]

Gain (no GPU needed): synth.make_batch DFM channels at each Eb/N0 through the CPU oracle, the twin (tests/dfm_rescue_reference.py) over
its records and chips, and the conventional yardstick receiver (oracle/or_yardstick.c) on the same samples; one markdown table row
per Eb/N0: records on a transmitted frame, valid as recorded (nerr[1] == 0) and how many of those are the transmitted frame, failed,
rescued, rescued and right, the share of wrong frames among the rescued and among the first pass's own valid frames, and the
yardstick's valid frames.  --gpu adds the same counts from the library with the flag on (they must equal the twin's).

Cost (GPU): submit time (host clock around `steps` submits that end in a synchronise) with the flag off and on, the two batches
alternating `reps` times on the same samples: 1024 DFM channels x 24 tiles at Eb/N0 9 dB (frames to rescue) and 16 dB (none), and the
mixed batch of 4096 channels x 24 tiles (RS41, M10, DFM by channel % 3, 16 dB); one JSON line each with all values, both medians,
their ratio and the spread of each side."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sdrpp_radiosonde_amd import _lib, synth                    # noqa: E402

TILE = 2048
DFM = 1


def _tx(frames, f):
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in frames[c]), key=lambda t: t[0])
    return tx if d < 64 else None


def _count(frames, fr):
    """(records on a transmitted frame, valid, valid and right, rescued, rescued and right)"""
    on = valid = right = res = res_right = 0
    for f in fr:
        tx = _tx(frames, f)
        ok = tx is not None and np.array_equal(f["data"][:33], tx)
        on += tx is not None
        if int(f["nerr"][1]) == 0 and tx is not None:
            if int(f["flags"]) & _lib.FRAME_RESCUED:
                res += 1
                res_right += ok
            else:
                valid += 1
                right += ok
    return on, valid, right, res, res_right


def gain(args):
    import dfm_rescue_reference as dr
    import oracle_lib
    oracle_lib.build()
    C, n = args.channels, TILE * args.tiles
    print(f"DFM, {C} channels x {args.tiles} tiles, synth.make_batch seed {args.seed}; CPU oracle, twin, yardstick (oracle/or_yardstick.c)"
          + ("; gpu = libsonde_mi355.so with SONDE_FLAG_DFM_RESCUE" if args.gpu else ""))
    print()
    print("| Eb/N0 | records on a transmitted frame | valid today (right) | failed | rescued | rescued and right | wrong among rescued | "
          "wrong among first-pass valid | yardstick valid (right) |" + (" gpu valid / rescued (right) |" if args.gpu else ""))
    print("|---|---|---|---|---|---|---|---|---|" + ("---|" if args.gpu else ""))
    for e in args.ebn0:
        sb = synth.make_batch(DFM, C, n, seed=args.seed, ebn0_db=e)
        iq = sb.iq.numpy()
        recs, streams = [], []
        for c in range(C):
            ch = oracle_lib.Channel(DFM, c)
            ch.feed(iq[c])
            recs.append(ch.frames())
            streams.append(ch.bits())
        fr = np.concatenate(recs)
        out, outcomes, _ = dr.rescue(fr, dr.chips_of_streams(streams))
        on, valid, right, res, res_right = _count(sb.frames, out)
        y = oracle_lib.yard_run(DFM, iq)
        _, yvalid, yright, _, _ = _count(sb.frames, y)
        share = lambda bad, tot: f"{bad}/{tot}" + (f" = {100.0 * bad / tot:.1f} %" if tot else "")      # noqa: E731
        row = (f"| {e:g} dB | {on} | {valid} ({right}) | {on - valid} | {res} | {res_right} | {share(res - res_right, res)} | "
               f"{share(valid - right, valid)} | {yvalid} ({yright}) |")
        if args.gpu:
            import torch
            from sdrpp_radiosonde_amd.batch import SondeBatch
            b = SondeBatch(C, n, types=np.full(C, DFM, dtype=np.uint8), flags=_lib.FLAG_DFM_RESCUE)
            b.submit(torch.from_numpy(iq).to("cuda:0"))
            g = b.frames()
            b.close()
            _, gv, gr, gres, gres_right = _count(sb.frames, g)
            row += f" {gv} / {gres} ({gres_right}){'' if g.tobytes() == out.tobytes() else ' RECORDS DIFFER FROM THE TWIN'} |"
        print(row, flush=True)


def _time_pair(make, iq, steps, reps):
    from sdrpp_radiosonde_amd.batch import SondeBatch  # noqa: F401
    batches = {"off": make(0), "on": make(_lib.FLAG_DFM_RESCUE)}
    ms = {"off": [], "on": []}
    for b in batches.values():
        b.set_timing(0)
        for _ in range(10):
            b.submit(iq)
        b.sync()
    for _ in range(reps):
        for key, b in batches.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                b.submit(iq)
            b.sync()
            ms[key].append((time.perf_counter() - t0) * 1e3 / steps)
    fr = batches["on"].frames()
    out = dict(steps=steps, reps=reps, records_last_submit=int(len(fr)),
               dfm_failed_last_submit=int(((fr["type"] == DFM) & (fr["nerr"][:, 1] != 0)).sum()),
               dfm_rescued_last_submit=int(((fr["type"] == DFM) & (fr["flags"] & _lib.FRAME_RESCUED != 0)).sum()),
               ms_off=[round(v, 4) for v in ms["off"]], ms_on=[round(v, 4) for v in ms["on"]],
               median_off=round(statistics.median(ms["off"]), 4), median_on=round(statistics.median(ms["on"]), 4),
               spread_off=round(max(ms["off"]) - min(ms["off"]), 4), spread_on=round(max(ms["on"]) - min(ms["on"]), 4))
    out["on_over_off"] = round(out["median_on"] / out["median_off"], 4)
    for b in batches.values():
        b.close()
    return out


def cost(args):
    import torch
    from sdrpp_radiosonde_amd.batch import SondeBatch
    n = TILE * 24
    for e in (9.0, 16.0):
        C = 1024
        iq = synth.make_batch(DFM, C, n, seed=args.seed, ebn0_db=e, device="cuda:0").iq
        types = np.full(C, DFM, dtype=np.uint8)
        r = _time_pair(lambda flags: SondeBatch(C, n, types=types, flags=flags), iq, args.steps, args.reps)
        print(json.dumps(dict(cost="DFM", channels=C, tiles=24, ebn0_db=e, **r)), flush=True)
        del iq
    C = 4096
    order = (0, 3, 1)
    types = np.array([order[c % 3] for c in range(C)], dtype=np.uint8)
    full = torch.empty((C, n, 2), dtype=torch.float32, device="cuda:0")
    for t in order:
        idx = np.nonzero(types == t)[0]
        part = synth.make_batch(int(t), len(idx), n, seed=args.seed + 10 * t, ebn0_db=16.0, device="cuda:0").iq
        full[torch.from_numpy(idx).to("cuda:0")] = part
        del part
    r = _time_pair(lambda flags: SondeBatch(C, n, types=types, flags=flags), full, max(args.steps // 2, 5), args.reps)
    print(json.dumps(dict(cost="mix RS41/M10/DFM by channel % 3", channels=C, tiles=24, ebn0_db=16.0, **r)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--gpu", action="store_true", help="gain: add the library's own counts with the flag on")
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--tiles", type=int, default=100)
    ap.add_argument("--ebn0", type=float, nargs="+", default=[7.0, 8.0, 9.0, 10.0, 11.0, 12.0])
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.cost or args.gpu:
        import torch
        if not torch.cuda.is_available():
            sys.exit("dfm_rescue_measure: --cost and --gpu need a GPU (there is no CPU path)")
    if args.cost:
        cost(args)
    else:
        gain(args)


if __name__ == "__main__":
    main()
