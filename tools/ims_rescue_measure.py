#!/usr/bin/env python3
"""What SONDE_FLAG_IMS_RESCUE (DESIGN SPEC 3.3h) gains on noisy iMS-100 signals, and what it costs:

    python tools/ims_rescue_measure.py [--ebn0 8 8.5 9 9.5 10 10.5 11] [--channels 8] [--tiles 100] [--seed 5] [--gpu]
    python tools/ims_rescue_measure.py --cost [--steps 40] [--reps 7]
    python tools/ims_rescue_measure.py --cost-off --parent-lib PATH [--steps 40] [--reps 5]

Gain (no GPU needed): synth.make_batch iMS-100 channels at each Eb/N0 through the CPU oracle and the twin
(tests/ims_rescue_reference.py) over its records and chips; one markdown table row per Eb/N0: records on a transmitted frame, valid as
recorded (nerr[1] == 0) and how many of those are the transmitted frame, failed, rescued, rescued and right, the share of wrong frames
among the rescued and among the first pass's own valid frames.  A second table breaks the rescued frames and the wrong ones among
them down by SONDE_FRAME_BLOCKS and by the largest number m of violated boundaries among the frame's decoded blocks.  --gpu adds the
same counts from the library with the flag on (they must equal the twin's).

Cost with the flag on (GPU): submit time (host clock around `steps` submits that end in a synchronise) with the flag off and on, the
two batches alternating `reps` times on the same samples: 1024 iMS-100 channels x 24 tiles at Eb/N0 9.5 dB (frames to rescue) and
16 dB (none); one JSON line each with all values, both medians, their ratio, the difference in microseconds and the spread of each side.

Cost with the flag off (GPU): the same all-iMS-100 step, flag off, timed in a FRESH process per run with SONDE_MI355_LIB = the parent
commit's library (built beside this tree), a second copy of the parent's library, and this tree's library, in that order, `reps`
rounds (the scheme of tools/ab_repeat.sh with the copy added to show the parent's own spread); one JSON line with all values, the
medians and the spreads.  --cost-child is that child."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sdrpp_radiosonde_amd import _lib, synth                    # noqa: E402

TILE = 2048
IMS = 2
COST_CHANNELS, COST_TILES = 1024, 24


def _tx(frames, f):
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in frames[c]), key=lambda t: t[0])
    return tx if d < 64 else None


def _count(frames, fr):
    """(records on a transmitted frame, valid, valid and right, rescued, rescued and right)"""
    on = valid = right = res = res_right = 0
    for f in fr:
        tx = _tx(frames, f)
        ok = tx is not None and np.array_equal(f["data"][:51], tx)
        on += tx is not None
        if int(f["nerr"][1]) == 0 and tx is not None:
            if int(f["flags"]) & _lib.FRAME_RESCUED:
                res += 1
                res_right += ok
            else:
                valid += 1
                right += ok
    return on, valid, right, res, res_right


def _breakdown(ir, frames, before, after, get, by_blocks, by_m):
    """rescued frames and the wrong ones among them by SONDE_FRAME_BLOCKS and by the largest m of the frame's decoded blocks"""
    for f0, f in zip(before, after):
        if not int(f["flags"]) & _lib.FRAME_RESCUED:
            continue
        tx = _tx(frames, f)
        wrong = int(tx is None or not np.array_equal(f["data"][:51], tx))
        fc = get(int(f["channel"]), int(f["bitpos"]), ir.FRAME_CHIPS)
        blocks = ir.received_blocks(fc)
        m = max(len(ir.violations(fc, L)) for L in range(ir.NBLK) if ir.first_pass_rejects(blocks[L]))
        for table, key in ((by_blocks, int(_lib.frame_blocks(f["flags"]))), (by_m, m)):
            n, w = table.get(key, (0, 0))
            table[key] = (n + 1, w + wrong)


def gain(args):
    import ims_rescue_reference as ir
    import oracle_lib
    oracle_lib.build()
    C, n = args.channels, TILE * args.tiles
    print(f"iMS-100, {C} channels x {args.tiles} tiles, synth.make_batch seed {args.seed}; CPU oracle and twin"
          + ("; gpu = libsonde_mi355.so with SONDE_FLAG_IMS_RESCUE" if args.gpu else ""))
    print()
    print("| Eb/N0 | records on a transmitted frame | valid today (right) | failed | rescued | rescued and right | wrong among rescued | "
          "wrong among first-pass valid |" + (" gpu valid / rescued (right) |" if args.gpu else ""))
    print("|---|---|---|---|---|---|---|---|" + ("---|" if args.gpu else ""))
    by_blocks, by_m = {}, {}
    for e in args.ebn0:
        sb = synth.make_batch(IMS, C, n, seed=args.seed, ebn0_db=e)
        iq = sb.iq.numpy()
        recs, streams = [], []
        for c in range(C):
            ch = oracle_lib.Channel(IMS, c)
            ch.feed(iq[c])
            recs.append(ch.frames())
            streams.append(ch.bits())
        fr = np.concatenate(recs)
        get = ir.chips_of_streams(streams)
        out, outcomes, _ = ir.rescue(fr, get)
        _breakdown(ir, sb.frames, fr, out, get, by_blocks, by_m)
        on, valid, right, res, res_right = _count(sb.frames, out)
        share = lambda bad, tot: f"{bad}/{tot}" + (f" = {100.0 * bad / tot:.1f} %" if tot else "")      # noqa: E731
        row = (f"| {e:g} dB | {on} | {valid} ({right}) | {on - valid} | {res} | {res_right} | {share(res - res_right, res)} | "
               f"{share(valid - right, valid)} |")
        if args.gpu:
            import torch
            from sdrpp_radiosonde_amd.batch import SondeBatch
            b = SondeBatch(C, n, types=np.full(C, IMS, dtype=np.uint8), flags=_lib.FLAG_IMS_RESCUE)
            b.submit(torch.from_numpy(iq).to("cuda:0"))
            g = b.frames()
            b.close()
            _, gv, gr, gres, gres_right = _count(sb.frames, g)
            row += f" {gv} / {gres} ({gres_right}){'' if g.tobytes() == out.tobytes() else ' RECORDS DIFFER FROM THE TWIN'} |"
        print(row, flush=True)
    print()
    print("| rescued frames over the whole sweep | " + " | ".join(f"{k} block{'s' * (k > 1)}" for k in sorted(by_blocks)) + " | "
          + " | ".join(f"largest m = {k}" for k in sorted(by_m)) + " |")
    print("|---|" + "---|" * (len(by_blocks) + len(by_m)))
    print("| rescued | " + " | ".join(str(by_blocks[k][0]) for k in sorted(by_blocks)) + " | " + " | ".join(str(by_m[k][0]) for k in sorted(by_m)) + " |")
    print("| of them not the transmitted frame | " + " | ".join(str(by_blocks[k][1]) for k in sorted(by_blocks)) + " | "
          + " | ".join(str(by_m[k][1]) for k in sorted(by_m)) + " |")


def _cost_scene(seed, ebn0_db):
    return synth.make_batch(IMS, COST_CHANNELS, TILE * COST_TILES, seed=seed, ebn0_db=ebn0_db, device="cuda:0").iq


def _time_pair(make, iq, steps, reps):
    batches = {"off": make(0), "on": make(_lib.FLAG_IMS_RESCUE)}
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
               ims_failed_last_submit=int(((fr["type"] == IMS) & (fr["nerr"][:, 1] != 0)).sum()),
               ims_rescued_last_submit=int(((fr["type"] == IMS) & (fr["flags"] & _lib.FRAME_RESCUED != 0)).sum()),
               ms_off=[round(v, 4) for v in ms["off"]], ms_on=[round(v, 4) for v in ms["on"]],
               median_off=round(statistics.median(ms["off"]), 4), median_on=round(statistics.median(ms["on"]), 4),
               spread_off=round(max(ms["off"]) - min(ms["off"]), 4), spread_on=round(max(ms["on"]) - min(ms["on"]), 4))
    out["on_over_off"] = round(out["median_on"] / out["median_off"], 4)
    out["added_us"] = round((out["median_on"] - out["median_off"]) * 1e3, 2)
    for b in batches.values():
        b.close()
    return out


def cost(args):
    from sdrpp_radiosonde_amd.batch import SondeBatch
    types = np.full(COST_CHANNELS, IMS, dtype=np.uint8)
    for e in (9.5, 16.0):
        iq = _cost_scene(args.seed, e)
        r = _time_pair(lambda flags: SondeBatch(COST_CHANNELS, TILE * COST_TILES, types=types, flags=flags), iq, args.steps, args.reps)
        print(json.dumps(dict(cost="iMS-100", channels=COST_CHANNELS, tiles=COST_TILES, ebn0_db=e, **r)), flush=True)
        del iq


def cost_child(args):
    """one run, flag off, with whatever library SONDE_MI355_LIB names: ms per step on stdout"""
    from sdrpp_radiosonde_amd.batch import SondeBatch
    iq = _cost_scene(args.seed, 9.5)
    b = SondeBatch(COST_CHANNELS, TILE * COST_TILES, types=np.full(COST_CHANNELS, IMS, dtype=np.uint8), flags=0)
    b.set_timing(0)
    for _ in range(10):
        b.submit(iq)
    b.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        b.submit(iq)
    b.sync()
    print(json.dumps(dict(ms=(time.perf_counter() - t0) * 1e3 / args.steps, records=int(len(b.frames())))), flush=True)
    b.close()


def cost_off(args):
    new = _lib.LIB_PATH
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "libsonde_parent_copy.so")
        shutil.copy(args.parent_lib, copy)
        sides = (("parent", args.parent_lib), ("parent_copy", copy), ("new_flag_off", new))
        ms = {k: [] for k, _ in sides}
        records = set()
        for _ in range(args.reps):
            for key, lib in sides:
                env = dict(os.environ, SONDE_MI355_LIB=os.path.abspath(lib))
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cost-child", "--steps", str(args.steps), "--seed", str(args.seed)],
                                   env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    sys.exit(f"ims_rescue_measure: the {key} run ended with {p.returncode}: {p.stderr[-400:]}")
                r = json.loads(p.stdout.strip().splitlines()[-1])
                ms[key].append(round(r["ms"], 4))
                records.add(r["records"])
    out = dict(cost_off="iMS-100, flag off", channels=COST_CHANNELS, tiles=COST_TILES, steps=args.steps, reps=args.reps, ms=ms,
               median={k: round(statistics.median(v), 4) for k, v in ms.items()}, spread={k: round(max(v) - min(v), 4) for k, v in ms.items()},
               same_record_count=len(records) == 1)
    out["new_over_parent"] = round(out["median"]["new_flag_off"] / out["median"]["parent"], 4)
    out["copy_over_parent"] = round(out["median"]["parent_copy"] / out["median"]["parent"], 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--cost-off", action="store_true")
    ap.add_argument("--cost-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", help="--cost-off: the parent commit's libsonde_mi355.so")
    ap.add_argument("--gpu", action="store_true", help="gain: add the library's own counts with the flag on")
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--tiles", type=int, default=100)
    ap.add_argument("--ebn0", type=float, nargs="+", default=[8.0, 8.5, 9.0, 9.5, 10.0, 10.5, 11.0])
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.cost or args.gpu or args.cost_off or args.cost_child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("ims_rescue_measure: --cost, --cost-off and --gpu need a GPU (there is no CPU path)")
    if args.cost_off and not args.parent_lib:
        sys.exit("ims_rescue_measure: --cost-off needs --parent-lib")
    if args.cost_child:
        cost_child(args)
    elif args.cost_off:
        cost_off(args)
    elif args.cost:
        cost(args)
    else:
        gain(args)


if __name__ == "__main__":
    main()
