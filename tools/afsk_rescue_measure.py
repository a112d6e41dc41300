#!/usr/bin/env python3
"""What SONDE_FLAG_AFSK_RESCUE (DESIGN SPEC 3.3i) gains on noisy iMet and SRS-C50 signals, and what it costs:

    python tools/afsk_rescue_measure.py [--type imet c50] [--snr 4 5 6 7 8] [--channels 16] [--tiles 192] [--seed 5] [--gpu]
    python tools/afsk_rescue_measure.py --cost [--steps 40] [--reps 7]
    python tools/afsk_rescue_measure.py --cost-off --parent-lib PATH [--steps 40] [--reps 5]

Gain (no GPU needed): synth.make_imet_batch / make_c50_batch channels at each SNR through the CPU oracle and the twin
(tests/afsk_rescue_reference.py) over its records; one markdown table row per SNR: packets sent, valid in the first pass (and how
many of those are the transmitted packet), failed records, rescued by one bit and by an adjacent pair (SONDE_FRAME_FLIPS 1 / 2),
"not sent" = rescued packets that differ from the transmitted one, again split by FLIPS, and ambiguous records.  --gpu adds the same
counts from the library with the flag on (its records must equal the twin's).

Cost with the flag on (GPU): submit time (host clock around `steps` submits that end in a synchronise) with the flag off and on, the
two batches alternating `reps` times on the same samples: 512 iMet channels and 512 C50 channels x 24 tiles, each at 6 dB (packets
to rescue) and 20 dB (none); one JSON line each with all values, both medians, their ratio, the difference in microseconds and the
spread of each side.

Cost with the flag off (GPU): the same all-iMet and all-C50 steps, flag off, timed in a FRESH process per run with SONDE_MI355_LIB =
the parent commit's library (built beside this tree), a second copy of the parent's library, and this tree's library, in that order,
`reps` rounds; one JSON line per type with all values, the medians and the spreads.  --cost-child is that child."""
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
TYPES = {"imet": 4, "c50": 5}
COST_CHANNELS, COST_TILES = 512, 24


def _make(kind, C, n, seed, snr_db, **kw):
    return (synth.make_imet_batch if kind == "imet" else synth.make_c50_batch)(C, n, seed=seed, snr_db=snr_db, **kw)


def _tx(frames, f):
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in frames[c]), key=lambda t: t[0])
    return tx if d <= 24 else None


def _count(frames, fr):
    """valid, valid and right, failed, rescued by FLIPS {1, 2}, rescued and NOT the transmitted packet by FLIPS {1, 2}"""
    valid = right = failed = 0
    res, bad = {1: 0, 2: 0}, {1: 0, 2: 0}
    for f in fr:
        tx = _tx(frames, f)
        ok = tx is not None and int(f["len"]) == len(tx) and np.array_equal(f["data"][:len(tx)], tx)
        if int(f["flags"]) & _lib.FRAME_RESCUED:
            w = int(_lib.frame_flips(int(f["flags"])))
            res[w] += 1
            bad[w] += not ok
            failed += 1
        elif int(f["nerr"][0]) == 0:
            valid += 1
            right += ok
        else:
            failed += 1
    return valid, right, failed, res, bad


def gain(args):
    import afsk_rescue_reference as ar
    import oracle_lib
    oracle_lib.build()
    C, n = args.channels, TILE * args.tiles
    for kind in args.type:
        print(f"{kind}, {C} channels x {args.tiles} tiles, seed {args.seed}; CPU oracle and twin"
              + ("; gpu = libsonde_mi355.so with SONDE_FLAG_AFSK_RESCUE" if args.gpu else ""))
        print()
        print("| SNR | sent | valid, first pass (right) | failed records | rescued by 1 bit | rescued by adjacent pair | not sent (1 bit / pair) | "
              "ambiguous | valid with the flag |" + (" gpu valid / rescued 1 / 2 |" if args.gpu else ""))
        print("|---|---|---|---|---|---|---|---|---|" + ("---|" if args.gpu else ""))
        for s in args.snr:
            sb = _make(kind, C, n, args.seed, s)
            iq = sb.iq.numpy()
            fr = oracle_lib.batch_run(TYPES[kind], iq, nthreads=args.threads, cap_per_channel=n // 2048 + 64)
            fr = fr[np.lexsort((fr["bitpos"], fr["channel"]))]
            out, outcomes, _ = ar.rescue(fr)
            valid, right, failed, res, bad = _count(sb.frames, out)
            row = (f"| {s:g} dB | {sum(len(x) for x in sb.frames)} | {valid} ({right}) | {failed} | {res[1]} | {res[2]} | "
                   f"{bad[1] + bad[2]} ({bad[1]} / {bad[2]}) | {outcomes.count('ambiguous')} | {valid + res[1] + res[2]} |")
            if args.gpu:
                import torch
                from sdrpp_radiosonde_amd.batch import SondeBatch
                b = SondeBatch(C, n, types=np.full(C, TYPES[kind], dtype=np.uint8), flags=_lib.FLAG_AFSK_RESCUE)
                b.submit(torch.from_numpy(iq).to("cuda:0"))
                g = b.frames()
                g = g[np.lexsort((g["bitpos"], g["channel"]))]
                b.close()
                gv, _, _, gres, _ = _count(sb.frames, g)
                row += f" {gv} / {gres[1]} / {gres[2]}{'' if g.tobytes() == out.tobytes() else ' RECORDS DIFFER FROM THE TWIN'} |"
            print(row, flush=True)
        print()


def _cost_scene(kind, seed, snr_db):
    return _make(kind, COST_CHANNELS, TILE * COST_TILES, seed, snr_db, device="cuda:0").iq


def _time_pair(make, iq, steps, reps):
    batches = {"off": make(0), "on": make(_lib.FLAG_AFSK_RESCUE)}
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
    out = dict(steps=steps, reps=reps, records_last_submit=int(len(fr)), failed_last_submit=int((fr["nerr"][:, 0] == -1).sum()),
               rescued_last_submit=int((fr["flags"] & _lib.FRAME_RESCUED != 0).sum()),
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
    for kind in args.type:
        types = np.full(COST_CHANNELS, TYPES[kind], dtype=np.uint8)
        for s in (6.0, 20.0):
            iq = _cost_scene(kind, args.seed, s)
            r = _time_pair(lambda flags: SondeBatch(COST_CHANNELS, TILE * COST_TILES, types=types, flags=flags), iq, args.steps, args.reps)
            print(json.dumps(dict(cost=kind, channels=COST_CHANNELS, tiles=COST_TILES, snr_db=s, **r)), flush=True)
            del iq


def cost_child(args):
    """one run, flag off, with whatever library SONDE_MI355_LIB names: ms per step on stdout"""
    from sdrpp_radiosonde_amd.batch import SondeBatch
    kind = args.type[0]
    iq = _cost_scene(kind, args.seed, 6.0)
    b = SondeBatch(COST_CHANNELS, TILE * COST_TILES, types=np.full(COST_CHANNELS, TYPES[kind], dtype=np.uint8), flags=0)
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
        for kind in args.type:
            ms = {k: [] for k, _ in sides}
            records = set()
            for _ in range(args.reps):
                for key, lib in sides:
                    env = dict(os.environ, SONDE_MI355_LIB=os.path.abspath(lib))
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cost-child", "--type", kind, "--steps", str(args.steps),
                                        "--seed", str(args.seed)], env=env, capture_output=True, text=True, timeout=300)
                    if p.returncode != 0:
                        sys.exit(f"afsk_rescue_measure: the {key} run ended with {p.returncode}: {p.stderr[-400:]}")
                    r = json.loads(p.stdout.strip().splitlines()[-1])
                    ms[key].append(round(r["ms"], 4))
                    records.add(r["records"])
            out = dict(cost_off=f"{kind}, flag off", channels=COST_CHANNELS, tiles=COST_TILES, steps=args.steps, reps=args.reps, ms=ms,
                       median={k: round(statistics.median(v), 4) for k, v in ms.items()},
                       spread={k: round(max(v) - min(v), 4) for k, v in ms.items()}, same_record_count=len(records) == 1)
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
    ap.add_argument("--type", nargs="+", choices=sorted(TYPES), default=["imet", "c50"])
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--tiles", type=int, default=192)
    ap.add_argument("--snr", type=float, nargs="+", default=[4.0, 5.0, 6.0, 7.0, 8.0])
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8, help="gain: threads of the CPU oracle")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.cost or args.gpu or args.cost_off or args.cost_child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("afsk_rescue_measure: --cost, --cost-off and --gpu need a GPU (there is no CPU path)")
    if args.cost_off and not args.parent_lib:
        sys.exit("afsk_rescue_measure: --cost-off needs --parent-lib")
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
