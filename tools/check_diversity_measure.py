#!/usr/bin/env python3
"""What sonde_batch_set_diversity gains and costs for M10 / M20 and MRZ-N1 groups (DESIGN SPEC 3.3l).

    python tools/check_diversity_measure.py gain [--kind m10|mrz] [--sondes 16] [--copies 3] [--tiles 150] [--ebn0 8 9 10 11 12 13]
    python tools/check_diversity_measure.py cost [--channels 1024] [--tiles 24] [--ebn0 40 10] [--reps 5] [--rs41-only]

gain: `copies` receivers per sonde at equal Eb/N0, each copy modulated on its own (noise, carrier offset, timing and level are
independent).  Over the CPU oracle's records and the Python twin (tests/check_diversity_reference.py): no GPU.  Per Eb/N0 one JSON line:
the distinct transmitted frames delivered by one receiver, by selection (any copy good) and by the pass, over the first two and over
all copies; the distribution of |V| over the frames the pass tried; and per SONDE_FRAME_UNKNOWNS the combined records and those that
differ from the transmitted frame.

cost: the framer time (kernel_ms) of a step of `channels` M10 channels as channels / 2 pairs with the groups set against the same
batch without groups, per Eb/N0; and the same for an all-RS41 batch (groups never set / pairs set / learn | mark), which is what a
library of the parent commit can run too: with SONDE_MI355_LIB pointing at such a build the M10 variants are left out, and a shell
loop interleaves the two libraries (tools/ab_repeat.sh does the same for bench.py)."""
import argparse
import collections
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sdrpp_radiosonde_amd import _lib, synth                    # noqa: E402

TILE = 2048
KIND = {"m10": (3, False, 101), "m20": (3, True, 70), "mrz": (6, False, 45)}


def signals(kind, S, K, n, ebn0, seed, dev):
    """[S * K, n, 2] float32 on dev: channel s * K + k is copy k of sonde s; frames[s] = [(chip position, bytes)]"""
    typ, m20, ln = KIND[kind]
    baud = synth.SONDE_BAUD[typ]
    chips, frames = synth.chip_streams(typ, seed, np.arange(S), int(n * baud / 48000) + 16, m20=m20)
    frames = [[(p, tx[:ln]) for p, tx in lst] for lst in frames]
    clean, _, _, amp = synth.gfsk_modulate(np.repeat(chips, K, axis=0), n, baud, seed=seed, ebn0_db=200.0, device=dev)
    # Eb/N0 per on-air symbol, as synth.gfsk_modulate's own noise: sigma^2 per component = amp^2 (fs / baud) / (2 Eb/N0)
    sigma = torch.from_numpy(amp * math.sqrt(48000.0 / baud / (2.0 * 10.0 ** (ebn0 / 10.0)))).to(dev).to(torch.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 1)
    for c0 in range(0, S * K, 64):
        c1 = min(S * K, c0 + 64)
        clean[c0:c1] += sigma[c0:c1, None, None] * torch.randn((c1 - c0, n, 2), generator=g, device=dev, dtype=torch.float32)
    return clean, frames


def gain_point(args, ebn0, seed):
    import check_diversity_reference as cr
    import oracle_lib
    oracle_lib.build()
    typ, _, ln = KIND[args.kind]
    S, K, n = args.sondes, args.copies, TILE * args.tiles
    iq, frames = signals(args.kind, S, K, n, ebn0, seed, "cpu")
    base = oracle_lib.batch_run(typ, iq.numpy(), nthreads=args.threads)

    def frame_of(f):
        s = int(f["channel"]) // K
        d, j = min((abs(int(f["bitpos"]) - p), j) for j, (p, _) in enumerate(frames[s]))
        return (s, j) if d < 64 else None

    def good_frames(fr, members):
        return {frame_of(f) for f in fr if int(f["channel"]) % K < members and int(f["len"]) == ln and int(f["nerr"][0]) >= 0} - {None}

    res = dict(kind=args.kind, ebn0_db=ebn0, sondes=S, copies=K, samples=n, frames_sent=sum(len(f) for f in frames),
               one_receiver=len(good_frames(base, 1)))
    for m in sorted({2, K}):
        groups = [[s * K + k for k in range(m)] for s in range(S)]
        v_hist, per_v = collections.Counter(), collections.defaultdict(lambda: [0, 0])
        rule = cr.combine

        def counting(copies, n_copies=None):            # |V| of every frame the pass tries, from the copies it is given
            v_hist[min(len(cr.working_frame(list(copies))[1]), 16)] += 1
            return rule(copies, n_copies)
        cr.combine = counting
        try:
            out, outcomes, state = cr.diversity(base, groups, None, 960)
        finally:
            cr.combine = rule
        for i, o in enumerate(outcomes):
            if o == "combined":
                w = frame_of(out[i])
                u = cr.unknowns(out[i]["flags"])
                per_v[u][0] += 1
                per_v[u][1] += w is None or bytes(out[i]["data"][:ln]) != bytes(frames[w[0]][w[1]][1])
        wrong_frames = {frame_of(f) for f in out if int(f["flags"]) & 4 and (frame_of(f) is None or bytes(f["data"][:ln]) != bytes(frames[frame_of(f)[0]][frame_of(f)[1]][1]))}
        res[f"copies_{m}"] = dict(selection=len(good_frames(base, m)), with_the_pass=len(good_frames(out, m) - wrong_frames),
                                  tried=sum(state["tried"]), combined=sum(state["combined"]),
                                  unknowns_of_tried={str(k) if k < 16 else "16+": v for k, v in sorted(v_hist.items())},
                                  combined_and_wrong_by_unknowns={str(k): v for k, v in sorted(per_v.items())})
    return res


def rs41_signals(S, n, ebn0, seed, dev):
    bits, _ = synth.rs41_bitstreams(seed, np.arange(S), n // 10 + 16)
    iq, *_ = synth.gfsk_modulate(np.repeat(bits, 2, axis=0), n, 4800.0, seed=seed, ebn0_db=ebn0, device=dev)
    return iq


def cost_point(args, ebn0, seed):
    from sdrpp_radiosonde_amd.batch import SondeBatch
    C, n = args.channels, TILE * args.tiles
    new_lib = hasattr(_lib.load(), "sonde_batch_test_check_combine")
    res = dict(ebn0_db=ebn0, channels=C, tiles=args.tiles, lib=os.path.basename(_lib.LIB_PATH), has_check_groups=new_lib)
    pairs = [[2 * s, 2 * s + 1] for s in range(C // 2)]
    data = {"rs41": (rs41_signals(C // 2, n * args.steps, ebn0, seed, "cuda:0"), np.zeros(C, dtype=np.uint8))}
    variants = [("rs41", "never_called"), ("rs41", "pairs_set"), ("rs41", "learn_mark")]
    if new_lib and not args.rs41_only:
        data["m10"] = (signals("m10", C // 2, 2, n * args.steps, ebn0, seed, "cuda:0")[0], np.full(C, 3, dtype=np.uint8))
        variants += [("m10", "never_called"), ("m10", "pairs_set"), ("m10", "learn_mark")]
    ms = {v: [] for v in variants}
    for rep in range(args.reps):             # interleaved: the variants see the same machine in the same minute
        for v in variants:
            iq, types = data[v[0]]
            b = SondeBatch(C, n, types=types)
            if v[1] == "pairs_set":
                b.set_diversity(pairs)
            if v[1] == "learn_mark":         # offsets given (zeros, locked from the start): the combining pass does the same work
                b.set_diversity(pairs, np.zeros(C, dtype=np.int64), 0, learn=True, mark_duplicates=True)
            b.set_timing(1)
            for _ in range(2):               # the stream twice over: the first pass warms up
                for k in range(args.steps):
                    b.submit(iq[:, k * n:(k + 1) * n])
                b.sync()
                demod, framer = b.kernel_ms()
            ms[v].append(round(framer * 1e3, 1))
            if v[1] == "pairs_set" and rep == 0:
                info = [b.diversity_info(g) for g in range(C // 2)]
                res[f"{v[0]}_tried"], res[f"{v[0]}_combined"] = sum(i["tried"] for i in info), sum(i["combined"] for i in info)
            b.close()
    for v in variants:
        res["_".join(v)] = dict(framer_us=ms[v], framer_us_median=float(np.median(ms[v])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gain", "cost"])
    ap.add_argument("--kind", choices=list(KIND), default="m10")
    ap.add_argument("--sondes", type=int, default=16)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--tiles", type=int, default=None)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rs41-only", action="store_true")         # cost: the variants a library of the parent commit has too
    ap.add_argument("--ebn0", type=float, nargs="+", default=None)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=900)
    args = ap.parse_args()
    if args.mode == "gain":
        args.tiles = args.tiles or (150 if args.kind != "mrz" else 400)
        for e in args.ebn0 or [8.0, 9.0, 10.0, 11.0, 12.0, 13.0]:
            print(json.dumps(gain_point(args, e, args.seed)), flush=True)
    else:
        args.tiles = args.tiles or 24          # 24 tiles = 1.024 s per submit
        for e in args.ebn0 or [40.0, 10.0]:
            print(json.dumps(cost_point(args, e, args.seed)), flush=True)


if __name__ == "__main__":
    main()
