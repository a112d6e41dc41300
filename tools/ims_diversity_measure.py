#!/usr/bin/env python3
"""What sonde_batch_set_diversity gains and costs for iMS-100 groups (SONDE_FLAG_IMS_DIVERSITY, DESIGN SPEC 3.3n).  Results:
profiles/ims_diversity_notes.md.

    python tools/ims_diversity_measure.py gain [--sondes 16] [--copies 3] [--tiles 100] [--ebn0 8 8.5 9 9.5 10 10.5] [--fade-ms 0]
    python tools/ims_diversity_measure.py cost [--channels 1024] [--tiles 24] [--ebn0 40 9] [--reps 10]

gain: `copies` receivers per sonde at equal Eb/N0, each copy modulated on its own (noise, carrier offset, timing and level are
independent); with --fade-ms F every copy also loses F ms of signal every 1.3 s at a phase of its own (tools/diversity_measure.py's
fade, shorter: an iMS-100 frame lasts 240 ms).  Over the CPU oracle's records and chips and the Python twin
(tests/ims_diversity_reference.py): no GPU.  Per Eb/N0 one JSON line: the distinct transmitted frames delivered valid (nerr[1] == 0) by one receiver, by selection (any copy
valid) and by the pass, over the first two and over all copies; the combined records and those that are NOT the transmitted frame, in
all and per SONDE_FRAME_JOINT; and the same share among the first pass's own valid records (its miscorrections).

cost: the time behind the demodulators (kernel_ms' second figure: the align step and the pass; zero where nothing is launched there) and
the whole step (both figures) of a step of `channels` iMS-100 channels as channels / 2 pairs: created without the flag / with the
flag and groups never set / pairs set / pairs set with learn | mark (offsets given, locked from the start), per Eb/N0, interleaved.  A
library of the parent commit (SONDE_MI355_LIB) refuses iMS-100 groups: there only no_flag runs, which is the figure the others are
held against (nothing is launched for it in either)."""
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
IMS = 2
FADE_EVERY_S = 1.3


def signals(S, K, n, ebn0, seed, dev, fade_ms=0.0):
    """[S * K, n, 2] float32 on dev: channel s * K + k is copy k of sonde s; frames[s] = [(chip position, data bytes)]"""
    baud = synth.SONDE_BAUD[IMS]
    chips, frames = synth.chip_streams(IMS, seed, np.arange(S), int(n * baud / 48000) + 16)
    frames = [[(p, tx[:51]) for p, tx in lst] for lst in frames]
    clean, _, _, amp = synth.gfsk_modulate(np.repeat(chips, K, axis=0), n, baud, seed=seed, ebn0_db=200.0, device=dev)
    if fade_ms > 0:
        rng = np.random.default_rng(seed)
        ln, per = int(fade_ms * 48.0), int(FADE_EVERY_S * 48000)
        for c in range(S * K):
            for s0 in range(int(rng.integers(0, per)), n, per):
                clean[c, s0:s0 + ln] = 0.0
    # Eb/N0 per on-air symbol, as synth.gfsk_modulate's own noise: sigma^2 per component = amp^2 (fs / baud) / (2 Eb/N0)
    sigma = torch.from_numpy(amp * math.sqrt(48000.0 / baud / (2.0 * 10.0 ** (ebn0 / 10.0)))).to(dev).to(torch.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 1)
    for c0 in range(0, S * K, 64):
        c1 = min(S * K, c0 + 64)
        clean[c0:c1] += sigma[c0:c1, None, None] * torch.randn((c1 - c0, n, 2), generator=g, device=dev, dtype=torch.float32)
    return clean, frames


def gain_point(args, ebn0, seed):
    import ims_diversity_reference as cr
    import ims_rescue_reference as ir
    import oracle_lib
    oracle_lib.build()
    S, K, n = args.sondes, args.copies, TILE * args.tiles
    iq, frames = signals(S, K, n, ebn0, seed, "cpu", args.fade_ms)
    recs, streams = [], []
    for c in range(S * K):                   # channel by channel: the twin needs each channel's chips next to its records
        ch = oracle_lib.Channel(IMS, c)
        ch.feed(iq[c].numpy())
        recs.append(ch.frames())
        streams.append(ch.bits())
    base = np.concatenate(recs)
    chips = ir.chips_of_streams(streams)

    def frame_of(f):
        s = int(f["channel"]) // K
        d, j = min((abs(int(f["bitpos"]) - p), j) for j, (p, _) in enumerate(frames[s]))
        return (s, j) if d < 64 else None

    def wrong(f):
        w = frame_of(f)
        return w is None or bytes(f["data"][:51]) != bytes(frames[w[0]][w[1]][1])

    def valid(fr, members):
        return [f for f in fr if int(f["channel"]) % K < members and int(f["len"]) == 51 and int(f["nerr"][1]) == 0]

    def delivered(fr, members):
        return {frame_of(f) for f in valid(fr, members) if not wrong(f)}

    first = valid(base, K)
    res = dict(ebn0_db=ebn0, fade_ms=args.fade_ms, sondes=S, copies=K, samples=n, frames_sent=sum(len(f) for f in frames),
               one_receiver=len(delivered(base, 1)), first_pass_valid=len(first), first_pass_valid_and_wrong=sum(1 for f in first if wrong(f)))
    for m in sorted({2, K}):
        groups = [[s * K + k for k in range(m)] for s in range(S)]
        out, outcomes, state = cr.diversity(base, groups, chips, None, cr.WINDOW)
        per_j = collections.defaultdict(lambda: [0, 0])
        for i, o in enumerate(outcomes):
            if o == "combined":
                j = cr.joint(out[i]["flags"])
                per_j[j][0] += 1
                per_j[j][1] += wrong(out[i])
        res[f"copies_{m}"] = dict(selection=len(delivered(base, m)), with_the_pass=len(delivered(out, m)), tried=sum(state["tried"]),
                                  combined=sum(state["combined"]), combined_and_wrong=sum(v[1] for v in per_j.values()),
                                  outcomes=dict(collections.Counter(o for o in outcomes if o in ("guard", "none", "several", "left_out"))),
                                  combined_and_wrong_by_joint={str(k): v for k, v in sorted(per_j.items())})
    return res


def cost_point(args, ebn0, seed):
    from sdrpp_radiosonde_amd.batch import SondeBatch
    C, n = args.channels, TILE * args.tiles
    new_lib = hasattr(_lib.load(), "sonde_batch_test_ims_combine")
    res = dict(ebn0_db=ebn0, channels=C, tiles=args.tiles, steps=args.steps, lib=_lib.LIB_PATH, has_ims_groups=new_lib)
    pairs = [[2 * s, 2 * s + 1] for s in range(C // 2)]
    iq = signals(C // 2, 2, n * args.steps, ebn0, seed, "cuda:0")[0]
    types = np.full(C, IMS, dtype=np.uint8)
    variants = ["no_flag"] + (["never_called", "pairs_set", "learn_mark"] if new_lib else [])
    ms, whole = {v: [] for v in variants}, {v: [] for v in variants}
    for rep in range(args.reps):             # interleaved: the variants see the same machine in the same minute
        for v in variants:
            b = SondeBatch(C, n, types=types, flags=0 if v == "no_flag" else _lib.FLAG_IMS_DIVERSITY)
            if v == "pairs_set":
                b.set_diversity(pairs)
            if v == "learn_mark":            # offsets given (zeros, locked from the start): the combining pass does the same work
                b.set_diversity(pairs, np.zeros(C, dtype=np.int64), 0, learn=True, mark_duplicates=True)
            b.set_timing(1)
            for _ in range(2):               # the stream twice over: the first pass warms up
                for k in range(args.steps):
                    b.submit(iq[:, k * n:(k + 1) * n])
                b.sync()
                demod, framer = b.kernel_ms()
            ms[v].append(round(framer * 1e3, 1))
            whole[v].append(round((demod + framer) * 1e3, 1))
            if v == "pairs_set" and rep == 0:
                info = [b.diversity_info(g) for g in range(C // 2)]
                res["tried"], res["combined"] = sum(i["tried"] for i in info), sum(i["combined"] for i in info)
            b.close()
    for v in variants:
        res[v] = dict(framer_us=ms[v], framer_us_median=float(np.median(ms[v])), framer_us_min=min(ms[v]), framer_us_max=max(ms[v]),
                      step_us=whole[v], step_us_median=float(np.median(whole[v])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gain", "cost"])
    ap.add_argument("--sondes", type=int, default=16)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--tiles", type=int, default=None)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fade-ms", type=float, default=0.0)
    ap.add_argument("--ebn0", type=float, nargs="+", default=None)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=900)
    args = ap.parse_args()
    if args.mode == "gain":
        args.tiles = args.tiles or 100
        for e in args.ebn0 or [8.0, 8.5, 9.0, 9.5, 10.0, 10.5]:
            print(json.dumps(gain_point(args, e, args.seed)), flush=True)
    else:
        args.tiles = args.tiles or 24          # 24 tiles = 1.024 s per submit
        for e in args.ebn0 or [40.0, 9.0]:
            print(json.dumps(cost_point(args, e, args.seed)), flush=True)


if __name__ == "__main__":
    main()
