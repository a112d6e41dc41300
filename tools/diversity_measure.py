#!/usr/bin/env python3
"""What sonde_batch_set_diversity (DESIGN SPEC 3.3j) gains and costs.

    python tools/diversity_measure.py gain [--sondes 32] [--copies 3] [--tiles 300] [--ebn0 7 8 9 10 12] [--engine oracle|gpu]
    python tools/diversity_measure.py cost [--channels 1024] [--tiles 96] [--ebn0 40 9] [--reps 5]

gain: `copies` receivers per sonde at equal Eb/N0, noise independent per receiver (and carrier offset, timing and level: every copy
is modulated on its own), and in every copy the amplitude is cut to zero (the noise stays) for 60 ms once per 1.3 s at a phase of
its own: the fade of a spinning payload as each receiver sees it.  Per Eb/N0 one JSON line: the distinct transmitted frames a group
delivers with selection only (any copy with both codewords decoded), and with combining over the first two and over all copies; the
combined records, and those whose bytes 8..len differ from the transmitted frame (expected: 0).  --engine oracle: the CPU oracle's
records and the Python twin (tests/diversity_reference.py), no GPU; --engine gpu: the library with groups set, four submits.

cost: the framer time (kernel_ms) of an all-RS41 step with set_diversity never called and with channels / 2 pairs set, per Eb/N0.
With SONDE_MI355_LIB pointing at a build of the parent commit only the first figure exists: interleave the two libraries from a
shell loop (tools/ab_repeat.sh does the same for bench.py)."""
import argparse
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
FADE_S, FADE_EVERY_S = 0.060, 1.3


def signals(S, K, n, ebn0, seed, dev, fades=True):
    """[S * K, n, 2] float32 on dev: channel s * K + k is copy k of sonde s; frames[s] = [(bit position, bytes)]"""
    nbits = n // 10 + 16
    bits, frames = synth.rs41_bitstreams(seed, np.arange(S), nbits)
    clean, cfo, tau, amp = synth.gfsk_modulate(np.repeat(bits, K, axis=0), n, 4800.0, seed=seed, ebn0_db=200.0, device=dev)
    rng = np.random.default_rng(seed)
    if fades:
        ln, per = int(FADE_S * 48000), int(FADE_EVERY_S * 48000)
        for c in range(S * K):
            for s0 in range(int(rng.integers(0, per)), n, per):
                clean[c, s0:s0 + ln] = 0.0
    sigma = torch.from_numpy(amp * math.sqrt(10.0 / (2.0 * 10.0 ** (ebn0 / 10.0)))).to(dev).to(torch.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 1)
    for c0 in range(0, S * K, 64):           # in pieces: the noise of 1024 channels at once would double the footprint
        c1 = min(S * K, c0 + 64)
        clean[c0:c1] += sigma[c0:c1, None, None] * torch.randn((c1 - c0, n, 2), generator=g, device=dev, dtype=torch.float32)
    return clean, frames


def gain_point(args, ebn0, seed):
    import diversity_reference as dr
    S, K, n = args.sondes, args.copies, TILE * args.tiles
    gpu = args.engine == "gpu"
    iq, frames = signals(S, K, n, ebn0, seed, "cpu")          # on the CPU for either engine: the same samples, so the counts can be compared
    if gpu:
        iq = iq.to("cuda:0")
    else:
        import oracle_lib
        oracle_lib.build()
        base = oracle_lib.batch_run(0, iq.numpy(), nthreads=args.threads)

    def records(groups):
        if not gpu:
            return dr.diversity(base, groups, None, 960)[0] if groups else base
        from sdrpp_radiosonde_amd.batch import SondeBatch
        b = SondeBatch(S * K, n // 4)
        if groups:
            b.set_diversity(groups)
        parts = []
        for k in range(4):
            b.submit(iq[:, k * (n // 4):(k + 1) * (n // 4)])
            parts.append(b.frames())
        b.close()
        return np.concatenate(parts)

    def count(fr, members):
        got, comb, wrong = set(), 0, []
        for f in fr:
            ch = int(f["channel"])
            s, k = divmod(ch, K)
            if k >= members or int(f["len"]) != 320:
                continue
            d, j = min((abs(int(f["bitpos"]) - p), j) for j, (p, _) in enumerate(frames[s]))
            if d >= 64:
                continue
            if int(f["nerr"][0]) >= 0 and int(f["nerr"][1]) >= 0:
                got.add((s, j))
            if int(f["flags"]) & _lib.FRAME_COMBINED:
                comb += 1
                if not np.array_equal(f["data"][8:320], frames[s][j][1][8:320]):
                    wrong.append((ch, int(f["bitpos"]), [int(v) for v in f["nerr"]]))
        return got, comb, wrong

    res = dict(ebn0_db=ebn0, engine=args.engine, sondes=S, copies=K, samples=n, frames_sent=sum(len(f) for f in frames))
    off = records(None)
    res["one_receiver"] = len(count(off, 1)[0])
    for m in sorted({2, K}):
        on = records([[s * K + k for k in range(m)] for s in range(S)])
        got, comb, wrong = count(on, m)
        res[f"copies_{m}"] = dict(selection=len(count(off, m)[0]), combining=len(got), combined_records=comb, combined_wrong=wrong)
    return res


def cost_point(args, ebn0, seed):
    from sdrpp_radiosonde_amd.batch import SondeBatch
    C, n = args.channels, TILE * args.tiles
    iq, _ = signals(C // 2, 2, n * args.steps, ebn0, seed, "cuda:0", fades=ebn0 < 30)
    res = dict(ebn0_db=ebn0, channels=C, tiles=args.tiles, lib=os.path.basename(_lib.LIB_PATH))
    variants = ["never_called"] + (["pairs_set"] if hasattr(_lib.load(), "sonde_batch_set_diversity") else [])
    ms = {v: [] for v in variants}
    for rep in range(args.reps):             # interleaved: the two variants see the same box in the same minute
        for v in variants:
            b = SondeBatch(C, n)
            if v == "pairs_set":
                b.set_diversity([[2 * s, 2 * s + 1] for s in range(C // 2)])
            b.set_timing(1)
            for _ in range(2):               # the stream twice over: the first pass warms up
                for k in range(args.steps):
                    b.submit(iq[:, k * n:(k + 1) * n])
                b.sync()
                demod, framer = b.kernel_ms()
            ms[v].append((round(demod * 1e3, 1), round(framer * 1e3, 1)))
            if v == "pairs_set" and rep == 0:
                info = [b.diversity_info(g) for g in range(C // 2)]
                res["tried"], res["combined"] = sum(i["tried"] for i in info), sum(i["combined"] for i in info)
            b.close()
    for v in variants:
        res[v] = dict(demod_us=ms[v], framer_us_median=float(np.median([f for _, f in ms[v]])), demod_us_median=float(np.median([d for d, _ in ms[v]])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gain", "cost"])
    ap.add_argument("--sondes", type=int, default=32)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--tiles", type=int, default=None)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ebn0", type=float, nargs="+", default=None)
    ap.add_argument("--engine", choices=["oracle", "gpu"], default="oracle")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=700)
    args = ap.parse_args()
    if args.mode == "gain":
        args.tiles = args.tiles or 300
        for e in args.ebn0 or [7.0, 8.0, 9.0, 10.0, 12.0]:
            print(json.dumps(gain_point(args, e, args.seed)), flush=True)
    else:
        args.tiles = args.tiles or 96
        for e in args.ebn0 or [40.0, 9.0]:
            print(json.dumps(cost_point(args, e, args.seed)), flush=True)


if __name__ == "__main__":
    main()
