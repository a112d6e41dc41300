#!/usr/bin/env python3
"""What sonde_batch_set_diversity gains and costs for iMet and SRS-C50 groups (SONDE_FLAG_AFSK_DIVERSITY, DESIGN SPEC 3.3o).  Results:
profiles/afsk_diversity_notes.md.

    python tools/afsk_diversity_measure.py gain [--kind imet|c50] [--sondes 16] [--copies 3] [--tiles 288] [--cn 4 5 6 7 8] [--md FILE]
    python tools/afsk_diversity_measure.py cost [--kind imet|c50] [--channels 1024] [--granules 2] [--cn 40 6] [--reps 10]

gain: `copies` receivers per sonde at equal C/N, each copy modulated on its own (noise, carrier offset, timing and level are
independent).  Over the CPU oracle's records and the Python twin (tests/afsk_diversity_reference.py): no GPU.  Per C/N one JSON line:
the distinct transmitted packets delivered by one receiver, by selection (any copy good) and by the pass, over the first two and over
all copies; the first pass's own valid records and those of them that are not the transmitted packet; and per SONDE_FRAME_UNKNOWNS
the combined records and those that are not the transmitted packet.  --md appends the tables to a markdown file.

cost: the framer time (kernel_ms) of a step of `channels` channels as channels / 2 pairs with the groups set, and with the align
step as well (iMet), against the same batch without groups -- which is all a library of the parent commit launches there --, per
C/N, `reps` runs each, interleaved."""
import argparse
import collections
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sdrpp_radiosonde_amd import _lib, synth                    # noqa: E402

TILE, GRANULE = 2048, 16384
KIND = {"imet": 4, "c50": 5}


def signals(kind, S, K, n, cn, seed, dev):
    """[S * K, n, 2] float32 on dev: channel s * K + k is copy k of sonde s; frames[s] = [(symbol position, packet bytes)]"""
    if kind == "c50":
        bits, frames = synth.c50_bitstreams(seed, np.arange(S), int(n * synth.C50_BAUD / 48000) + 16)
        kw = dict(baud=synth.C50_BAUD, mark_hz=synth.C50_MARK_HZ, space_hz=synth.C50_SPACE_HZ, fm_dev_hz=4000.0)
    else:
        bits, frames = synth.imet_bitstreams(seed, np.arange(S), int(n * synth.IMET_BAUD / 48000) + 16, xdata=True)
        kw = {}
    iq = synth.afsk_modulate(np.repeat(bits, K, axis=0), n, seed=seed, snr_db=cn, device=dev, **kw)[0]
    return iq, frames


def gain_point(args, cn, seed):
    import afsk_diversity_reference as ad
    import check_diversity_reference as cr
    import oracle_lib
    oracle_lib.build()
    typ = KIND[args.kind]
    S, K, n = args.sondes, args.copies, TILE * args.tiles
    iq, frames = signals(args.kind, S, K, n, cn, seed, "cpu")
    base = oracle_lib.batch_run(typ, iq.numpy(), nthreads=args.threads, cap_per_channel=n // 2048 + 64)
    base = base[np.lexsort((base["bitpos"], base["channel"]))]

    def sent(f):
        """(sonde, packet) whose transmitted bytes the record holds; None: it holds no transmitted packet"""
        s = int(f["channel"]) // K
        d, j = min((abs(int(f["bitpos"]) - p), j) for j, (p, _) in enumerate(frames[s]))
        tx = frames[s][j][1]
        return (s, j) if d <= 24 and int(f["len"]) == len(tx) and bytes(f["data"][:len(tx)]) == bytes(tx) else None

    def delivered(fr, members):
        return {sent(f) for f in fr if int(f["channel"]) % K < members and int(f["nerr"][0]) >= 0} - {None}

    valid = base[base["nerr"][:, 0] >= 0]
    res = dict(kind=args.kind, cn_db=cn, sondes=S, copies=K, samples=n, packets_sent=sum(len(f) for f in frames),
               one_receiver=len(delivered(base, 1)), first_pass_valid=len(valid), first_pass_valid_and_wrong=sum(1 for f in valid if sent(f) is None))
    for m in sorted({2, K}):
        groups = [[s * K + k for k in range(m)] for s in range(S)]
        v_hist, per_v = collections.Counter(), collections.defaultdict(lambda: [0, 0])
        rule = ad.combine

        def counting(copies, n_copies=None):            # |V| of every packet the pass tries, from the copies it is given
            v_hist[min(len(cr.working_frame(list(copies))[1]), 16)] += 1
            return rule(copies, n_copies)
        ad.combine = counting
        try:
            out, outcomes, state = ad.diversity(base, groups, None, 0)
        finally:
            ad.combine = rule
        for i, o in enumerate(outcomes):
            if o == "combined":
                u = ad.unknowns(out[i]["flags"])
                per_v[u][0] += 1
                per_v[u][1] += sent(out[i]) is None
        res[f"copies_{m}"] = dict(selection=len(delivered(base, m)), with_the_pass=len(delivered(out, m)),
                                  tried=sum(state["tried"]), combined=sum(state["combined"]),
                                  unknowns_of_tried={str(k) if k < 16 else "16+": v for k, v in sorted(v_hist.items())},
                                  combined_and_wrong_by_unknowns={str(k): v for k, v in sorted(per_v.items())})
    return res


def gain_md(rows, path):
    kind = rows[0]["kind"]
    with open(path, "a") as f:
        f.write(f"\n### {kind}: {rows[0]['sondes']} sondes, {rows[0]['samples'] / 48000:.1f} s, {rows[0]['packets_sent']} packets sent\n\n")
        f.write("| C/N dB | one receiver | better of 2 | pass, 2 | better of 3 | pass, 3 | first pass valid / wrong | combined / wrong (2) | combined / wrong (3) |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            c2, c3 = r["copies_2"], r.get("copies_3", r["copies_2"])
            cw = lambda c: "%d / %d" % tuple(map(sum, zip(*c["combined_and_wrong_by_unknowns"].values()))) if c["combined_and_wrong_by_unknowns"] else "0 / 0"      # noqa: E731
            f.write(f"| {r['cn_db']:g} | {r['one_receiver']} | {c2['selection']} | {c2['with_the_pass']} | {c3['selection']} | {c3['with_the_pass']} | "
                    f"{r['first_pass_valid']} / {r['first_pass_valid_and_wrong']} | {cw(c2)} | {cw(c3)} |\n")
        f.write("\ncombined / wrong per SONDE_FRAME_UNKNOWNS, all C/N together:\n\n| copies | " + " | ".join(str(u) for u in range(1, 13)) + " |\n|---|" + "---|" * 12 + "\n")
        for m in (2, 3):
            tot = collections.defaultdict(lambda: [0, 0])
            for r in rows:
                for u, (c, w) in r.get(f"copies_{m}", {}).get("combined_and_wrong_by_unknowns", {}).items():
                    tot[int(u)][0] += c
                    tot[int(u)][1] += w
            f.write(f"| {m} | " + " | ".join("%d / %d" % tuple(tot[u]) for u in range(1, 13)) + " |\n")


def cost_point(args, cn, seed):
    import torch
    from sdrpp_radiosonde_amd.batch import SondeBatch
    C, n = args.channels, GRANULE * args.granules
    res = dict(kind=args.kind, cn_db=cn, channels=C, samples_per_step=n, lib=os.path.basename(_lib.LIB_PATH))
    pairs = [[2 * s, 2 * s + 1] for s in range(C // 2)]
    # 16 sondes' worth of signal, repeated over the pairs: the cost depends on the records, not on whose they are
    S = 16
    iq16, _ = signals(args.kind, S, 2, n * args.steps, cn, seed, "cuda:0")
    iq = iq16.repeat(C // (2 * S), 1, 1).contiguous()
    types = np.full(C, KIND[args.kind], dtype=np.uint8)
    variants = ["never_called", "pairs_set"] + (["learn_mark"] if args.kind == "imet" else [])
    ms = {v: [] for v in variants}
    for rep in range(args.reps):             # interleaved: the variants see the same machine in the same minute
        for v in variants:
            b = SondeBatch(C, n, types=types, flags=_lib.FLAG_AFSK_DIVERSITY)
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
            if v == "pairs_set" and rep == 0:
                info = [b.diversity_info(g) for g in range(C // 2)]
                res["tried"], res["combined"] = sum(i["tried"] for i in info), sum(i["combined"] for i in info)
            b.close()
    torch.cuda.synchronize()
    for v in variants:
        res[v] = dict(framer_us=ms[v], median=float(np.median(ms[v])), min=min(ms[v]), max=max(ms[v]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gain", "cost"])
    ap.add_argument("--kind", choices=list(KIND), default="imet")
    ap.add_argument("--sondes", type=int, default=16)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--tiles", type=int, default=288)
    ap.add_argument("--granules", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cn", type=float, nargs="+", default=None)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--seed", type=int, default=900)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.mode == "gain":
        rows = []
        for e in args.cn or [4.0, 5.0, 6.0, 7.0, 8.0]:
            rows.append(gain_point(args, e, args.seed))
            print(json.dumps(rows[-1]), flush=True)
        if args.md:
            gain_md(rows, args.md)
    else:
        for e in args.cn or [40.0, 6.0]:
            print(json.dumps(cost_point(args, e, args.seed)), flush=True)


if __name__ == "__main__":
    main()
