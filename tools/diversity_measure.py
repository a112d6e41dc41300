#!/usr/bin/env python3
"""What sonde_batch_set_diversity (DESIGN SPEC 3.3j) and its learned mode (sonde_batch_set_diversity_auto, SPEC 3.3k) gain and cost.

    python tools/diversity_measure.py gain [--sondes 32] [--copies 3] [--tiles 300] [--ebn0 7 8 9 10 12] [--engine oracle|gpu]
    python tools/diversity_measure.py learn [--sondes 32] [--copies 2] [--tiles 300] [--ebn0 9 10 14] [--cuts 10] [--engine oracle|gpu]
    python tools/diversity_measure.py cost [--channels 1024] [--tiles 96] [--ebn0 40 9] [--reps 5]

gain: `copies` receivers per sonde at equal Eb/N0, noise independent per receiver (and carrier offset, timing and level: every copy
is modulated on its own), and in every copy the amplitude is cut to zero (the noise stays) for 60 ms once per 1.3 s at a phase of
its own: the fade of a spinning payload as each receiver sees it.  Per Eb/N0 one JSON line: the distinct transmitted frames a group
delivers with selection only (any copy with both codewords decoded), and with combining over the first two and over all copies; the
combined records, and those whose bytes 8..len differ from the transmitted frame (expected: 0).  --engine oracle: the CPU oracle's
records and the Python twin (tests/diversity_reference.py), no GPU; --engine gpu: the library with groups set, four submits.

learn: the same signals, but every copy after the first starts at a random time of its own, up to --max-delay bits late, which
nobody tells the library.  Per Eb/N0 one JSON line: the distinct frames delivered in `cuts` submits with the true offsets given
(mode 0) and with learn | mark_duplicates and no offsets, the frames the second run lost before its group locked, the submit by
which half of the groups had locked, the groups that never locked, the worst error of a learned offset in bits, and the good records
left unmarked per delivered frame (1.0 = every duplicate marked).

cost: the framer time (kernel_ms) of an all-RS41 step with set_diversity never called, with channels / 2 pairs set (mode 0) and
with learn | mark_duplicates (mode 3, offsets given), per Eb/N0.  With SONDE_MI355_LIB pointing at a build of an older commit the
variants it lacks are left out: interleave the two libraries from a shell loop (tools/ab_repeat.sh does the same for bench.py)."""
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


def signals(S, K, n, ebn0, seed, dev, fades=True, delays=None):
    """[S * K, n, 2] float32 on dev: channel s * K + k is copy k of sonde s; frames[s] = [(bit position, bytes)]; delays [S * K]:
    copy c starts delays[c] alternating bits late"""
    nbits = n // 10 + 16
    bits, frames = synth.rs41_bitstreams(seed, np.arange(S), nbits)
    bits = np.repeat(bits, K, axis=0)
    if delays is not None:
        for c, d in enumerate(delays):
            bits[c] = np.concatenate([(np.arange(d) & 1).astype(np.uint8), bits[c]])[:bits.shape[1]]
    clean, cfo, tau, amp = synth.gfsk_modulate(bits, n, 4800.0, seed=seed, ebn0_db=200.0, device=dev)
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


def learn_point(args, ebn0, seed):
    import diversity_align_reference as dar
    import diversity_reference as dr
    S, K, n, cuts = args.sondes, args.copies, TILE * args.tiles, args.cuts
    assert args.tiles % cuts == 0
    rng = np.random.default_rng(seed + 5)
    delays = np.array([0 if c % K == 0 else int(rng.integers(0, args.max_delay)) for c in range(S * K)])
    iq, frames = signals(S, K, n, ebn0, seed, "cpu", delays=delays)
    groups = [[s * K + k for k in range(K)] for s in range(S)]
    gpu = args.engine == "gpu"
    if not gpu:
        import oracle_lib
        oracle_lib.build()
        base = oracle_lib.batch_run(0, iq.numpy(), nthreads=args.threads)
        end = base["bitpos"].astype(np.int64) + 8 * base["len"].astype(np.int64)
        which = np.minimum(end * cuts // (n // 10), cuts - 1)
        subs = [base[which == k] for k in range(cuts)]

    def run(learn):
        """[(records, locked members per group)] per submit, and the final offsets"""
        out = []
        if gpu:
            from sdrpp_radiosonde_amd.batch import SondeBatch
            b = SondeBatch(S * K, n // cuts)
            b.set_diversity(groups, None if learn else delays, 0, learn=learn, mark_duplicates=learn)
            dev = iq.to("cuda:0")
            for k in range(cuts):
                b.submit(dev[:, k * (n // cuts):(k + 1) * (n // cuts)])
                fr = b.frames()
                st = [b.diversity_offsets(g) for g in range(S)]
                out.append((fr, [bin(x["locked"]).count("1") for x in st]))
            off = {ch: st[g]["offsets"][m] for g, mem in enumerate(groups) for m, ch in enumerate(mem)}
            b.close()
            return out, off
        st = dar.new_state(groups, None if learn else delays, 3 if learn else 0)
        for sub in subs:
            fr, _, st = dar.run(sub.copy(), groups, st, 3 if learn else 0)
            out.append((fr, [sum(st["locked"][ch] for ch in mem) for mem in groups]))
        return out, dict(st["off"])

    def delivered(fr):
        got, unmarked = set(), 0
        for f in fr:
            ch = int(f["channel"])
            if int(f["len"]) != 320 or int(f["nerr"][0]) < 0 or int(f["nerr"][1]) < 0:
                continue
            d, j = min((abs(int(f["bitpos"]) - p - int(delays[ch])), j) for j, (p, _) in enumerate(frames[ch // K]))
            if d < 64:
                got.add((ch // K, j))
                unmarked += not int(f["flags"]) & _lib.FRAME_DUPLICATE
        return got, unmarked

    given, _ = run(False)
    learned, off = run(True)
    g_all, _ = delivered(np.concatenate([fr for fr, _ in given]))
    l_all, unmarked = delivered(np.concatenate([fr for fr, _ in learned]))
    full = [next((k for k, (_, lk) in enumerate(learned) if lk[g] == K), None) for g in range(S)]
    locked_by = sorted(k for k in full if k is not None)
    err = [abs((off[ch] - off[mem[0]]) - int(delays[ch])) for g, mem in enumerate(groups) if full[g] is not None for ch in mem]
    return dict(ebn0_db=ebn0, engine=args.engine, sondes=S, copies=K, samples=n, cuts=cuts, max_delay_bits=args.max_delay,
                delivered_offsets_given=len(g_all), delivered_learned=len(l_all), lost_before_lock=len(g_all - l_all),
                delivered_only_when_learned=len(l_all - g_all), groups_never_locked=sum(k is None for k in full),
                half_locked_by_submit=locked_by[len(locked_by) // 2] if locked_by else None, worst_offset_error_bits=max(err) if err else None,
                unmarked_good_records_per_delivered_frame=round(unmarked / max(1, len(l_all)), 3))


def cost_point(args, ebn0, seed):
    from sdrpp_radiosonde_amd.batch import SondeBatch
    C, n = args.channels, TILE * args.tiles
    iq, _ = signals(C // 2, 2, n * args.steps, ebn0, seed, "cuda:0", fades=ebn0 < 30)
    res = dict(ebn0_db=ebn0, channels=C, tiles=args.tiles, lib=os.path.basename(_lib.LIB_PATH))
    variants = (["never_called"] + (["pairs_set"] if hasattr(_lib.load(), "sonde_batch_set_diversity") else []) +
                (["learn_mark"] if hasattr(_lib.load(), "sonde_batch_set_diversity_auto") else []))
    ms = {v: [] for v in variants}
    for rep in range(args.reps):             # interleaved: the two variants see the same box in the same minute
        for v in variants:
            b = SondeBatch(C, n)
            if v == "pairs_set":
                b.set_diversity([[2 * s, 2 * s + 1] for s in range(C // 2)])
            if v == "learn_mark":            # offsets given (zeros, locked from the start): the combining pass does the same work
                b.set_diversity([[2 * s, 2 * s + 1] for s in range(C // 2)], np.zeros(C, dtype=np.int64), 0, learn=True, mark_duplicates=True)
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
    ap.add_argument("mode", choices=["gain", "learn", "cost"])
    ap.add_argument("--cuts", type=int, default=10)
    ap.add_argument("--max-delay", type=int, default=2400)      # under one frame period (2880 bits): SPEC 3.3k's limit
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
    elif args.mode == "learn":
        args.tiles = args.tiles or 300
        if args.copies == 3 and "--copies" not in sys.argv:
            args.copies = 2
        for e in args.ebn0 or [9.0, 10.0, 14.0]:
            print(json.dumps(learn_point(args, e, args.seed)), flush=True)
    else:
        args.tiles = args.tiles or 96
        for e in args.ebn0 or [40.0, 9.0]:
            print(json.dumps(cost_point(args, e, args.seed)), flush=True)


if __name__ == "__main__":
    main()
