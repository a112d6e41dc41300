#!/usr/bin/env python3
"""What SONDE_FLAG_RS41_RESCUE (DESIGN SPEC 3.3c) gains on fading RS41 signals:

    python tools/rescue_measure.py [--channels 64] [--tiles 600] [--ebn0 12] [--runs 3]

RS41 channels at the given Eb/N0; in every transmitted frame the signal's amplitude is cut to zero (the noise stays) for 40-90 ms at a
random place: the fade of a spinning payload.  The same samples go through a batch without and with the flag; per run one JSON line:
CRC-good blocks and complete frames (every block good) among the transmitted frames, without / with the flag, the frames the second
pass rescued, and the rescued frames whose bytes 8..len differ from the transmitted ones (expected: 0; anything else is a false accept
and is listed)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrpp_radiosonde_amd import _lib, synth                    # noqa: E402
from sdrpp_radiosonde_amd.batch import SondeBatch               # noqa: E402

TILE = 2048


_CRC_TAB = []
for _v in range(256):
    _c = _v << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x1021) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC_TAB.append(_c)


def crc16(data):
    """CRC16-CCITT (0x1021, init 0xFFFF)"""
    crc = 0xFFFF
    for v in bytes(data):
        crc = ((crc << 8) & 0xFFFF) ^ _CRC_TAB[(crc >> 8) ^ v]
    return crc


def good_blocks(d, tx):
    """blocks of the generator's standard layout whose CRC passes on d and whose bytes are the transmitted ones"""
    off, n = 57, 0
    for _, ln in synth.RS41_SUBFRAMES_STD:
        blk = slice(off, off + ln + 4)
        if np.array_equal(d[blk], tx[blk]) and crc16(d[off + 2: off + 2 + ln].tobytes()) == (int(d[off + 2 + ln]) | int(d[off + 3 + ln]) << 8):
            n += 1
        off += ln + 4
    return n


def run(args, seed):
    C, n = args.channels, TILE * args.tiles
    dev = "cuda:0"
    nbits = n // 10 + 16
    bits, frames = synth.rs41_bitstreams(seed, np.arange(C), nbits)
    clean, cfo, tau, amp = synth.gfsk_modulate(bits, n, 4800.0, seed=seed, ebn0_db=200.0, device=dev)
    rng = np.random.default_rng(seed)
    gain = torch.ones((C, n), dtype=torch.float32, device=dev)
    for c in range(C):
        for pos, _ in frames[c]:
            ln = int(rng.integers(int(0.040 * 48000), int(0.090 * 48000) + 1))
            s0 = int((pos + tau[c]) * 10) + int(rng.integers(0, 320 * 80 - ln))
            gain[c, s0:s0 + ln] = 0.0
    sigma = torch.from_numpy(amp * math.sqrt(10.0 / (2.0 * 10.0 ** (args.ebn0 / 10.0)))).to(dev).to(torch.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 1)
    iq = clean * gain[:, :, None] + sigma[:, None, None] * torch.randn((C, n, 2), generator=g, device=dev, dtype=torch.float32)
    del clean, gain
    res = {}
    cuts = 4 if args.tiles % 4 == 0 else 1
    for name, flags in (("off", 0), ("on", _lib.FLAG_RS41_RESCUE)):
        b = SondeBatch(C, n // cuts, flags=flags)
        parts = []
        for k in range(cuts):
            b.submit(iq[:, k * (n // cuts):(k + 1) * (n // cuts)])
            parts.append(b.frames())
        b.close()
        fr = np.concatenate(parts)
        blocks = complete = rescued = 0
        wrong = []
        for f in fr:
            c = int(f["channel"])
            d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in frames[c]), key=lambda t: t[0])
            if d >= 64 or int(f["len"]) != 320:
                continue
            gb = good_blocks(f["data"], tx)
            blocks += gb
            complete += gb == len(synth.RS41_SUBFRAMES_STD)
            if int(f["flags"]) & _lib.FRAME_RESCUED:
                rescued += 1
                if not np.array_equal(f["data"][8:320], tx[8:320]):
                    wrong.append((c, pos, [int(v) for v in f["nerr"]]))
        res[name] = dict(records=int(len(fr)), failed_records=int((fr["nerr"] < 0).any(axis=1).sum()), good_blocks=int(blocks),
                         complete_frames=int(complete), rescued=int(rescued), rescued_wrong=wrong)
    sent = sum(len(f) for f in frames)
    return dict(seed=seed, channels=C, samples=n, ebn0_db=args.ebn0, frames_sent=sent, blocks_sent=sent * len(synth.RS41_SUBFRAMES_STD), **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=600)
    ap.add_argument("--ebn0", type=float, default=12.0)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    for r in range(args.runs):
        print(json.dumps(run(args, 500 + r)), flush=True)


if __name__ == "__main__":
    main()
