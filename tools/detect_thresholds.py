"""Threshold study of the sonde type detector: the float64 / integer reference (tests/detect_reference.py) over
complex AWGN and over 30 dB signals of every type, on the CPU.  Prints, per type k, the largest best_k seen on noise and on
each other type's signals, the smallest best_k on the type's own signals, and theta_k = margin x the largest foreign value.

    python tools/detect_thresholds.py [--channels 16] [--noise-seconds 256] [--margin 1.1] [--ebn0 30]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_reference as R                      # noqa: E402
from sdrpp_radiosonde_amd import synth            # noqa: E402

NAMES = ("RS41", "DFM", "iMS-100", "M10", "iMet-4", "SRS-C50", "MRZ-N1")
N2S = 96000


def type_rows(t: int, C: int, seed: int, ebn0: float, invert: bool = False):
    kw = {} if t in (R.IMET4, R.C50) else dict(cfo_max_hz=2000.0, invert=invert)
    sb = synth.make_batch(t, C, N2S, seed=seed, ebn0_db=ebn0, **kw)
    return sb.iq.numpy(), sb


def bests(rows):
    return np.array([R.detect_rows(r, False)[1] for r in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--noise-seconds", type=int, default=256)
    ap.add_argument("--margin", type=float, default=1.1)
    ap.add_argument("--ebn0", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=101)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    nz = []
    for i in range(a.noise_seconds // 2):
        x = rng.standard_normal((N2S, 2)).astype(np.float32)
        nz.append(R.detect_rows(x, False)[1])
    nz = np.max(nz, axis=0)
    own = np.zeros((7, 7))            # [signal type, template type]: max best
    own_min = np.zeros(7)
    for t in range(7):
        B = bests(type_rows(t, a.channels, a.seed + t, a.ebn0)[0])
        if t not in (R.IMET4, R.C50):
            B = np.concatenate([B, bests(type_rows(t, a.channels, a.seed + 50 + t, a.ebn0, invert=True)[0])])
        own[t] = B.max(axis=0)
        own_min[t] = B[:, t].min()
    print(f"noise: {a.noise_seconds} channel-seconds; signals: {a.channels} channels x 2 s per type (GFSK: upright and inverted), Eb/N0 {a.ebn0} dB")
    print("type      noise   " + " ".join(f"{n[:7]:>7}" for n in NAMES) + "   foreign  own-min  theta")
    for k in range(7):
        foreign = max(nz[k], max(own[t, k] for t in range(7) if t != k))
        print(f"{NAMES[k]:<8} {nz[k]:6.3f}   " + " ".join(f"{own[t, k]:7.3f}" for t in range(7)) +
              f"   {foreign:7.3f}  {own_min[k]:7.3f}  {a.margin * foreign:5.3f}")


if __name__ == "__main__":
    main()
