"""Kernel A (demod_kernel.hip: the single-type and the one-launch mixed instantiations) and the tone front-end (afsk.hip) against the
float64 reference of tests/demod_reference.py, tile by tile: 2048-sample submits (16 384 with AFSK channels), and after every submit
the state and new bits of every channel are replayed against one step of the SPEC's recurrence (test_demod_reference.py applies the
same to the oracle).  This does not need the kernel to be bit-exact to the oracle.  The last test carries the per-tile verdict over to
the launch shapes the benchmark times: the same IQ in submits of 96 tiles, with and without time slices, gives the same bits and end
states as the 2048-sample submits."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

import demod_reference as D
from sdrpp_radiosonde_amd._lib import FLAG_WIDE, FLAG_WIDE_AUTO, INPUT_IQ, INPUT_IQ8, INPUT_IQ16, INPUT_REAL
from sdrpp_radiosonde_amd.batch import SondeBatch
from test_demod_reference import AMB_LIMIT, Scene, check, make_input

pytestmark = pytest.mark.gpu
NT = 24                     # tiles per channel
KIND = {"iq": INPUT_IQ, "iq16": INPUT_IQ16, "iq8": INPUT_IQ8, "real": INPUT_REAL}
CFO = (0.0, 1000.0, -2000.0, 2000.0, -1000.0)
EBN0 = (10.0, 30.0, 15.0, 20.0)
LEVEL = {"iq": (1.0, 1e-6, 1e6, 1.0), "iq16": (20000.0, 40000.0), "iq8": (8.0, 150.0), "real": (1.0,)}


def scenes(types, n: int, kind: str = "iq", wide: bool = False, seed: int = 0, ntiles: int = NT):
    """n channels drawn from the CPU scene matrix: types in turn, carriers 0 / +1 / -2 / +2 / -1 kHz, Eb/N0 10-30 dB, clocks
    +-100 ppm, levels"""
    out = []
    for i in range(n):
        t = types[i % len(types)]
        out.append(Scene(f"{kind}-t{t}-{i}", t, wide=wide, kind=kind, ebn0=EBN0[i % 4] if t not in (4, 5) else 20.0 - 4 * (i % 2),
                         cfo=CFO[i % 5] if t not in (4, 5) else 0.0, ppm=(100.0, -100.0, 0.0)[i % 3],
                         level=LEVEL[kind][i % len(LEVEL[kind])], seed=1000 + seed + i, m20=(t == 3 and i % 2 == 1), ntiles=ntiles))
    return out


def tile_in(S) -> int:
    return D.TILE * (8 if any(s.stype in (4, 5) for s in S) else 1)


def run_gpu(S, xs, flags: int = 0, submit_tiles: int = 1, time_slices: int = 0):
    """feed SondeBatch `submit_tiles` tiles per submit: (states [channel][submit], bits [channel][submit])"""
    C = len(S)
    tin = tile_in(S)
    n = S[0].ntiles * tin
    step = submit_tiles * tin
    b = SondeBatch(C, step, types=np.array([s.stype for s in S], np.uint8), input_kind=KIND[S[0].kind], flags=flags,
                   time_slices=time_slices)
    x = torch.from_numpy(np.stack(xs)).cuda()
    states = [[] for _ in range(C)]
    bits = [[] for _ in range(C)]
    nb = [0] * C
    for off in range(0, n, step):
        b.submit(x[:, off:off + step])
        b.sync()
        for c in range(C):
            k = b.nbits(c)
            bits[c].append(b.read_bits(c, nb[c], k - nb[c]) if k > nb[c] else np.zeros(0, np.uint8))
            nb[c] = k
            states[c].append(b.state(c))
    b.close()
    return states, bits


def replay_all(S, xs, states, bits, tag: str):
    worst, amb, nbits = {}, 0, 0
    for s, x, st, bt in zip(S, xs, states, bits):
        chk = check(s, x, st, bt)
        assert not chk.failures(), chk.line(s.name)
        if s.ebn0 >= 10.0:
            assert chk.amb <= AMB_LIMIT * chk.nbits, chk.line(s.name)
        for k, v in chk.worst.items():
            worst[k] = max(worst.get(k, 0.0), v)
        amb += chk.amb
        nbits += chk.nbits
    w = " ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items()))
    print(f"DEMOD-REF gpu {tag}: channels={len(S)} tiles={S[0].ntiles} bits={nbits} ambiguous={amb} ({amb / max(nbits, 1):.2e}) {w}")


MIXED = (0, 1, 2, 3, 6)
CASES = {
    "rs41-iq": dict(types=(0,), kind="iq"),
    "mixed-iq": dict(types=MIXED, kind="iq"),
    "mixed-iq-wide": dict(types=MIXED, kind="iq", flags=FLAG_WIDE),
    "mixed-iq-wide-auto": dict(types=MIXED, kind="iq", flags=FLAG_WIDE_AUTO),
    "mixed-iq16": dict(types=MIXED, kind="iq16"),
    "mixed-iq8": dict(types=MIXED, kind="iq8"),
    "mixed-real": dict(types=MIXED, kind="real"),
    "afsk-iq": dict(types=(4, 5), kind="iq", ntiles=6),
}


def _wide_of(t: int, flags: int) -> bool:
    return bool(flags & FLAG_WIDE) or (bool(flags & FLAG_WIDE_AUTO) and t in D.WIDE_AUTO_TYPES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_replay(case):
    c = CASES[case]
    flags = c.get("flags", 0)
    S = scenes(c["types"], 35 if len(c["types"]) == 5 else 32, c["kind"], seed=17 * len(case), ntiles=c.get("ntiles", NT))
    S = [dataclasses.replace(s, wide=_wide_of(s.stype, flags)) for s in S]
    xs = [make_input(s) for s in S]
    states, bits = run_gpu(S, xs, flags=flags)
    replay_all(S, xs, states, bits, case)


@pytest.mark.parametrize("types", [(0,), MIXED], ids=["rs41", "mixed"])
def test_bench_shapes_equal_tile_submits(types):
    """96 tiles per submit (the benchmark's launch shape), with the library's time slices and with 4: bits and end states identical to
    2048-sample submits of the same IQ, whose every tile the replay accepts"""
    S = scenes(types, 35 if len(types) == 5 else 32, "iq", seed=5, ntiles=96)
    xs = [make_input(s) for s in S]
    st1, b1 = run_gpu(S, xs)
    replay_all(S, xs, st1, b1, "96-tiles-" + "-".join(map(str, types)))
    for ts in (0, 4):
        st, b = run_gpu(S, xs, submit_tiles=96, time_slices=ts)
        for c in range(len(S)):
            assert np.array_equal(np.concatenate(b[c]), np.concatenate(b1[c])), (ts, c)
            assert st[c][-1] == st1[c][-1], (ts, c)
