"""sd_bins_kernel (bins_kernel.hip: the one-wave-per-bin decoder behind the filter bank, all of config 4 after the bank) against the
float64 references written from DESIGN.md alone: after every submit the phases the bank produced (SondeChannelizer.read), and the loop
state and new bits of every watched bin, are replayed with d, bd = fe_reference.composite_rows(phases) (SPEC 3.5b as "resample, then
average") through demod_reference.replay, whose hidden-state mode bridges the 3 (6) tiles of a submit.  This does not need the kernel
to be bit-exact to the oracle (tests/test_channelizer.py holds it to that): a rewrite that sums in another order keeps this test.
The scene is bins_scenes.scene(): generated on the CPU, the samples test_bins_reference.py runs through the oracle.  The last test
carries the verdict over to the launch shapes that cannot be replayed (5 blocks per submit: the pass pipeline's n_pass = 40; eight
streams x 4 blocks: the benchmark's wideband8x4): same bits and end states as the 1-block submits whose every span the replay accepted."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import bins_scenes as B
from sdrpp_radiosonde_amd._lib import INPUT_IQ, INPUT_IQ16
from sdrpp_radiosonde_amd.batch import SondeChannelizer
from test_demod_reference import AMB_LIMIT

pytestmark = pytest.mark.gpu
_dev: dict = {}
_runs: dict = {}


def device_scene(int16: bool = False, late: bool = False) -> torch.Tensor:
    key = "late" if late else "i16" if int16 else "f32"
    if key not in _dev:
        _dev[key] = torch.from_numpy(B.late_scene() if late else B.scene_int16() if int16 else B.scene()).cuda()
    return _dev[key]


def run_chz(channels, *, types=None, bps: int = 1, dual: bool = False, int16: bool = False, streams: int = 1, nblk: int = B.NBLK,
            phases: bool = True, late: bool = False):
    """the scene (late: bins_scenes.late_scene) through a fused SondeChannelizer, bps blocks per submit (the same content in every
    stream): {channel: (q over the whole run or None, states per submit, new bits per submit)}"""
    x = device_scene(int16, late)
    chz = SondeChannelizer(types=types, blocks_per_submit=bps, n_streams=streams, dual=dual, input_kind=INPUT_IQ16 if int16 else INPUT_IQ)
    assert chz.fused and chz.samples_per_submit == bps * B.BLOCK
    res = {c: ([], [], []) for c in channels}
    nb = {c: 0 for c in channels}
    for s in range(nblk // bps):
        blk = x[s * bps * B.BLOCK:(s + 1) * bps * B.BLOCK]
        chz.submit(blk.unsqueeze(0).expand(streams, -1, -1).contiguous() if streams > 1 else blk.contiguous())
        chz.batch.sync()
        ph = chz.read()[0] if phases else None
        for c in channels:
            q, states, bits = res[c]
            if ph is not None:
                q.append(B.to_q16(ph[c]))
            n = chz.batch.nbits(c)
            bits.append(chz.batch.read_bits(c, nb[c], n - nb[c]) if n > nb[c] else np.zeros(0, np.uint8))
            nb[c] = n
            states.append(chz.batch.state(c))
    chz.close()
    return {c: (np.concatenate(q) if q else None, st, bt) for c, (q, st, bt) in res.items()}


def _even(all_rs41: bool = False):
    w = B.watched_even()
    return [(k, k, 0 if all_rs41 else ty, e) for k, ty, e in (w[::2] if all_rs41 else w)]


# case: (watched [(name bin, channel, type, Eb/N0)], run_chz arguments)
CASES = {
    "mixed-1": (_even(), dict(types=B.bin_types(), bps=1)),
    "mixed-2": (_even(), dict(types=B.bin_types(), bps=2)),
    "rs41-1": (_even(True), dict(types=None, bps=1)),
    "rs41-2": (_even(True), dict(types=None, bps=2)),
    "dual-1": ([(k, 512 + k, ty, e) for k, _, ty, e in B.ODD_TX] + [(k, k, ty, e) for k, ty, e in B.watched_even() if k in (64, 65, 511)],
               dict(types=B.bin_types(dual=True), bps=1, dual=True)),
    "int16-1": (_even(), dict(types=B.bin_types(), bps=1, int16=True)),
}


def replayed(case: str):
    """run the case once, replay every watched channel, assert, and keep the run: (results, the printed line)"""
    if case not in _runs:
        watch, kw = CASES[case]
        res = run_chz([c for _, c, _, _ in watch], **kw)
        chks = []
        for k, c, ty, _ in watch:
            q, states, bits = res[c]
            chks.append((f"ch{c}", B.replay_bin(q, ty, states, bits, B.TILES_PER_BLOCK * kw["bps"])))
        _runs[case] = (res, B.summarise(case, chks, [e for _, _, _, e in watch], AMB_LIMIT))
    return _runs[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_bins_kernel_block_replay(case):
    """1 and 2 blocks per submit, per-bin types (four types in the eight bins of one workgroup: the four tap slots, utype = -1) and
    all-RS41 (utype >= 0), the dual bank (the odd bins' own phases feed the reference) and 16-bit input: no failure, the ambiguity limit
    for the channels at >= 10 dB, and the unresolved cap (at most 5 % of all spans, no channel more than a quarter of its own).
    Observed on the MI355X: see profiles/bins_reference_notes.md (no span unresolved in any case; the oracle, on the same samples: none)."""
    _, line = replayed(case)
    print(line)


def test_bins_kernel_late_carrier_replay():
    """bins_scenes.late_scene, one stream, one block per submit, two submits: the branch of the loop update that no round of the scene
    above takes, the ONE-SIDED round (SPEC 3.2: block 2's first tile, every symbol below the threshold), behind the acquisition boundary
    (SPEC 3.2b: block 1) and on a state carried from one submit to the next.  The block replay of the cases above, the same conditions;
    that the round is one-sided is asserted of the bits (test_bins_reference.py asserts it of the oracle's)."""
    k, _, ty, e = B.LATE_TX
    q, states, bits = run_chz([k], types=B.bin_types(), bps=1, nblk=B.LATE_NBLK, late=True)[k]
    print(B.summarise("late-1", [(f"ch{k}", B.replay_bin(q, ty, states, bits, B.TILES_PER_BLOCK))], [e], AMB_LIMIT))
    assert len(set(bits[1][:190].tolist())) == 1 and 0.25 < bits[1][230:].mean() < 0.75


@pytest.mark.parametrize("shape", ["5-blocks", "8-streams-x-4-blocks"])
def test_larger_submits_equal_block_submits(shape):
    """5 blocks per submit (n_pass = 40) and eight streams x 4 blocks per submit (the launch shape of bench.py's wideband8x4), the same
    content in every stream: bits and end states identical to the 1-block submits of the same scene, whose every span the replay
    accepted (the argument of test_gpu_demod_reference.py::test_bench_shapes_equal_tile_submits)."""
    ref, line = replayed("mixed-1")
    print(line)
    watch, kw = CASES["mixed-1"]
    bps, streams = (5, 1) if shape == "5-blocks" else (4, 8)
    nblk = (B.NBLK // bps) * bps
    chans = [512 * s + c for s in range(streams) for _, c, _, _ in watch]
    types = np.tile(kw["types"], streams)
    got = run_chz(chans, types=types, bps=bps, streams=streams, nblk=nblk, phases=False)
    for s in range(streams):
        for _, c, _, _ in watch:
            _, st1, b1 = ref[c]
            _, st, b = got[512 * s + c]
            assert np.array_equal(np.concatenate(b), np.concatenate(b1[:nblk])), (shape, s, c)
            assert st[-1] == st1[nblk - 1], (shape, s, c)
