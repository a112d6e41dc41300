"""The HIP front-ends (channelizer.hip: sd_pfb_kernel + its FFT, the discriminator + 12/5 resampler; vfo.hip) against the float64
reference of tests/fe_reference.py under the same bounds as test_frontend_reference.py applies to the oracle.  Unlike the
parity tests these do not need the kernels to be bit-exact to the oracle: they hold for any float32 arithmetic that computes
the SPEC's operation within its rounding.  Every test prints its worst error as a fraction of its bound ("FE-REF" lines)."""
import numpy as np
import pytest
import torch

import fe_reference as R
from sdrpp_radiosonde_amd._lib import INPUT_IQ, INPUT_IQ8, INPUT_IQ16
from sdrpp_radiosonde_amd.batch import SondeChannelizer, SondeVfo
from test_frontend_reference import ROW_BINS, chan_rows_ratio, ratio, tone_scene, vfo_signals

pytestmark = pytest.mark.gpu
BLOCK = R.STEPS * R.D
NSUB = 3


def stream_scene(s: int, n: int) -> np.ndarray:
    """stream s of a multi-stream object: its own content (tones in other bins, noise at another level), complex128"""
    return (R.tones(n, [(k + 37 * s, df, 1.0) for k, df in ((0, 0.0), (1, 5000.0), (255, -9500.0), (256, R.BIN_HZ / 2), (511, 9500.0))], seed=40 + s)
            + R.chirp(n, 120.3 + 50 * s, 124.7 + 50 * s, 0.5) + R.noise(n, 0.05 * (s + 1), seed=50 + s))


def run_chan(blocks, bps=1, fused=False, dual=False, input_kind=INPUT_IQ):
    """blocks: [n_streams] arrays [NSUB * bps * BLOCK, 2] of the submit dtype.  Returns (phases [channels, steps] int64,
    rows [channels, steps * 12 / 5] or None), the submits' read() concatenated."""
    S = len(blocks)
    chz = SondeChannelizer(blocks_per_submit=bps, n_streams=S, fused=fused, dual=dual, input_kind=input_kind)
    assert chz.samples_per_submit == bps * BLOCK and chz.fused == fused
    dev = torch.from_numpy(np.stack(blocks)).cuda()
    n = chz.samples_per_submit
    ph, rows = [], []
    for b in range(NSUB):
        x = dev[:, b * n:(b + 1) * n].contiguous()
        chz.submit(x if S > 1 else x[0])
        q, o = chz.read()
        ph.append(np.rint(q.astype(np.float64) * 16384).astype(np.int64) & 0xFFFF)
        rows.append(o)
    chz.close()
    return np.concatenate(ph, axis=1), (None if fused else np.concatenate(rows, axis=1))


def check_bank(tag, q, x, odd, rows=None):
    """q: the 512 phases of one bank over the whole stream x (complex128); rows: its 48 kS/s rows or None"""
    Y, A = R.bank(x, odd)
    r = R.phase_errors(q, Y, A, odd)
    rl = R.phase_errors(q, Y, A, odd, loose=True)
    rr = chan_rows_ratio(q[ROW_BINS], rows[ROW_BINS]).max() if rows is not None else float("nan")
    print(f"FE-REF chan {tag} {'odd' if odd else 'even'}: phases {r.max():.3f} of the tight bound, {rl.max():.3f} of the loose; rows {rr:.3f}")
    assert r.max() <= 1.0, (tag, odd, r.max(), np.unravel_index(r.argmax(), r.shape))
    assert rl.max() <= 1.0, (tag, odd, rl.max())
    assert rows is None or rr <= 1.0, (tag, rr)


def as_complex(iq):
    iq = np.asarray(iq)
    return iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)


@pytest.mark.parametrize("bps,fused", [(1, False), (2, True), (5, True)])
def test_hip_bank_blocks_per_submit(bps, fused):
    n = NSUB * bps * BLOCK
    iq = R.as_iq32(tone_scene(bps, n) + R.chirp(n, 379.6, 384.4) + R.noise(n, 0.1, seed=bps))
    q, rows = run_chan([iq], bps=bps, fused=fused)
    check_bank(f"bps={bps} fused={fused}", q, as_complex(iq), False, rows)


def test_hip_bank_three_streams():
    """three streams with different content: a stream mixed up with another fails"""
    n = NSUB * BLOCK
    iqs = [R.as_iq32(stream_scene(s, n)) for s in range(3)]
    q, rows = run_chan(iqs)
    for s in range(3):
        check_bank(f"stream {s} of 3", q[512 * s:512 * (s + 1)], as_complex(iqs[s]), False, rows[512 * s:512 * (s + 1)])


@pytest.mark.parametrize("fused", [False, True])
def test_hip_bank_dual(fused):
    n = NSUB * BLOCK
    iq = R.as_iq32(stream_scene(0, n) + R.tones(n, [(100, R.BIN_HZ / 2, 1.0), (300, R.BIN_HZ / 2 + 4000.0, 0.5)], seed=3))
    q, rows = run_chan([iq], fused=fused, dual=True)
    x = as_complex(iq)
    check_bank(f"dual fused={fused}", q[:512], x, False, None if fused else rows[:512])
    check_bank(f"dual fused={fused}", q[512:], x, True, None if fused else rows[512:])


@pytest.mark.parametrize("bits,fused", [(16, False), (8, True)])
def test_hip_bank_integer_input(bits, fused):
    """SONDE_INPUT_IQ16 / IQ8 at full scale, clipped: +-32767 and -128 occur"""
    n = NSUB * BLOCK
    x = 0.5 * tone_scene(bits, n) / 3 + 0.3 * R.noise(n, 1.0, seed=bits)
    iq = R.as_int_iq(x, bits)
    assert iq.max() == (1 << (bits - 1)) - 1 and iq.min() == (-32767 if bits == 16 else -128)
    q, rows = run_chan([iq], fused=fused, input_kind=INPUT_IQ16 if bits == 16 else INPUT_IQ8)
    check_bank(f"int{bits} fused={fused}", q, as_complex(iq), False, rows)


@pytest.mark.parametrize("rate", R.VFO_RATES)
def test_hip_vfo_rows(rate):
    """SondeVfo at every rate: one channel per signal of vfo_signals (strided rows of one recording), in the ragged pieces of
    test_gpu_vfo.py across the kernel's 1600-sample chunk edge: rows within the tight and (levels above 1e-12) loose bounds"""
    up, down, _ = R.vfo_ratio(rate)
    pieces = [down, 1600, 1600 + down, 3 * 1600, 7 * down, 4800 - 2 * down, 12800]
    n = sum(pieces)
    sigs = vfo_signals(rate, n)
    iq = np.stack([s for _, s, _ in sigs])
    C = iq.shape[0]
    v = SondeVfo(C, rate, max(pieces))
    dev = torch.from_numpy(iq).cuda()
    got, a = [], 0
    for m in pieces:
        out = v.process(dev[:, a:a + m])
        assert out.shape == (C, m * up // down)
        got.append(out.cpu().numpy())
        a += m
    v.close()
    got = np.concatenate(got, axis=1)
    worst = {}
    for c, (name, s, tight_only) in enumerate(sigs):
        o, b, _ = R.vfo_rows_ref(s, rate)
        rt = ratio(np.abs(got[c].astype(np.float64) - o), b).max()
        rl = 0.0
        if not tight_only:
            o, b, valid = R.vfo_rows_ref(s, rate, loose=True)
            rl = np.where(valid, ratio(np.abs(got[c].astype(np.float64) - o), b), 0.0).max()
        worst[name] = (rt, rl)
        assert rt <= 1.0 and rl <= 1.0, (name, rt, rl)
    print(f"FE-REF vfo {rate}: " + ", ".join(f"{k} {a:.3f}/{b:.3f}" for k, (a, b) in worst.items()) + " (tight/loose fraction of bound)")
