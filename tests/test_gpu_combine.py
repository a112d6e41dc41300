"""The coherent antenna combiner on the GPU (DESIGN SPEC 3.14) against tests/combine_reference.py: M, the weights and the output
within their bounds on rows of the real tuner, bit-identical however the stream is cut and through strided NaN-filled buffers,
restart, zero rows, refusals; then DiversityReceiver(combine="coherent") on a two-antenna wideband scene with fades against a
SondeBatch fed by hand, and combine="frames" left as it was."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import combine_reference as CR
import combine_scenes as CS
import track_reference as TR
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd import combine as cb
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError
from sdrpp_radiosonde_amd.combine import SondeCombiner
from sdrpp_radiosonde_amd.diversity import DiversityReceiver
from sdrpp_radiosonde_amd.tuner import SondeTuner

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FS = 1_000_000
GRANULE = 128_000            # the iq48 chain's granule at 1 MS/s: 6144 samples at 48 kHz
SONDES = [(-300_000, 0), (100_000, 1), (350_000, 3)]          # RS41, DFM, M10
S, N = 3, 8192
SIGMA = 0.02                 # each antenna's own noise floor (per component); the carriers stand 20 dB (Eb/N0) above it


def _scene(n, seed):
    """the carriers alone (the generator's floor 40 dB below the antennas' own), on the device: ([n] complex64, frames, symbols)"""
    iq, frames, symbols = synth.make_wideband_scene(SONDES, n, fs=FS, ebn0_db=60.0, noise_sigma=SIGMA / 100.0, seed=seed, device=DEV)
    return torch.view_as_complex(iq.contiguous()), frames, symbols


def _antenna(sc, gain, seed):
    """what one antenna delivers: the scene through its gain (a complex number or a [n] tensor) under its own noise, [n, 2] float32"""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    noise = SIGMA * torch.randn((sc.shape[0], 2), generator=gen, device=DEV, dtype=torch.float32)
    return (torch.view_as_real((sc * gain).to(torch.complex64)) + noise).contiguous()


@pytest.fixture(scope="module")
def rows():
    """[4 * 3, 8192, 2]: row a * 3 + i = sonde i (RS41 / DFM / M10 VFOs at 48 kHz) on antenna a, four antennas"""
    n_in = 2 * GRANULE
    sc, _, _ = _scene(n_in, 5)
    g = CS.gains(4, 1, equal=False)
    out = []
    for a in range(4):
        tu = SondeTuner(FS, 48_000, [(f, b) for f, _, b in TR.iq48_vfos(SONDES)], n_in)
        out.append(tu.process(_antenna(sc, complex(g[a]), 40 + a))[:, :N].clone())
        tu.close()
    return torch.cat(out, 0).contiguous()


def _host(rows, K, i):
    """sonde i's K rows as [K, n] complex128"""
    h = rows[:K * S].cpu().numpy().astype(np.float64)
    return np.stack([h[a * S + i, :, 0] + 1j * h[a * S + i, :, 1] for a in range(K)])


def _cplx(v):
    return v[..., 0::2] + 1j * v[..., 1::2]


def _sorted(r):
    return r[np.lexsort((r["block"], r["sonde"]))]


def _feed(comb, rows, cuts, inbuf=None, outbuf=None):
    """(output [S, n, 2] on the host, read-out of every submit, sorted)"""
    outs, reads, a = [], [], 0
    for k in cuts:
        part = rows[:, a:a + k]
        if inbuf is not None:
            inbuf[:, :k] = part
            part = inbuf[:, :k]
        y = comb.process(part, out=None if outbuf is None else outbuf)
        reads.append(comb.readout())
        outs.append(y.cpu().numpy().copy())
        a += k
    assert a == rows.shape[1]
    return np.concatenate(outs, axis=1), _sorted(np.concatenate(reads))


def _check(rows, K, L, y, r, first_prev=None):
    """the read-out and the output of one run over rows[:, :n] against the reference, sonde by sonde"""
    for i in range(S):
        x = _host(rows, K, i)
        M, A = CR.stats_ref(x, L)
        bnd = CR.bound(A, L)
        ri = r[r["sonde"] == i]
        assert len(ri) == len(M) and np.array_equal(ri["block"], np.arange(len(M)))
        dev = np.abs(ri["m"] - M)
        used = A > 0
        print(f"K {K} L {L} sonde {i}: worst M deviation / bound {float(np.max(dev[used] / bnd[used])):.3f}")
        assert np.all(dev <= bnd), (i, float(np.max(dev[used] / bnd[used])))
        assert np.all(ri["m"][~used] == 0.0)
        cross = np.hypot(ri["m"][:, 4], ri["m"][:, 5])
        assert np.all(cross > 1000.0 * np.maximum(bnd[:, 4], bnd[:, 5]))                 # the cross terms lie well above the bound
        W = _cplx(ri["w"])[:, :K]
        prev = None if first_prev is None else first_prev[i]
        for b in range(len(ri)):
            want = cb.weights(ri["m"][b], prev, antennas=K)
            assert np.max(np.abs(W[b].real - want.real)) <= 1e-12 and np.max(np.abs(W[b].imag - want.imag)) <= 1e-12, (i, b, W[b], want)
            prev = W[b]
        assert np.all(np.abs(np.linalg.norm(W, axis=1) - 1.0) <= 1e-12)
        assert np.array_equal(ri["wf"], ri["w"].astype(np.float32)) and np.all(ri["w"][:, 2 * K:] == 0.0)
        wf = _cplx(ri["wf"].astype(np.float64))[:, :K]
        ref, T = CR.apply_ref(x, wf, L)
        ab = CR.apply_bound(T, K)
        got = y[i].astype(np.float64)
        er, ei = np.abs(got[:, 0] - ref.real), np.abs(got[:, 1] - ref.imag)
        nz = ab[:, 0] > 0
        print(f"K {K} L {L} sonde {i}: worst output deviation / bound {float(np.max(er[nz] / ab[nz, 0])):.3f}")
        assert np.all(er <= ab[:, 0]) and np.all(ei <= ab[:, 1])
        assert np.median(np.abs(ref)) > 1e4 * np.median(ab)


# ---------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("L", [256, 1024])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_arithmetic_within_the_reference_bounds(rows, K, L):
    comb = SondeCombiner(S, K, 48_000, N, L)
    assert comb.block == L
    y, r = _feed(comb, rows[:K * S], [N])
    assert len(r) == S * (N // L)
    _check(rows, K, L, y, r)
    comb.close()


def test_default_block(rows):
    comb = SondeCombiner(S, 2, 48_000, N)
    assert comb.block == 1024 == cb.defaults(48_000)
    comb.close()


# ---------------------------------------------------------------- cutting and layout
@pytest.mark.parametrize("K", [2, 4])
def test_bit_identical_however_the_stream_is_cut_and_through_strided_buffers(rows, K):
    x = rows[:K * S]
    one_y, one_r = _feed(SondeCombiner(S, K, 48_000, N), x, [N])
    for cuts in ([1024] * 8, [1024, 3072, 4096]):
        y, r = _feed(SondeCombiner(S, K, 48_000, max(cuts)), x, cuts)
        assert y.tobytes() == one_y.tobytes() and r.tobytes() == one_r.tobytes(), cuts
    # rows an odd number of samples apart, in and out, longer than any submit, filled with NaN
    inbuf = torch.full((K * S, 4099, 2), float("nan"), device=DEV)
    outbuf = torch.full((S, 4101, 2), float("nan"), device=DEV)
    y, r = _feed(SondeCombiner(S, K, 48_000, 4096), x, [1024, 3072, 4096], inbuf=inbuf, outbuf=outbuf)
    assert y.tobytes() == one_y.tobytes() and r.tobytes() == one_r.tobytes()
    assert bool(torch.isnan(outbuf[:, 4096:]).all())                       # nothing written past the rows


# ---------------------------------------------------------------- restart and zero rows
def test_restart_makes_the_output_that_of_a_stream_that_began_there(rows):
    K, h = 2, N // 2
    x = rows[:K * S]
    one_y, one_r = _feed(SondeCombiner(S, K, 48_000, N), x, [N])
    comb = SondeCombiner(S, K, 48_000, N)
    y0 = comb.process(x[:, :h]).cpu().numpy().copy()
    comb.restart(1)
    y1 = comb.process(x[:, h:]).cpu().numpy().copy()
    r1 = _sorted(comb.readout())
    lone = torch.cat([x[a * S + 1:a * S + 2, h:] for a in range(K)], 0).contiguous()
    fresh_y, fresh_r = _feed(SondeCombiner(1, K, 48_000, N), lone, [N - h])
    assert y1[1].tobytes() == fresh_y[0].tobytes()
    mine = r1[r1["sonde"] == 1]
    assert np.array_equal(mine["block"], np.arange(h // 1024))
    for k in ("m", "w", "wf"):
        assert mine[k].tobytes() == fresh_r[k].tobytes(), k
    assert y1[1].tobytes() != one_y[1, h:].tobytes()                        # (the weights' phase started anew)
    for i in (0, 2):
        assert np.concatenate([y0[i], y1[i]]).tobytes() == one_y[i].tobytes()
        assert r1[r1["sonde"] == i].tobytes() == one_r[(one_r["sonde"] == i) & (one_r["block"] >= h // 1024)].tobytes()
    assert y0[1].tobytes() == one_y[1, :h].tobytes()
    with pytest.raises(SondeError, match="no such sonde"):
        comb.restart(3)
    comb.close()


def test_zero_rows(rows):
    K, L = 3, 1024
    x = rows[:K * S].clone()
    x[S:2 * S] = 0.0                                                        # antenna 1 hears nothing (an idle tuner slot reads as zeros)
    comb = SondeCombiner(S, K, 48_000, N, L)
    y, r = _feed(comb, x, [N])
    assert np.all(np.isfinite(y)) and np.all(r["w"][:, 2:4] == 0.0) and np.all(r["m"][:, 1] == 0.0)
    for i in range(S):
        xs = _host(x, K, i)
        ri = r[r["sonde"] == i]
        W = _cplx(ri["w"])[:, :K]
        assert np.all(np.abs(np.linalg.norm(W, axis=1) - 1.0) <= 1e-12)
        ref, T = CR.apply_ref(xs, _cplx(ri["wf"].astype(np.float64))[:, :K], L)
        ab = CR.apply_bound(T, K)
        assert np.all(np.abs(y[i, :, 0] - ref.real) <= ab[:, 0]) and np.all(np.abs(y[i, :, 1] - ref.imag) <= ab[:, 1])
    # all-zero input: zeros out, the weights hold
    last = r[r["block"] == N // L - 1]
    z = comb.process(torch.zeros_like(x[:, :2048]))
    rz = _sorted(comb.readout())
    assert bool((z == 0).all()) and np.all(rz["m"] == 0.0)
    for i in range(S):
        for b in rz[rz["sonde"] == i]:
            assert np.array_equal(b["w"], last[last["sonde"] == i][0]["w"]) and b["block"] >= N // L
    # a combiner that has seen nothing but zeros: antenna 0, zeros out
    c2 = SondeCombiner(S, K, 48_000, 2048, L)
    z = c2.process(torch.zeros_like(x[:, :2048]))
    assert bool((z == 0).all()) and np.all(c2.readout()["w"] == np.array([1.0, 0, 0, 0, 0, 0, 0, 0]))
    comb.close(); c2.close()


# ---------------------------------------------------------------- refusals
def test_refusals(rows):
    with pytest.raises(SondeError, match="antennas"):
        SondeCombiner(S, 1, 48_000, 2048)
    with pytest.raises(SondeError, match="antennas"):
        SondeCombiner(S, 5, 48_000, 2048)
    with pytest.raises(SondeError, match="input_kind"):
        SondeCombiner(S, 2, 48_000, 2048, input_kind=_lib.INPUT_REAL)
    with pytest.raises(SondeError, match="block"):
        SondeCombiner(S, 2, 48_000, 2048, 1000)
    with pytest.raises(SondeError, match="max_samples"):
        SondeCombiner(S, 2, 48_000, 1536)
    with pytest.raises(SondeError, match="rate"):
        SondeCombiner(S, 2, 1000, 2048)
    with pytest.raises(SondeError, match="sonde_combine_create: no such HIP device"):
        SondeCombiner(S, 2, 48_000, 2048, device=torch.cuda.device_count())
    comb = SondeCombiner(S, 2, 48_000, 2048)
    x = rows[:2 * S]
    with pytest.raises(SondeError, match="multiple of the block"):
        comb.process(x[:, :1280])
    with pytest.raises(SondeError, match="max_samples"):
        comb.process(x[:, :4096])
    with pytest.raises(SondeError, match="2 x 3 rows"):
        comb.process(rows[:3 * S, :2048])
    with pytest.raises(SondeError, match="REAL"):
        comb.process(x[:, :2048, 0])
    with pytest.raises(SondeError, match="device"):
        comb.process(x[:, :2048].cpu())
    with pytest.raises(SondeError, match="out must be"):
        comb.process(x[:, :2048], out=torch.empty((S, 1024, 2), device=DEV))
    with pytest.raises(SondeError, match="no such sonde"):
        comb.restart(S)
    import ctypes as C
    L = _lib.load()
    o = torch.empty((S, 2048, 2), device=DEV)
    assert L.sonde_combine_process(comb.h, C.c_void_p(x.data_ptr()), 2048, 1024, C.c_void_p(o.data_ptr()), 2048, None) != 0
    assert b"row_stride" in L.sonde_last_error()
    assert len(comb.readout()) == 0
    comb.close()


# ---------------------------------------------------------------- the receiver
N_SUB = 24                   # submits of one granule: 3.07 s
RX_BLOCK = 256               # as the CPU fades test: blocks that follow the edges of a 60 ms fade


@pytest.fixture(scope="module")
def fading_antennas():
    """two antennas' wideband streams [n, 2] of one scene: gains of their own, the fade pattern of combine_scenes at the wideband
    rate, noise floors of their own"""
    n = N_SUB * GRANULE
    sc, frames, symbols = _scene(n, 7)
    g = CS.gains(2, 4, equal=False)
    n48 = n * 48_000 // FS
    blocks = []
    for a, starts in enumerate(CS.fade_windows(n48, 2)):
        f48 = torch.from_numpy(CS.fade_gain(n48, starts)).to(DEV)
        idx = (torch.arange(n, device=DEV, dtype=torch.int64) * 48_000) // FS            # the fade's edges at the wideband rate
        blocks.append(_antenna(sc, (f48[idx] * complex(g[a])).to(torch.complex64), 90 + a))
    return blocks, frames, symbols


def _run(rx, blocks, n_sub):
    got = []
    for k in range(n_sub):
        rx.submit([b[k * GRANULE:(k + 1) * GRANULE] for b in blocks])
        f, ant = rx.frames()
        assert np.all(ant == -1) if rx.combine == "coherent" else np.all(ant >= 0)
        assert all(0 <= i < len(rx.sondes) for i, _ in rx.poll())
        got.append(f)
    return np.concatenate(got)


def test_coherent_receiver_equals_a_batch_fed_by_hand_and_delivers_every_frame(fading_antennas):
    blocks, frames, symbols = fading_antennas
    types = [t for _, t in SONDES]
    rx = DiversityReceiver(FS, SONDES, antennas=2, combine="coherent", combine_block=RX_BLOCK)
    assert rx.granule == GRANULE and rx.max_in == GRANULE and rx.combiner.block == RX_BLOCK
    with pytest.raises(SondeError, match="no offsets"):
        rx.offsets(0)
    got = _run(rx, blocks, N_SUB)
    sh = rx.weights(1)
    assert sh.shape == (6144 // RX_BLOCK, 2) and np.allclose(sh.sum(axis=1), 1.0, atol=1e-12)
    # by hand: the same tuners, a combiner, a batch of three channels
    n48 = 6144
    tuners = [SondeTuner(FS, 48_000, [(f, b) for f, _, b in TR.iq48_vfos(SONDES)], GRANULE) for _ in range(2)]
    comb = SondeCombiner(S, 2, 48_000, n48, RX_BLOCK)
    batch = SondeBatch(S, n48, types=np.array(types, dtype=np.uint8), input_kind=_lib.INPUT_IQ)
    stride = int(_lib.load().sonde_row_stride(n48, _lib.INPUT_IQ))
    ant = torch.empty((2 * S, n48, 2), dtype=torch.float32, device=DEV)
    buf = torch.empty((S, stride, 2), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    hand, shares = [], []
    for k in range(N_SUB):
        for a in range(2):
            tuners[a].process(blocks[a][k * GRANULE:(k + 1) * GRANULE], out=ant[a * S:(a + 1) * S], stream=stream)
        comb.process(ant, out=buf, stream=stream)
        batch.submit(buf[:, :n48], stream)
        hand.append(batch.frames())
        r = comb.readout()
        shares.append(np.abs(_cplx(r[r["sonde"] == 0]["w"])[:, :2]) ** 2)
    hand = np.concatenate(hand)
    assert len(got) > 0 and got.tobytes() == hand.tobytes()
    tally = TR.tally(got, types, frames, symbols)
    print("coherent (sent, decoded, .., .., stray):", tally)
    for i, (sent, hit, _, _, stray) in enumerate(tally):
        assert sent >= 3 and hit == sent and stray == 0, (i, tally[i])
    # the weight goes to the antenna that still hears the sonde: in the middle of each antenna's second fade its share is small
    shares = np.concatenate(shares)
    w0, w1 = CS.fade_windows(N_SUB * 6144, 2)
    assert shares[(w0[1] + CS.FADE_SAMPLES // 2) // RX_BLOCK, 0] < 0.05 and shares[(w1[1] + CS.FADE_SAMPLES // 2) // RX_BLOCK, 1] < 0.05
    for tu in tuners:
        tu.close()
    comb.close(); batch.close(); rx.close()


def test_frames_mode_is_what_it_was():
    sc, _, _ = _scene(12 * GRANULE, 7)                       # 1.5 s, no fades: the frame-level pass is not what is tested here
    g = CS.gains(2, 4, equal=False)
    blocks = [_antenna(sc, complex(g[a]), 90 + a) for a in range(2)]
    with pytest.raises(SondeError, match="RS41 sondes only"):
        DiversityReceiver(FS, SONDES, antennas=2, combine="frames")
    with pytest.raises(SondeError, match="RS41 sondes only"):
        DiversityReceiver(FS, SONDES, antennas=2)
    with pytest.raises(SondeError, match="combine must be"):
        DiversityReceiver(FS, SONDES, antennas=2, combine="both")
    only = [SONDES[0]]
    a = DiversityReceiver(FS, only, antennas=2)
    b = DiversityReceiver(FS, only, antennas=2, combine="frames")
    for rx in (a, b):
        assert rx.combine == "frames" and not hasattr(rx, "combiner") and not hasattr(rx, "_ant")       # no combiner created
        assert rx.batch.n_channels == 2 and len(rx.tuners) == 2 and rx._rows.shape[0] == 2
        with pytest.raises(SondeError, match="no weights"):
            rx.weights(0)
    fa, fb = _run(a, blocks, 12), _run(b, blocks, 12)
    assert len(fa) > 0 and fa.tobytes() == fb.tobytes()
    assert a.offsets(0)["offsets"] == b.offsets(0)["offsets"]
    a.close(); b.close()
