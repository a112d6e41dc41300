"""The coherent antenna combiner's host half and its float64 reference (tests/combine_reference.py, DESIGN SPEC 3.14), on the CPU: the
library's weights routine against the reference on designed matrices, the float32 chain of the spec inside the derived bound, the
gain in noise, the fades of a spinning payload (RS41 and DFM, the CPU oracle as decoder) with the variant whose phase leans on
antenna 0, and M10 -- a type the frame-level pass never served -- in plain noise.  Measured figures: profiles/combine_notes.md."""
from __future__ import annotations

import numpy as np
import pytest

import combine_reference as CR
import combine_scenes as CS
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd import combine as cb
from sdrpp_radiosonde_amd.batch import SondeError


# ---------------------------------------------------------------- host half
def test_defaults_and_constants():
    assert cb.defaults(48_000) == CR.BLOCK == _lib.COMBINE_BLOCK == 1024
    hdr = open(_lib.PKG_DIR + "/../include/sonde_abi.h").read()
    assert "#define SONDE_COMBINE_BLOCK 1024 " in hdr and "#define SONDE_COMBINE_MAX_ANTENNAS 4\n" in hdr
    assert "ONE sample clock" in hdr and "START TOGETHER" in hdr          # the coherence condition is said where a host reads it
    with pytest.raises(SondeError, match="rate"):
        cb.defaults(1000)
    w = np.array([0.6, 0.8j])
    assert cb.share(w, 0) == pytest.approx(0.36, abs=1e-15) and cb.share(w, 1) == pytest.approx(0.64, abs=1e-15)


def _of_vectors(vecs, lams):
    """sum lam_k v_k v_k^H over orthonormalised vectors"""
    q, _ = np.linalg.qr(np.array(vecs, np.complex128).T)
    return (q * np.array(lams)) @ np.conj(q.T)


def _matrices():
    rng = np.random.default_rng(5)
    out = []
    for K in (2, 3, 4):
        v = rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K))
        out.append((f"K{K} two close eigenvalues", K, _of_vectors(v, [1.0, 0.999] + [0.1] * (K - 2))))
        out.append((f"K{K} rank one", K, _of_vectors(v, [7.0e4] + [0.0] * (K - 1))))
        out.append((f"K{K} zero", K, np.zeros((K, K), np.complex128)))
        x = rng.standard_normal((K, 1024)) + 1j * rng.standard_normal((K, 1024))
        x[K - 1] = 0.0
        out.append((f"K{K} last antenna zero", K, x @ np.conj(x.T)))
        x[K - 1], x[0] = x[0], 0.0
        out.append((f"K{K} antenna 0 zero", K, x @ np.conj(x.T)))
        x = (rng.standard_normal(K) + 1j * rng.standard_normal(K))[:, None] * np.exp(2j * np.pi * rng.uniform(size=1024)) \
            + 0.5 * (rng.standard_normal((K, 1024)) + 1j * rng.standard_normal((K, 1024)))
        out.append((f"K{K} signal in noise", K, x @ np.conj(x.T)))
        d = np.diag([3.0] * K).astype(np.complex128)
        out.append((f"K{K} equal diagonal (a tie)", K, d))
    return out


def test_weights_routine_equals_the_reference():
    rng = np.random.default_rng(6)
    worst = 0.0
    for name, K, M in _matrices():
        m16 = CR.m16_of(M)
        assert np.allclose(CR.matrix(m16, K), M)
        prevs = [None]
        for _ in range(3):
            p = rng.standard_normal(K) + 1j * rng.standard_normal(K)
            prevs.append(p / np.linalg.norm(p))
        prevs.append(np.eye(K)[K - 1].astype(np.complex128))
        for p in prevs:
            got = cb.weights(m16, p, antennas=K)
            want = CR.weights_ref(K, m16, p)
            worst = max(worst, float(np.max(np.abs(got - want))))
            assert np.max(np.abs(got.real - want.real)) <= 1e-12 and np.max(np.abs(got.imag - want.imag)) <= 1e-12, (name, p, got, want)
            assert abs(np.linalg.norm(got) - 1.0) <= 1e-12, name
            if name == f"K{K} zero":
                # nothing to learn from: the weights hold (after a restart: antenna 0, the lowest index of the tie)
                assert np.array_equal(got, p if p is not None else np.eye(K)[0]), (name, got)
            if p is not None and abs(np.vdot(p, got)) > 0:
                assert abs(np.vdot(p, got).imag) <= 1e-12 and np.vdot(p, got).real > 0           # the phase rule
    print(f"worst |library - reference| over the designed matrices: {worst:.2e}")
    # a tie on the diagonal after a restart starts from the lowest index
    assert np.array_equal(cb.weights(CR.m16_of(np.diag([3.0, 3.0]).astype(np.complex128)), None, antennas=2), [1.0, 0.0])
    with pytest.raises(SondeError, match="antennas"):
        cb.weights(np.zeros(16), None, antennas=5)
    with pytest.raises(SondeError, match="antennas"):
        cb.weights(np.zeros(16), np.ones(1))


def test_weights_find_the_dominant_eigenvector():
    """what the four iterations are for: from the previous block's weights the rule stays on the signal's direction"""
    rng = np.random.default_rng(9)
    for K in (2, 3, 4):
        g = rng.standard_normal(K) + 1j * rng.standard_normal(K)
        x = g[:, None] * np.exp(2j * np.pi * rng.uniform(size=4096)) + 0.7 * (rng.standard_normal((K, 4096)) + 1j * rng.standard_normal((K, 4096)))
        _, W, _ = CR.combine_ref(x, 1024)
        for w in W:
            assert abs(np.vdot(g / np.linalg.norm(g), w)) > 0.995, (K, w)


# ---------------------------------------------------------------- the bounds
@pytest.fixture(scope="module")
def noisy_rows():
    s, _, _ = CS.clean(1, 1, 8192, 3)
    sig, noi = CS.antennas(s, 4, CS.sigma(1, 15.0), 2, equal=False)
    return CS.as_f32((sig + noi)[0])


@pytest.mark.parametrize("K", [2, 3, 4])
def test_float32_chain_of_the_spec_is_within_the_bound(noisy_rows, K):
    x = noisy_rows[:K]
    _, W, _ = CR.combine_ref(x, 1024)
    wf = W.real.astype(np.float32).astype(np.float64) + 1j * W.imag.astype(np.float32).astype(np.float64)
    y, T = CR.apply_ref(x, wf, 1024)
    bnd = CR.apply_bound(T, K)
    y32 = CR.apply_f32(x, wf, 1024)
    assert np.all(np.abs(y32.real - y.real) <= bnd[:, 0]) and np.all(np.abs(y32.imag - y.imag) <= bnd[:, 1])
    mag = np.sum(np.abs(wf[:, :, None].repeat(1024, axis=2).transpose(1, 0, 2).reshape(K, -1)) * np.abs(x), axis=0)
    assert np.all(bnd[:, 0] <= (2 * K + 2) * CR.U * mag) and np.all(bnd[:, 1] <= (2 * K + 2) * CR.U * mag)       # the order the issue names
    assert np.median(np.abs(y)) > 1e5 * np.median(bnd)                   # the bound is not vacuous
    # the bound rejects what it exists for: the conjugate left out, two antennas' weights swapped
    for bad in (np.conj(wf), wf[:, ::-1]):
        yb, _ = CR.apply_ref(x, bad, 1024)
        assert np.mean((np.abs(yb.real - y.real) > bnd[:, 0]) | (np.abs(yb.imag - y.imag) > bnd[:, 1])) > 0.99


def test_stats_bound_rejects_a_block_one_sample_late(noisy_rows):
    M, A = CR.stats_ref(noisy_rows, 1024)
    bnd = CR.bound(A, 1024)
    Ml, _ = CR.stats_ref(np.roll(noisy_rows, -1, axis=1), 1024)
    used = A > 0
    assert np.all(np.abs(Ml - M)[used] > bnd[used])
    assert np.all(np.abs(M[:, 4]) > 1e3 * bnd[:, 4])                     # the cross terms carry signal


# ---------------------------------------------------------------- gain in noise
@pytest.mark.parametrize("K,snr_db", [(2, 0.0), (3, 0.0), (4, 0.0), (2, 6.0), (4, 6.0)])
def test_gain_in_noise(K, snr_db):
    """K equal antennas at a per-antenna SNR of snr_db in the row's band: the output SNR is the sum of the antennas' less at most
    0.2 dB (the estimation loss is about (K - 1) / (L snr) <= 3 / 1024, under 0.02 dB; 0.2 dB covers the scatter of measuring it)"""
    n = 64 * 1024
    s, _, _ = CS.clean(0, 1, n, 4)
    sig, noi = CS.antennas(s, K, np.sqrt(0.5 / 10.0 ** (snr_db / 10.0)), 20 + K)
    sig, noi = sig[0], noi[0]
    _, W, _ = CR.combine_ref(CS.as_f32(sig + noi), 1024)
    wf = W.real.astype(np.float32).astype(np.float64) + 1j * W.imag.astype(np.float32).astype(np.float64)
    ys, _ = CR.apply_ref(sig, wf, 1024)
    yn, _ = CR.apply_ref(noi, wf, 1024)
    snr_a = np.mean(np.abs(sig) ** 2, axis=1) / np.mean(np.abs(noi) ** 2, axis=1)
    out = np.mean(np.abs(ys) ** 2) / np.mean(np.abs(yn) ** 2)
    loss = 10.0 * np.log10(np.sum(snr_a) / out)
    print(f"K {K} at {snr_db} dB: output {10 * np.log10(out):.3f} dB, the sum of the antennas' {10 * np.log10(np.sum(snr_a)):.3f} dB, loss {loss:.3f} dB")
    assert np.all(10.0 * np.log10(snr_a) >= snr_db - 0.1)
    assert loss <= 0.2
    assert np.allclose(np.linalg.norm(W, axis=1), 1.0, atol=1e-12)


# ---------------------------------------------------------------- fades
FADE_L = 256          # the fades are 60 ms: blocks of 5.3 ms follow their edges closely, and give the phase rule many blocks to hold through


@pytest.mark.parametrize("t,channels,seconds", [(0, 5, 6), (1, 2, 3)], ids=["rs41", "dfm"])
def test_fades(t, channels, seconds):
    """K = 2 at Eb/N0 20 dB; each antenna drops to 0.05 of its amplitude for 60 ms windows that never overlap (what it still hears
    there is scatter whose phase moves: combine_scenes).  The combined rows deliver every transmitted frame, each antenna alone loses
    frames, and so does the reference with the phase taken from antenna 0: its output's phase jumps from block to block while
    antenna 0 is in a fade, which is what the phase rule (rho = w_prev^H v) is there to prevent."""
    n = seconds * 48_000 // 2048 * 2048
    s, frames, _ = CS.clean(t, channels, n, 5)
    sig, noi = CS.antennas(s, 2, CS.sigma(t, 20.0), 3 + t, fades=True, equal=False)
    x = CS.as_f32(sig + noi)
    w0, w1 = CS.fade_windows(n, 2)
    assert all(abs(a - b) >= CS.FADE_SAMPLES for a in w0 for b in w1)        # never two antennas at once
    sent, both = CS.delivered(t, np.stack([CR.combine_ref(x[c], FADE_L)[0] for c in range(channels)]), frames)
    _, alone0 = CS.delivered(t, x[:, 0], frames)
    _, alone1 = CS.delivered(t, x[:, 1], frames)
    _, lean0 = CS.delivered(t, np.stack([CR.combine_ref(x[c], FADE_L, phase="antenna0")[0] for c in range(channels)]), frames)
    print(f"type {t}: sent {sent}, combined {both}, antenna 0 alone {alone0}, antenna 1 alone {alone1}, phase from antenna 0 {lean0}")
    assert sent >= 40
    assert both == sent
    assert alone0 < sent and alone1 < sent
    assert lean0 < sent
    # the weight follows the antenna that still hears the sonde
    _, W, _ = CR.combine_ref(x[0], FADE_L)
    share = np.abs(W) ** 2
    mid0, mid1 = (w0[1] + CS.FADE_SAMPLES // 2) // FADE_L, (w1[1] + CS.FADE_SAMPLES // 2) // FADE_L
    assert share[mid0, 0] < 0.02 and share[mid1, 1] < 0.02
    assert 0.3 < share[w0[1] // FADE_L - 2, 0] < 0.8


# ---------------------------------------------------------------- plain noise, a type the frame-level pass never served
M10_E = 10.0          # chosen by the sweep in profiles/combine_notes.md: at 10 dB either antenna alone delivers 4 and 5 of 89 frames, at 11 dB 28 and 33


def test_m10_in_noise():
    """K = 2 equal antennas at E = 10 dB: either antenna alone delivers at most a third of the frames; the combined rows deliver at
    least what one antenna delivers at E + 10 log10(K) - 0.5 dB, less 10 % of the transmitted frames"""
    t, C, n, K = 3, 6, 4 * 48_000 // 2048 * 2048, 2
    s, frames, _ = CS.clean(t, C, n, 8)
    sig, noi = CS.antennas(s, K, CS.sigma(t, M10_E), 11)
    x = CS.as_f32(sig + noi)
    sent, a0 = CS.delivered(t, x[:, 0], frames)
    _, a1 = CS.delivered(t, x[:, 1], frames)
    _, both = CS.delivered(t, np.stack([CR.combine_ref(x[c])[0] for c in range(C)]), frames)
    better = M10_E + 10.0 * np.log10(K) - 0.5
    sig2, noi2 = CS.antennas(s, K, CS.sigma(t, better), 11)
    _, one = CS.delivered(t, CS.as_f32(sig2 + noi2)[:, 0], frames)
    print(f"M10: sent {sent}; at {M10_E} dB antenna 0 alone {a0}, antenna 1 alone {a1}, combined {both}; one antenna at {better:.2f} dB {one}")
    assert sent >= 40
    assert 3 * a0 <= sent and 3 * a1 <= sent
    assert both >= one - 0.1 * sent
