"""The sonde type detector on the GPU (DESIGN SPEC 3.8) against tests/detect_reference.py: front-end error bounds, exact scores on
the product's own quantised streams, submit boundaries, classification, masks and reset, detect-then-decode, refusals."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import detect_reference as R
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError
from sdrpp_radiosonde_amd.detect import SondeDetector

pytestmark = pytest.mark.gpu

N2 = 98304                 # 48 tiles: a 2-s clip
DEV = "cuda:0"
# 12 dB (Eb/N0 for GFSK, C/N in 48 kHz for AFSK): channels of 32 per type the float64 reference detects with these seeds
# (DESIGN 3.8); the GPU's front-end differs from the float64 one by the atan2q approximation, hence a margin of 3 per type
RATE12 = {0: 32, 1: 0, 2: 0, 3: 30, 4: 32, 5: 32, 6: 0}
RATE12_MARGIN = 3


def _synth(t, C, seed, ebn0=30.0, invert=False):
    kw = {} if t in (R.IMET4, R.C50) else dict(cfo_max_hz=2000.0, invert=invert)
    sb = synth.make_batch(t, C, N2, seed=seed, ebn0_db=ebn0, **kw)        # on the CPU: the noise of the seeds DESIGN quotes
    sb.iq = sb.iq.to(DEV)
    return sb


def _as_kind(iq: torch.Tensor, kind: int) -> torch.Tensor:
    if kind == _lib.INPUT_IQ16:
        return torch.clamp(torch.round(iq * 8000.0), -32767, 32767).to(torch.int16)
    if kind == _lib.INPUT_IQ8:
        return torch.clamp(torch.round(iq * 60.0), -127, 127).to(torch.int8)
    return torch.round(iq * 256.0) / 256.0          # float rows whose 2:1 boxcar sums are exact


def _run(rows, kind=_lib.INPUT_IQ, chunks=None, mask=None, read=False):
    C, n = rows.shape[0], rows.shape[1]
    chunks = chunks or [n]
    det = SondeDetector(C, max(chunks), input_kind=kind, type_mask=mask)
    streams = [([], [], []) for _ in range(C)] if read else None
    s0 = 0
    for k in chunks:
        det.submit(rows[:, s0:s0 + k])
        if read:
            for c in range(C):
                for lst, a in zip(streams[c], det.read(c)):
                    lst.append(a.astype(np.int64))
        s0 += k
    res = det.results()
    det.close()
    if read:
        streams = [tuple(np.concatenate(x) for x in st) for st in streams]
    return res, streams


def _mixed_rows(C_per=2, seed=40):
    rows, truth = [], []
    for t in range(7):
        rows.append(_synth(t, C_per, seed + t).iq)
        truth += [t] * C_per
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    rows.append(torch.randn((2, N2, 2), generator=g, device=DEV))
    rows.append(torch.zeros((2, N2, 2), device=DEV))
    truth += [-1] * 4
    return torch.cat(rows).contiguous(), np.array(truth)


# ---------------------------------------------------------------- 1. front-end bounds
@pytest.mark.parametrize("kind", [_lib.INPUT_IQ, _lib.INPUT_IQ16, _lib.INPUT_IQ8, _lib.INPUT_REAL])
def test_front_end_within_bounds(kind):
    n = 16384
    iq = torch.cat([_synth(t, 1, 70 + t).iq[:, :n] for t in (R.RS41, R.IMET4, R.C50, R.M10)])
    if kind == _lib.INPUT_REAL:
        rows = torch.from_numpy(np.stack([np.round(R.disc(R.as_complex(x)) * 8192) / 8192 for x in iq.cpu().numpy()])).float().to(DEV)
    else:
        rows = _as_kind(iq, kind)
    _, st = _run(rows.contiguous(), kind, chunks=[8192, 8192], read=True)
    host = rows.cpu().numpy()
    for c in range(rows.shape[0]):
        D, Ai, Ac = st[c]
        d2, qi, qc = R.front_end(host[c], kind == _lib.INPUT_REAL)
        if kind == _lib.INPUT_REAL:
            assert np.array_equal(D, R.quantise(d2))                    # exact sums of exact inputs: the same integers
        else:
            assert np.abs(R.wrap_diff(D, R.QSTEP * d2)).max() <= R.gfsk_bound()
        for A, q, (bound, ok) in zip((Ai, Ac), (qi, qc), R.afsk_bound(host[c], kind == _lib.INPUT_REAL)):
            assert ok.mean() > 0.9
            err = np.abs(R.wrap_diff(A, R.QSTEP * q))
            assert (err <= bound)[ok].all(), (c, float((err - bound)[ok].max()))


# ---------------------------------------------------------------- 2. exact scores
def _check_exact(res, streams, mask=None):
    for c, (D, Ai, Ac) in enumerate(streams):
        best, inv, pos = R.detect_streams(D, Ai, Ac)
        assert np.array_equal(res["best"][c], best), (c, res["best"][c] - best)
        assert np.array_equal(res["pos"][c], pos), c
        assert np.array_equal(res["inverted"][c], inv), c
        assert res["type"][c] == R.decide(best, 0x7F if mask is None else int(mask[c])), c


def test_scores_equal_the_integer_reference_bit_for_bit():
    rows, truth = _mixed_rows()
    res, st = _run(rows, chunks=[49152, 49152], read=True)
    _check_exact(res, st)
    assert (res["type"] == truth).all()


# ---------------------------------------------------------------- 3. submit boundaries
def test_submit_boundaries_do_not_matter():
    rows, _ = _mixed_rows(seed=50)
    one, _ = _run(rows)
    small, _ = _run(rows, chunks=[2048] * (N2 // 2048))
    wide = torch.zeros((rows.shape[0], N2 + 4096, 2), device=DEV)
    wide[:, :N2] = rows
    ragged, _ = _run(wide[:, :N2], chunks=[6144, 2048, 20480, 10240, 59392])
    for r in (small, ragged):
        for key in ("type", "best", "pos", "inverted"):
            assert np.array_equal(one[key], r[key]), key
    # at least one winning sync straddled a 2048-sample boundary
    straddle = 0
    for c in range(rows.shape[0]):
        t = one["type"][c]
        if t >= 0:
            p, span = int(one["pos"][c][t]), len(R.template(t)) * R.DEC[t]
            straddle += p // 2048 != (p + span - 1) // 2048
    assert straddle > 0


# ---------------------------------------------------------------- 4. classification
def _sync_sample_positions(sb, t, c):
    """sample index (k + tau) fs / baud of every place the type's sync chips occur in the transmitted stream of channel c"""
    pat = np.array(R.sync_chips(t), np.uint8)
    bits = np.asarray(sb.bits[c], np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(bits, len(pat))
    hit = (win == pat).all(axis=1)
    if t == R.IMS100:                      # biphase-S: either level
        hit |= (win == 1 - pat).all(axis=1)
    k = np.flatnonzero(hit)
    return (k + sb.tau[c]) * (R.FS / R.BAUD[t])


@pytest.mark.parametrize("kind", [_lib.INPUT_IQ, _lib.INPUT_IQ16, _lib.INPUT_IQ8])
def test_classification_at_30_db(kind):
    C = 32
    for t in range(7):
        for inv in ((False, True) if t not in (R.IMET4, R.C50) else (False,)):
            sb = _synth(t, C, 300 + 10 * t + inv, invert=inv)
            res, _ = _run(_as_kind(sb.iq, kind).contiguous(), kind)
            assert (res["type"] == t).all(), (t, inv, res["type"])
            if t != R.IMS100:
                assert (res["inverted"][:, t] == inv).all(), (t, inv)
            sps = R.FS / R.BAUD[t]
            for c in range(C):
                cand = _sync_sample_positions(sb, t, c)
                assert np.abs(cand - float(res["pos"][c][t])).min() <= sps, (t, c)
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    noise = torch.randn((32, N2, 2), generator=g, device=DEV)
    rows = torch.cat([_as_kind(noise, kind), _as_kind(torch.zeros((4, N2, 2), device=DEV), kind)]).contiguous()
    res, _ = _run(rows, kind)
    assert (res["type"] == -1).all()
    assert (res["best"][32:] == 0).all()


def test_classification_at_12_db_misses_but_never_errs():
    for t in range(7):
        sb = _synth(t, 32, 1200 + t, ebn0=12.0)
        res, _ = _run(sb.iq.contiguous())
        got = res["type"]
        assert ((got == t) | (got == -1)).all(), (t, got)
        assert (got == t).sum() >= RATE12[t] - RATE12_MARGIN, (t, int((got == t).sum()))


# ---------------------------------------------------------------- 5. mask and reset
def test_mask_and_reset():
    rows, truth = _mixed_rows(seed=60)
    C = rows.shape[0]
    mask = np.full(C, 0x7F, np.uint8)
    rng = np.random.default_rng(1)
    for c in range(C):
        if truth[c] >= 0:
            mask[c] &= ~np.uint8(1 << truth[c])                 # the true type masked out
        mask[c] &= ~np.uint8(1 << int(rng.integers(0, 7)))
    res, st = _run(rows, mask=mask, read=True)
    _check_exact(res, st, mask)
    for c in range(C):
        assert res["type"][c] < 0 or (mask[c] >> res["type"][c]) & 1
    det = SondeDetector(C, N2)
    other, _ = _mixed_rows(seed=61)
    det.submit(other)
    det.results()
    det.reset()
    det.submit(rows)
    again = det.results()
    det.close()
    fresh, _ = _run(rows)
    for key in ("type", "best", "pos", "inverted"):
        assert np.array_equal(again[key], fresh[key]), key


# ---------------------------------------------------------------- 6. detect, then decode
def test_detect_then_decode():
    rows, truth = _mixed_rows(C_per=3, seed=80)
    keep = truth >= 0
    perm = np.random.default_rng(2).permutation(int(keep.sum()))
    rows = rows[torch.from_numpy(np.flatnonzero(keep)[perm]).to(DEV)].contiguous()
    truth = truth[keep][perm]
    res, _ = _run(rows)
    assert (res["type"] == truth).all()

    def frames(types):
        b = SondeBatch(rows.shape[0], N2, types=types.astype(np.uint8))
        b.submit(rows, torch.cuda.current_stream().cuda_stream)
        f = b.frames()
        b.close()
        return f

    got, want = frames(res["type"]), frames(truth)
    assert len(want) > 0 and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    L = _lib.load()
    import ctypes as C
    h = C.c_void_p()
    assert L.sonde_detect_create(4, 4096, 7, None, 0, C.byref(h)) < 0 and _lib.last_error()
    assert L.sonde_detect_create(4, 3000, 0, None, 0, C.byref(h)) < 0
    assert L.sonde_detect_create(0, 4096, 0, None, 0, C.byref(h)) < 0
    assert L.sonde_detect_create(4, 4096, 0, None, 0, None) < 0
    with pytest.raises(SondeError, match="sonde_detect_create: no such HIP device"):
        SondeDetector(4, 4096, device=torch.cuda.device_count())
    det = SondeDetector(4, 4096)
    x = torch.zeros((4, 8192, 2), device=DEV)
    p = C.c_void_p(x.data_ptr())
    assert L.sonde_detect_submit(None, p, 2048, 8192, None) < 0
    assert L.sonde_detect_submit(det.h, None, 2048, 8192, None) < 0
    assert L.sonde_detect_submit(det.h, p, 3000, 8192, None) < 0 and "SONDE_TILE" in _lib.last_error()
    assert L.sonde_detect_submit(det.h, p, 8192, 8192, None) < 0          # > max_samples
    assert L.sonde_detect_submit(det.h, p, 4096, 2048, None) < 0          # stride too small
    assert L.sonde_detect_results(det.h, None, 4) < 0
    assert L.sonde_detect_read(det.h, 9, None, None, None) < 0
    assert L.sonde_detect_templates(7, None, 0) < 0
    assert L.sonde_detect_thresholds(None) < 0
    with pytest.raises(SondeError):
        det.submit(torch.zeros((4, 2048), device=DEV))
    with pytest.raises(SondeError):
        SondeDetector(4, 4096, type_mask=np.zeros(3, np.uint8))
    det.submit(x[:, :4096])
    assert (det.results()["type"] == -1).all()
    det.close()
