"""CPU checks of the sonde type detector's SPEC: the library's templates against tests/detect_reference.py, the
score's algebra, a slice of the threshold study, the SondeDetection layout, and mutations of the reference that must fail."""
from __future__ import annotations

import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import detect_reference as R
from sdrpp_radiosonde_amd import _lib, detect, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N2S = 96000


def brute_r(D, s):
    """Pearson correlation of s with every window of D, from its definition in float64"""
    D = np.asarray(D, np.float64)
    L = len(s)
    out = []
    for t in range(len(D) - L + 1):
        w = D[t:t + L]
        dw, ds = w - w.mean(), s - s.mean()
        den = math.sqrt((dw * dw).sum() * (ds * ds).sum())
        out.append(0.0 if (dw * dw).sum() == 0 else (dw * ds).sum() / den)
    return np.array(out)



@pytest.mark.parametrize("t", range(7))
def test_library_templates_equal_reference(t):
    got = detect.templates(t)
    want = R.template(t)
    assert got.dtype == np.int8 and np.array_equal(got.astype(np.int64), want), t
    assert len(want) == {0: 320, 1: 154, 2: 240, 3: 80, 4: 60, 5: 53, 6: 240}[t]


def test_thresholds_equal_reference():
    assert np.array_equal(detect.thresholds(), R.THETA)


def test_detection_struct_layout_matches_header():
    S = _lib.SondeDetection
    assert (S.type.offset, S.inverted.offset, S.best.offset, S.pos.offset, C.sizeof(S)) == (0, 4, 8, 64, 120)
    assert _lib.DETECTION_DTYPE.itemsize == 120
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/llvm/bin/clang"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sonde_abi.h"\nint main(void){printf("%zu %zu %zu %zu %zu", '
           'offsetof(SondeDetection, type), offsetof(SondeDetection, inverted), offsetof(SondeDetection, best), '
           'offsetof(SondeDetection, pos), sizeof(SondeDetection)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.c"), "w") as f:
            f.write(src)
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "l"), os.path.join(d, "l.c")])
        out = subprocess.check_output([os.path.join(d, "l")]).decode().split()
    assert [int(v) for v in out] == [0, 4, 8, 64, 120]


def test_scores_equal_their_definition():
    rng = np.random.default_rng(3)
    for t in (R.DFM09, R.M10, R.C50):
        s = R.template(t)
        D = rng.integers(-9000, 9000, size=len(s) + 300)
        assert np.allclose(R.scores(D, s), brute_r(D, s), rtol=0, atol=1e-12)


def test_score_is_invariant_to_offset_and_gain_and_exact_on_the_template():
    rng = np.random.default_rng(4)
    for t in range(7):
        s = R.template(t)
        D = rng.integers(-3000, 3000, size=len(s) + 500)
        r = R.scores(D, s)
        assert np.array_equal(R.scores(D + 777, s), r)                 # the centred sums are exact integers
        assert np.array_equal(R.scores(4 * D - 123, s), r)             # a power-of-two gain scales N^2 and Ed alike, exactly
        assert np.allclose(R.scores(3 * D, s), r, rtol=1e-15, atol=0)
        assert R.scores(s, s)[0] == 1.0 and R.scores(-s, s)[0] == -1.0
        assert R.scores(5 * s + 9, s)[0] == 1.0
        assert not R.scores(np.zeros(len(s) + 40, np.int64), s).any()
        assert not R.scores(np.full(len(s) + 40, -1234), s).any()
        assert R.best_of(R.scores(np.zeros(len(s) + 40, np.int64), s)) == (0.0, False, 0)


def test_best_takes_the_earliest_of_equal_scores():
    s = R.template(R.M10)
    D = np.concatenate([np.zeros(7, np.int64), s, np.zeros(50, np.int64), s, np.zeros(9, np.int64)])
    b, neg, t = R.best_of(R.scores(D, s))
    assert (b, neg, t) == (1.0, False, 7)


def _rows(t, C, seed, ebn0=30.0, invert=False):
    kw = {} if t in (R.IMET4, R.C50) else dict(cfo_max_hz=2000.0, invert=invert)
    return synth.make_batch(t, C, N2S, seed=seed, ebn0_db=ebn0, **kw).iq.numpy()


def test_threshold_study_slice_holds():
    """a small slice of DESIGN 3.8's study (other seeds): no foreign signal nor noise reaches theta_k; every channel is its type"""
    rng = np.random.default_rng(77)
    for _ in range(4):                                     # 8 channel-seconds of complex AWGN
        x = rng.standard_normal((N2S, 2)).astype(np.float32)
        typ, best, _, _ = R.detect_rows(x, False)
        assert typ == -1 and (best < R.THETA).all(), best
    for t in range(7):
        for inv in ((False, True) if t not in (R.IMET4, R.C50) else (False,)):
            for row in _rows(t, 2, 900 + t, invert=inv):
                typ, best, flags, _ = R.detect_rows(row, False)
                foreign = np.delete(best, t) < np.delete(R.THETA, t)
                assert typ == t and foreign.all(), (t, inv, best)
                if t != R.IMS100:
                    assert flags[t] == inv


# ---------------------------------------------------------------- mutations of the reference must fail
def test_mutation_template_off_by_one_chip_fails():
    for t in range(7):
        assert not np.array_equal(R.template(t, chip_off=1), detect.templates(t).astype(np.int64)), t


def test_mutation_floor_instead_of_ceil_fails():
    for t in (R.DFM09, R.C50):                 # chip rates that do not divide the stream rate
        assert not np.array_equal(R.template(t, ceil_mode="floor"), detect.templates(t).astype(np.int64)), t


def test_mutation_short_window_fails():
    rng = np.random.default_rng(5)
    s = R.template(R.RS41)
    D = rng.integers(-9000, 9000, size=len(s) + 100)
    assert not np.allclose(R.scores(D, s, short=True)[:101], brute_r(D, s), atol=1e-6)


def test_mutation_ed_without_s1_fails():
    rng = np.random.default_rng(6)
    s = R.template(R.DFM09)
    D = rng.integers(-2000, 6000, size=len(s) + 100)
    assert not np.allclose(R.scores(D, s, ed_no_s1=True), brute_r(D, s), atol=1e-6)


def test_mutation_afsk_phase_reset_per_submit_fails():
    """a mixer restarted at every submit turns z by a step at each boundary: q jumps there by more than the bound"""
    rows = _rows(R.IMET4, 1, 31)[0]
    sub = [2048] * (N2S // 2048) + ([N2S % 2048] if N2S % 2048 else [])
    _, qi, qc = R.front_end(rows, False)
    Ai_m, Ac_m = R.quantised_streams(rows, False, submits=sub, phase_reset=True)[1:]
    for A, q, (bound, ok) in zip((Ai_m, Ac_m), (qi, qc), R.afsk_bound(rows, False)):
        assert (np.abs(R.wrap_diff(A, R.QSTEP * q)) > bound)[ok].sum() >= len(sub) // 2
