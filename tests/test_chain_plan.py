"""The block arithmetic the three receivers share (sdrpp_radiosonde_amd/_chain.py): the granules, worked out by integer arithmetic
from the formulas the receivers carried before they shared them and equal to the constants the GPU tests pin; the refusals; the
one 40 kHz constant.  No GPU: the library is loaded for sonde_tuner_ratio / sonde_vfo_ratio only."""
from __future__ import annotations

import pytest

from sdrpp_radiosonde_amd import _chain, live, scan, tuner
from sdrpp_radiosonde_amd._lib import C50, DFM09, IMET4, IMS100, M10, MRZN1, RS41
from sdrpp_radiosonde_amd.batch import VFO_RATE, SondeError

GFSK = [RS41, DFM09, M10]


@pytest.mark.parametrize("rate_in, types, granule, n48", [
    (1_000_000, GFSK, 128_000, 6_144),
    (1_000_000, [RS41, IMET4], 1_024_000, 49_152),
    (1_000_000, [C50], 1_024_000, 49_152),
    (1_000_000, GFSK + [IMS100, MRZN1, IMET4, C50], 1_024_000, 49_152),
    (2_400_000, [RS41], 102_400, 2_048),
    (10_000_000, [RS41], 1_280_000, 6_144),
    (10_000_000, [RS41, IMET4], 10_240_000, 49_152),
])
def test_iq48_granules(rate_in, types, granule, n48):
    p = _chain.plan(rate_in, types)
    assert (p.granule, p.max_in, p.n48) == (granule, granule, n48)
    assert p.groups == {48000: list(range(len(types)))}
    assert p.tile == (16384 if IMET4 in types or C50 in types else 2048) and p.n48 % p.tile == 0
    p3 = _chain.plan(rate_in, types, 3 * granule)
    assert (p3.granule, p3.max_in, p3.n48) == (granule, 3 * granule, 3 * n48)
    assert _chain.out48(rate_in, granule) == n48


@pytest.mark.parametrize("types, track, granule", [
    (GFSK, False, 128_000),
    (GFSK, True, 256_000),
    ([RS41], True, 128_000),
])
def test_reference_granules(types, track, granule):
    p = _chain.plan(1_000_000, types, None, "reference", track)
    assert p.granule == p.max_in == granule
    assert p.groups == {VFO_RATE[t]: [i] for i, t in enumerate(types)}          # one tuner per distinct VFO rate, in order of appearance


def test_reference_groups_share_a_tuner_per_rate():
    p = _chain.plan(1_000_000, [IMS100, RS41, MRZN1], None, "reference")
    assert p.groups == {20000: [0, 2], 10000: [1]}


def test_max_in_must_be_a_multiple_of_the_granule():
    with pytest.raises(SondeError, match=r"max_in must be a multiple of the granule \(128000\)"):
        _chain.plan(1_000_000, GFSK, 128_001)


@pytest.mark.parametrize("noun", ["block", "blocks"])
def test_check_block(noun):
    text = rf"the {noun} must hold a positive multiple of the granule \(128000\) samples, at most max_in \(256000\)"
    for n in (128_000, 256_000):
        _chain.check_block(n, 128_000, 256_000, noun)
    for n in (0, 1, 127_999, 192_000, 384_000):          # nothing, no multiple (three ways), more than max_in
        with pytest.raises(SondeError, match=text):
            _chain.check_block(n, 128_000, 256_000, noun)


def test_one_bandwidth_constant():
    assert scan.DETECT_BW is live.PROBE_BW is _chain.IQ48_MAX_BW is tuner.IQ48_MAX_BW
    assert _chain.IQ48_MAX_BW == 40_000
    assert _chain.iq48_bandwidth(M10) == 40_000
    for t in VFO_RATE:
        if t != M10:
            assert _chain.iq48_bandwidth(t) == VFO_RATE[t]


def test_the_names_the_arithmetic_had_in_tuner_stay():
    assert tuner.ratio is _chain.ratio and tuner._lcm is _chain.lcm and tuner._multiple_for is _chain.multiple_for
    assert tuner.ratio(1_000_000, 48_000) == (6, 125)
