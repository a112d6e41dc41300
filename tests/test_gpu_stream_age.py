"""-m gpu: every kernel that carries an absolute position, at high stream age (DESIGN "Stream age").  The test hooks
sonde_batch_test_shift_age, sonde_tuner_test_set_base and sonde_detect_test_shift_age move an object's origin and leave everything
relative where it is; an aged object B is then fed the same input as an unaged A, across 2^31, 2^32, 2^37, 2^40, 2^47, 2^48 of
whatever the kernel counts.  B's bits, records, loop state and fragments must be A's (positions less the shift), B's per-tile states
go through the float64 replay of tests/demod_reference.py, the tuner's rows are held to tests/tuner_reference.py at the aged index,
the detector's scores to tests/detect_reference.py.  Every stage asserts from what it observed that its boundary was crossed inside
it."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import age_scenes as A
import demod_reference as D
import detect_reference as DR
import tuner_reference as R
from rescue_gpu_harness import run as harness_run
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError
from sdrpp_radiosonde_amd.detect import SondeDetector
from sdrpp_radiosonde_amd.tuner import SondeTuner, tuner_taps
from test_gpu_demod_reference import KIND, replay_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAGS = {"iq": 0, "iq-wide": _lib.FLAG_WIDE, "iq16": 0, "real": 0, "afsk": 0}


# ---------------------------------------------------------------- batch: demodulator, tone front-end, framers
class Pair:
    """an unaged batch A and an aged batch B over the same input, fed submit by submit and compared after every submit"""

    def __init__(self, name: str, submit_tiles: int, flags: int = 0, time_slices: int = 0):
        self.S, self.xs = A.scene_set(name)
        S = self.S
        self.C, self.tin = len(S), A.tile_in(S)
        assert (submit_tiles * D.TILE) % self.tin == 0
        self.step = submit_tiles * D.TILE
        types = np.array([s.stype for s in S], np.uint8)
        mk = lambda: SondeBatch(self.C, A.SUBMIT * D.TILE, types=types, input_kind=KIND[S[0].kind], flags=FLAGS[name] | flags,   # noqa: E731
                                time_slices=time_slices)
        self.a, self.b = mk(), mk()
        self.x = torch.from_numpy(np.stack(self.xs)).to(DEV)
        self.div = [A.div_of(s) for s in S]
        self.fed = 0                                    # input samples per channel so far
        self.samples = [0] * self.C                     # B's shift so far: input samples, internal samples, bits
        self.dn0 = [0] * self.C
        self.added = [0] * self.C
        self.nb = [0] * self.C                          # A's bit count
        self.st_a = [None] * self.C
        self.st_b = [None] * self.C
        self.states = [[] for _ in range(self.C)]       # B's per-submit states with the shift taken off t_next, and its new bits
        self.bits = [[] for _ in range(self.C)]
        self.frames_a = []

    def close(self):
        self.a.close()
        self.b.close()

    def feed(self, submits: int):
        for _ in range(submits):
            blk = self.x[:, self.fed:self.fed + self.step]
            assert blk.shape[1] == self.step, "the scene is too short for this stage"
            self.a.submit(blk)
            self.b.submit(blk)
            self.fed += self.step
            self.compare()

    def compare(self):
        a, b = self.a, self.b
        fa, fb = a.frames(), b.frames()
        why = A.frames_diff(fa, fb, self.added)
        assert not why, why[:3]
        self.frames_a.append(fa)
        assert a.overflow() == 0 and b.overflow() == 0
        pa, pb = a.poll(), b.poll()
        assert [(c, bytes(d)) for c, d in pa] == [(c, bytes(d)) for c, d in pb]
        for c in range(self.C):
            ka, kb = a.nbits(c), b.nbits(c)
            assert kb == ka + self.added[c], (c, ka, kb, self.added[c])
            n = ka - self.nb[c]
            ba = a.read_bits(c, self.nb[c], n) if n else np.zeros(0, np.uint8)
            bb = b.read_bits(c, self.nb[c] + self.added[c], n) if n else np.zeros(0, np.uint8)
            assert np.array_equal(ba, bb), c
            self.nb[c] = ka
            sa, sb = a.state(c), b.state(c)
            why = A.state_diff(sa, sb, self.dn0[c] << 16)
            assert not why, (c, why)
            self.st_a[c], self.st_b[c] = sa, sb
            self.states[c].append(dict(sb, t_next=sb["t_next"] - (self.dn0[c] << 16)))
            self.bits[c].append(bb)

    def shift(self, samples, turns):
        """shift every channel of B; returns the bits added by this shift"""
        got = self.b.test_shift_age(np.arange(self.C), samples, turns)
        for c in range(self.C):
            assert int(samples[c]) % self.div[c] == 0
            self.samples[c] += int(samples[c])
            self.dn0[c] += int(samples[c]) // self.div[c]
            self.added[c] += int(got[c])
        return got

    def n0(self, c: int) -> int:
        """B's internal sample count"""
        return self.fed // self.div[c] + self.dn0[c]

    def t_int(self, c: int) -> int:
        """the whole internal-rate sample of B's next symbol instant, as observed after the last submit"""
        return self.st_b[c]["t_next"] >> 16

    def replay(self, tag: str):
        import dataclasses
        n = len(self.states[0]) * self.step
        S = [dataclasses.replace(s, ntiles=len(self.states[0])) for s in self.S]           # the stretch that was fed
        replay_all(S, [x[:n] for x in self.xs], self.states, self.bits, tag)


def _n0_stage(p: Pair, boundary: int, submits: int):
    """n0 to less than 15 input tiles below `boundary`, then `submits` submits: t_next's integer part crosses `boundary`, t_next itself
    boundary << 16"""
    samples = [A.samples_below(boundary, p.n0(c), p.div[c]) for c in range(p.C)]
    # t_next as the last submit left it, seen from the new origin: it trails n0, so it lies below the boundary as well
    before = [p.st_b[c]["t_next"] + (samples[c] // p.div[c] << 16) for c in range(p.C)]
    p.shift(samples, [0] * p.C)
    for c in range(p.C):
        assert p.n0(c) < boundary and boundary - p.n0(c) <= A.Q // p.div[c]
    p.feed(submits)
    for c in range(p.C):
        assert p.n0(c) > boundary and before[c] >> 16 < boundary <= p.t_int(c), (c, before[c], p.t_int(c))
        assert before[c] < boundary << 16 <= p.st_b[c]["t_next"]


def _per_tile(name: str, flags: int = 0):
    mixed = name != "afsk"
    tiles = 1 if mixed else 8
    per_stage = A.STAGE if mixed else 6
    p = Pair(name, tiles, flags)
    p.feed(A.WARM)
    if not mixed:
        # SdAfskState::n, the tone mixers' phase counter, just below 2^32 input samples (n0 is then about 2^29)
        p.shift([A.samples_below(1 << 32, p.fed + p.samples[c]) for c in range(p.C)], [0] * p.C)
        assert all(0 < (1 << 32) - (p.fed + p.samples[c]) <= A.Q for c in range(p.C))
        p.feed(per_stage)
        assert all(p.fed + p.samples[c] > 1 << 32 for c in range(p.C))
    for boundary in (1 << 31, 1 << 32, 1 << 40):
        _n0_stage(p, boundary, per_stage)
    p.replay(f"aged-{name}")
    p.close()


@pytest.mark.parametrize("name", ["iq", "iq-wide", "iq16", "real", "afsk"])
def test_n0_and_t_next_cross_their_boundaries_tile_by_tile(name):
    """n0 across 2^31, 2^32 and 2^40 (t_next across 2^47, 2^48, 2^56), the AFSK set first with the tone front-end's sample count across
    2^32: B equals A after every tile, and B's every tile passes the float64 replay"""
    _per_tile(name)


def test_n0_stages_with_time_slices():
    """24-tile submits cut into 4 time slices: a slice is to the arithmetic what a submit is, at any age"""
    p = Pair("iq", A.SUBMIT, time_slices=4)
    p.feed(1)
    for boundary in (1 << 31, 1 << 32, 1 << 40):
        _n0_stage(p, boundary, 1)
    p.close()


def test_shift_is_ordered_behind_the_last_submit_and_before_the_next():
    """SONDE_FLAG_LATE_JOIN, launch units on their own streams: submit, shift, submit with nothing in between that waits; the first
    submit must see the old origin, the second the new one"""
    S, xs = A.scene_set("iq")
    C = len(S)
    types = np.array([s.stype for s in S], np.uint8)
    step = A.SUBMIT * D.TILE
    x = torch.from_numpy(np.stack(xs)).to(DEV)
    a = SondeBatch(C, step, types=types, flags=_lib.FLAG_LATE_JOIN)
    b = SondeBatch(C, step, types=types, flags=_lib.FLAG_LATE_JOIN)
    assert b.launch_info()["units"] > 1 and b.launch_info()["join"] == 1
    ring = A.ring_bits(S)
    div = [A.div_of(s) for s in S]
    fed, dn0, added = 0, [0] * C, [0] * C
    for boundary in (1 << 31, 1 << 32):
        blk0, blk1 = x[:, fed:fed + step], x[:, fed + step:fed + 2 * step]
        a.submit(blk0)
        a.submit(blk1)
        b.submit(blk0)
        # the shift is computed from what B will hold once blk0 has run: its sample count is known without waiting for it
        samples = [A.samples_below(boundary, (fed + step) // div[c] + dn0[c], div[c]) for c in range(C)]
        turns = [(boundary >> 20) + c for c in range(C)]
        got = b.test_shift_age(np.arange(C), samples, turns)
        assert [int(v) for v in got] == [t * ring for t in turns]
        b.submit(blk1)
        fed += 2 * step
        t = a.ticket()
        fa0, fa1, fb0, fb1 = a.frames_of(t - 1), a.frames_of(t), b.frames_of(t - 1), b.frames_of(t)
        assert len(fa0) + len(fa1) > C
        assert not A.frames_diff(fa0, fb0, added)                      # the first submit: the old origin
        for c in range(C):
            dn0[c] += samples[c] // div[c]
            added[c] += int(got[c])
        assert not A.frames_diff(fa1, fb1, added)                      # the second: the new one
        for c in range(C):
            assert b.nbits(c) == a.nbits(c) + added[c]
            assert not A.state_diff(a.state(c), b.state(c), dn0[c] << 16), c
            assert b.state(c)["t_next"] >> 16 >= boundary
    a.close()
    b.close()


@pytest.mark.parametrize("boundary", [1 << 32, 1 << 37], ids=["2^32", "2^37"])
@pytest.mark.parametrize("name", ["iq", "iq-wide", "iq16", "real", "afsk"])
def test_wpos_crosses_its_boundary_with_frames_across_it(name, boundary):
    """wpos, rpos, fstart and bitpos across 2^32, and the ring word index (wpos >> 5 as 32 bits) across 2^37, in 24-tile submits:
    bits, records, fragments and state equal A's, and every sonde type has a frame whose bits span the boundary"""
    p = Pair(name, A.SUBMIT)
    p.feed(1)
    ring = A.ring_bits(p.S)
    turns = [A.turns_below(boundary, p.nb[c], ring) for c in range(p.C)]
    got = p.shift([0] * p.C, turns)
    assert all(int(g) == t * ring for g, t in zip(got, turns)), "tests/age_scenes.ring_bits is not the batch's ring"
    before = [p.nb[c] + p.added[c] for c in range(p.C)]
    assert all(0 < boundary - v <= ring for v in before)
    first = len(p.frames_a)
    p.feed(A.submits_to_cross(p.S))
    for c in range(p.C):
        assert before[c] < boundary <= p.b.nbits(c), c
    fa = np.concatenate(p.frames_a[first:])
    want = {s.stype for s in p.S}
    assert A.spanning_types(fa, p.added, boundary) == want, (A.spanning_types(fa, p.added, boundary), want)
    p.close()


def test_refusals():
    S, xs = A.scene_set("iq")
    b = SondeBatch(4, A.SUBMIT * D.TILE)
    with pytest.raises(SondeError, match="nothing has run"):
        b.test_shift_age([0], [0], [0])
    b.submit(torch.zeros((4, 2048, 2), device=DEV))
    for bad in (1, 2048, 480, A.Q + 2048):
        with pytest.raises(SondeError, match="multiple of 30720"):
            b.test_shift_age([0], [bad], [0])
    with pytest.raises(SondeError, match="no such channel"):
        b.test_shift_age([4], [0], [0])
    with pytest.raises(SondeError, match="listed twice"):
        b.test_shift_age([1, 1], [0, 0], [0, 0])
    assert list(b.test_shift_age([0, 2], [A.Q, 0], [0, 3])) == [0, 3 * A.ring_bits([S[0]])]
    b.close()
    g = SondeBatch(4, A.SUBMIT * D.TILE)
    g.set_diversity([[0, 1], [2, 3]])
    g.submit(torch.zeros((4, 2048, 2), device=DEV))
    with pytest.raises(SondeError, match="all members"):
        g.test_shift_age([0], [A.Q], [1])
    with pytest.raises(SondeError, match="same amount"):
        g.test_shift_age([0, 1], [A.Q, 2 * A.Q], [1, 1])
    with pytest.raises(SondeError, match="same amount"):
        g.test_shift_age([0, 1], [A.Q, A.Q], [1, 2])
    g.test_shift_age([0, 1], [A.Q, A.Q], [2, 2])
    g.close()
    from sdrpp_radiosonde_amd.batch import SondeChannelizer
    ch = SondeChannelizer()
    with pytest.raises(SondeError, match="channelizer"):
        ch.batch.test_shift_age([0], [0], [0])
    ch.close()
    tu = SondeTuner(10_000_000, 48_000, [0], 6250)
    for bad in (-625, 1, 624, (1 << 62) + 625):
        with pytest.raises(SondeError, match="n_base"):
            tu.test_set_base(bad)
    tu.test_set_base((1 << 62) // 625 * 625)
    tu.process(torch.zeros((625, 2), device=DEV))
    with pytest.raises(SondeError, match="already"):
        tu.test_set_base(0)
    tu.close()
    tu = SondeTuner(10_000_000, 48_000, [0], 6250)
    tu.retune(0, 1000)
    with pytest.raises(SondeError, match="already"):
        tu.test_set_base(0)
    tu.close()
    det = SondeDetector(2, 2048)
    with pytest.raises(SondeError, match="nothing has run"):
        det.test_shift_age([0], [A.Q])
    det.submit(torch.zeros((2, 2048, 2), device=DEV))
    with pytest.raises(SondeError, match="multiple of 30720"):
        det.test_shift_age([0], [2048])
    with pytest.raises(SondeError, match="listed twice"):
        det.test_shift_age([0, 0], [A.Q, A.Q])
    det.close()


# ---------------------------------------------------------------- batch: the passes that index the ring by bitpos
def _rescue_cases():
    import afsk_rescue_scenes as asc
    import dfm_rescue_scenes as dsc
    import ims_rescue_scenes as isc
    import manchester_rescue_scenes as msc
    import rescue_scenes as rsc
    return {
        "rs41": (lambda: rsc.scene().iq, None, _lib.FLAG_RS41_RESCUE, "rescue_info", rsc.TILE),
        "manchester": (lambda: msc.scene("m10").iq, msc.KINDS["m10"][0], _lib.FLAG_MANCHESTER_RESCUE, "manchester_rescue_info", msc.TILE),
        "dfm": (lambda: dsc.scene_of("designed").iq, dsc.DFM, _lib.FLAG_DFM_RESCUE, "dfm_rescue_info", dsc.TILE),
        "ims": (lambda: isc.scene_of("designed").iq, isc.IMS, _lib.FLAG_IMS_RESCUE, "ims_rescue_info", isc.TILE),
        "afsk": (lambda: asc.scene_of("imet").iq, asc.IMET4, _lib.FLAG_AFSK_RESCUE, "afsk_rescue_info", 8 * asc.TILE),
    }


def _cuts(n: int, tile: int) -> int:
    """the most equal submits (at most 6) the scene divides into"""
    return max(k for k in range(1, 7) if n % (k * tile) == 0)


@pytest.mark.parametrize("boundary", [1 << 32, 1 << 37], ids=["2^32", "2^37"])
@pytest.mark.parametrize("which", ["rs41", "manchester", "dfm", "ims", "afsk"])
def test_rescue_passes_across_the_boundary(which, boundary):
    """each rescue pass's own designed scene through rescue_gpu_harness, cut into submits.  A bit count moves by whole ring turns
    only, and the scenes are about a ring long, so the scene is fed several times over (the damaged frames with it) and the shift is
    placed behind the first submit after which every channel still crosses the boundary with rescued frames beyond it.  The records
    (less the shift) and the counters are those of the unaged run, and the unaged run rescues frames beyond the boundary: the pass ran
    on positions on both sides of it."""
    get, stype, flag, info, tile = _rescue_cases()[which]
    one = torch.from_numpy(get()).to(DEV)
    C, n = one.shape[0], one.shape[1]
    cuts = _cuts(n, tile)
    ring = A.ring_bits_of([D.modem(stype or 0)], n // cuts)
    per_pass = int(n // (D.modem(stype or 0).pre * D.modem(stype or 0).decim) * 65536 // D.modem(stype or 0).period0)
    passes = 1 + -(-ring // per_pass)
    iq = torch.cat([one] * passes, dim=1).contiguous()
    kw = dict(tile=tile, keep=True)
    if stype is not None:
        kw["types"] = np.full(C, stype, np.uint8)
    parts_a, nb_a = [], []

    def watch(b_, k):
        parts_a.append(b_.frames())
        nb_a.append([b_.nbits(c) for c in range(C)])

    fa, a = harness_run(iq, flag, cuts * passes, after_submit=watch, **kw)
    # where to shift: the first submit behind which every channel crosses and a rescued record lies wholly beyond the boundary
    where = None
    for k in range(len(parts_a) - 1):
        turns = [A.turns_below(boundary, nb_a[k][c], ring) for c in range(C)]
        later = np.concatenate(parts_a[k + 1:])
        res = later[later["flags"] & _lib.FRAME_RESCUED != 0]
        beyond = sum(int(f["bitpos"]) + turns[int(f["channel"])] * ring >= boundary for f in res)
        below = sum(int(f["bitpos"]) + turns[int(f["channel"])] * ring < boundary for f in res)
        if all(nb_a[-1][c] + turns[c] * ring > boundary for c in range(C)) and beyond and below:
            where = (k, turns)
            break
    assert where is not None, "no submit behind which the boundary is crossed with rescued frames on both sides"
    added = [0] * C

    def shift(b_, k):
        if k == where[0]:
            got = b_.test_shift_age(np.arange(C), [0] * C, where[1])
            for c in range(C):
                added[c] = int(got[c])
                assert added[c] == where[1][c] * ring, "tests/age_scenes.ring_bits_of is not the batch's ring"
                assert 0 < boundary - (nb_a[k][c] + added[c]) <= ring

    fb, b = harness_run(iq, flag, cuts * passes, after_submit=shift, **kw)
    fb = fb.copy()
    add = np.asarray([added[int(c)] for c in fb["channel"]], np.uint64)
    old = fb["bitpos"] < add                                           # the records from before the shift: at the old origin
    fb["bitpos"][old] += add[old]
    why = A.frames_diff(fa, fb, added)
    assert not why, why[:3]
    assert sum(getattr(a, info)(c)["rescued"] for c in range(C)) > 0
    for c in range(C):
        assert getattr(b, info)(c) == getattr(a, info)(c), c
        assert b.nbits(c) == a.nbits(c) + added[c] > boundary
    a.close()
    b.close()


@pytest.mark.parametrize("boundary", [1 << 32, 1 << 37], ids=["2^32", "2^37"])
@pytest.mark.parametrize("mode", ["offsets", "learn_mark"])
def test_diversity_across_the_boundary(mode, boundary):
    """the standard scene of diversity_scenes (two-member groups, a three-member group), fed twice over in 10 submits each (with
    offsets unknown the three-member group locks late in the first pass), every member shifted by the same amount once the two- and
    the three-member group have combined a frame, so that a carried record exists and must move:
    combined records, duplicate marks, diversity_info and diversity_offsets equal the unaged run's, and every member crosses"""
    import diversity_scenes as dsc
    sc = dsc.scene()
    iq = torch.from_numpy(sc.iq).to(DEV)
    iq = torch.cat([iq, iq], dim=1).contiguous()
    C, n, cuts = sc.C, 2 * sc.n, 20
    step = n // cuts
    ring = A.ring_bits_of([D.modem(0)], step)
    kw = dict(offsets=sc.offsets) if mode == "offsets" else dict(offsets=None, learn=True, mark_duplicates=True)

    def run(shift_after=None):
        b = SondeBatch(C, step)
        b.set_diversity(sc.groups, window_bits=sc.window, **kw)
        parts, added = [], 0
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            parts.append((b.frames(), [added] * C))
            if k == shift_after:
                turns = A.turns_below(boundary, max(b.nbits(c) for c in range(C)), ring)
                got = b.test_shift_age(np.arange(C), [0] * C, [turns] * C)
                assert all(int(g) == turns * ring for g in got)
                added = turns * ring
        return b, parts, added

    a, pa, _ = run()
    comb = [{int(c) for c in f["channel"][f["flags"] & _lib.FRAME_COMBINED != 0]} for f, _ in pa]
    two = {c for g in sc.groups if len(g) == 2 for c in g}
    three = {c for g in sc.groups if len(g) == 3 for c in g}
    # the first submit by which a two-member group and the three-member group have each combined a frame (with offsets unknown only
    # the groups that see a frame good in two members lock at all)
    k0 = next(k for k in range(cuts) if any(c in two for s in comb[:k + 1] for c in s) and any(c in three for s in comb[:k + 1] for c in s))
    assert any(comb[k0 + 1:]), "no frame is combined behind the shift"
    b, pb, added = run(shift_after=k0)
    for k, ((fa, _), (fb, add)) in enumerate(zip(pa, pb)):
        why = A.frames_diff(fa, fb, add)
        assert not why, (k, why[:3])
    if mode == "learn_mark":
        assert sum(int((f["flags"] & _lib.FRAME_DUPLICATE != 0).sum()) for f, _ in pa[k0 + 1:]) > 0
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == a.diversity_info(g), g
        assert b.diversity_offsets(g) == a.diversity_offsets(g), g
    for c in range(C):
        assert b.nbits(c) == a.nbits(c) + added > boundary, c
    a.close()
    b.close()


# ---------------------------------------------------------------- tuner
T_IQ, T_IQ16, T_IQ8 = _lib.INPUT_IQ, _lib.INPUT_IQ16, _lib.INPUT_IQ8
TUNER_CFG = [          # (Fs, R, B, offsets at both band edges and near 0, input kind, two ragged submits in units of `down`)
    (20_000_000, 48_000, 40_000, [-9_979_999, 9_980_000, 7], T_IQ, [43, 36]),
    (10_000_000, 48_000, 40_000, [-4_980_000, 4_979_999, -3], T_IQ16, [57, 100]),
    (2_400_000, 48_000, 0, [-1_176_000, 1_175_999, 1], T_IQ, [3000, 997]),
]
DT = {T_IQ: torch.float32, T_IQ16: torch.int16, T_IQ8: torch.int8}


def _stream(fs, n, kind, seed, tones=None):
    """integer-valued complex samples (exact in every kind): noise plus tones, by default near 0 and inside both band-edge VFOs"""
    rng = np.random.default_rng(seed)
    a = 40.0 if kind == T_IQ8 else 3000.0
    t = np.arange(n)
    x = a * 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for amp, f in tones or ((0.3, 3_234), (0.2, -fs // 2 + 30_000), (0.2, fs // 2 - 30_000)):
        x = x + a * amp * np.exp(2j * np.pi * (f * t / fs + rng.uniform()))
    x = np.round(x)
    return x, torch.from_numpy(np.stack([x.real, x.imag], axis=1)).to(DT[kind]).to(DEV)


def _bases(down: int, first: int, total: int):
    """the four ages: the largest multiple of `down` that puts 2^31 / 2^32 inside the first submit, 2^40, 2^62 less the submits"""
    b31, b32 = ((1 << 31) - 1) // down * down, ((1 << 32) - 1) // down * down
    assert b31 < 1 << 31 <= b31 + first and b32 < 1 << 32 <= b32 + first
    return [b31, b32, (1 << 40) // down * down, ((1 << 62) - total) // down * down]


@pytest.mark.parametrize("cfg", TUNER_CFG, ids=[f"{c[0]}-k{c[4]}" for c in TUNER_CFG])
def test_tuner_rows_within_the_bound_at_high_n_base(cfg):
    fs, r, bw, offs, kind, subs = cfg
    up, down = R.ratio(fs, r)
    n = sum(subs) * down
    assert n <= 200_000
    x, dev = _stream(fs, n, kind, seed=fs % 991 + 5)
    g = tuner_taps(fs, r, bw).astype(np.float64)
    for base in _bases(down, subs[0] * down, n):
        tu = SondeTuner(fs, r, [(f, bw) for f in offs], max(subs) * down, input_kind=kind)
        tu.test_set_base(base)
        got, a = [], 0
        for k in subs:
            got.append(tu.process(dev[a:a + k * down].contiguous()).cpu().numpy().copy())
            a += k * down
        got = np.concatenate(got, axis=1)
        tu.close()
        for k, f in enumerate(offs):
            y, Ab = R.tuner_ref(x, fs, r, g, [f] * len(subs), [s * down for s in subs], start=base)
            bnd = R.bound(Ab, g.shape[1])
            gk = got[k, :, 0] + 1j * got[k, :, 1]
            assert len(gk) == len(y) == n * up // down
            dev_re, dev_im = np.abs(gk.real - y.real), np.abs(gk.imag - y.imag)
            assert np.all(dev_re <= bnd) and np.all(dev_im <= bnd), (base, k, float(np.max(np.maximum(dev_re, dev_im) / bnd)))
            assert np.max(np.abs(y)) > 100.0 * np.max(bnd)          # the rows carry signal: the bound is not vacuous


def test_tuner_rows_bit_identical_at_a_base_that_keeps_every_phase():
    """n_base a multiple of lcm(Fs, down): the mixer's phase and the filter's phase are those of a fresh tuner, so the rows are too,
    bit for bit, slots and both integer input kinds included"""
    fs, r, b = 10_000_000, 48_000, 10_000
    up, down = R.ratio(fs, r)
    assert fs % down == 0
    offs = [(-2_345_678, b), (17_001, 0), (4_970_000, 20_000)]
    subs = [1, 13, 100, 7, 30]
    n = sum(subs) * down
    _, d16 = _stream(fs, n, T_IQ16, seed=3)
    dflt = d16.to(torch.float32)

    def rows(base, kind, dev, slots=False):
        if slots:
            tu = SondeTuner.slots(fs, r, 4, [b, 20_000, 0], max(subs) * down, input_kind=kind)
        else:
            tu = SondeTuner(fs, r, offs, max(subs) * down, input_kind=kind)
        if base:
            tu.test_set_base(base)
        if slots:
            for k, (f, bw) in enumerate(offs):
                tu.slot_set(k + 1 if k else 0, f, bw)          # slots 0, 2, 3 active, slot 1 idle
        out, a = [], 0
        for k in subs:
            out.append(tu.process(dev[a:a + k * down].contiguous()).cpu().numpy().copy())
            a += k * down
        tu.close()
        return np.concatenate(out, axis=1).view(np.uint32)

    fresh = rows(0, T_IQ, dflt)
    for base in (fs * 215, fs * ((1 << 40) // fs), fs * ((1 << 62) // fs - 1)):          # 2.15e9: between 2^31 and 2^32
        assert np.array_equal(rows(base, T_IQ, dflt), fresh), base
        assert np.array_equal(rows(base, T_IQ16, d16), fresh), base
    _, d8 = _stream(fs, n, T_IQ8, seed=4)
    fresh8 = rows(0, T_IQ, d8.to(torch.float32))
    assert fresh8.any() and np.array_equal(rows(fs * ((1 << 32) // fs), T_IQ8, d8), fresh8)
    fresh_slots = rows(0, T_IQ, dflt, slots=True)
    assert fresh_slots[[0, 2, 3]].any() and not fresh_slots[1].any()
    assert np.array_equal(rows(fs * ((1 << 40) // fs), T_IQ, dflt, slots=True), fresh_slots)


@pytest.mark.parametrize("continuous", [False, True], ids=["plain", "continuous"])
def test_tuner_retune_with_the_first_submit_across_2_32(continuous):
    """test_retune_between_submits' plan (and the continuous one), the tuner's base such that 2^32 lies inside the first submit; the
    reference's plan carries theta' = (theta + (f_old - f_new)(n0 - T / 2)) mod Fs in exact integers at the aged n0"""
    fs, r = 2_400_000, 20_000
    up, down = R.ratio(fs, r)
    subs = [40, 40, 40]
    plan = [[-500_000, -500_000, 31_234], [100_003, 700_000, 700_000]]
    n = sum(subs) * down
    x, dev = _stream(fs, n, T_IQ, seed=9, tones=((0.4, 31_234), (0.4, 700_000), (0.3, -500_000), (0.3, 100_003)))
    base = ((1 << 32) - 1) // down * down
    assert base < 1 << 32 <= base + subs[0] * down
    tu = SondeTuner(fs, r, [p[0] for p in plan], max(subs) * down)
    tu.test_set_base(base)
    g = tuner_taps(fs, r).astype(np.float64)
    T = g.shape[1]
    thetas = [[0], [0]]
    got, a = [], 0
    for s, k in enumerate(subs):
        for v in range(2):
            th = thetas[v][-1]
            if s and plan[v][s] != plan[v][s - 1]:
                tu.retune(v, plan[v][s], continuous=continuous)
                th = (th + ((plan[v][s - 1] - plan[v][s]) % fs) * ((base + a - T // 2) % fs)) % fs if continuous else 0
            if s:
                thetas[v].append(th)
        got.append(tu.process(dev[a:a + k * down].contiguous()).cpu().numpy())
        a += k * down
    got = np.concatenate(got, axis=1)
    tu.close()
    assert not continuous or any(any(t) for t in thetas)
    for v in range(2):
        y, Ab = R.tuner_ref(x, fs, r, g, plan[v], [k * down for k in subs], start=base, thetas=thetas[v])
        gk = got[v, :, 0] + 1j * got[v, :, 1]
        bnd = R.bound(Ab, T)
        assert np.all(np.abs(gk.real - y.real) <= bnd) and np.all(np.abs(gk.imag - y.imag) <= bnd), v
        assert np.max(np.abs(y)) > 100.0 * np.max(bnd)


# ---------------------------------------------------------------- detector
N_DET, CUT_DET = 98304, 32768          # test_gpu_detect's clip, cut behind 16 tiles: the crossing lies in the second submit's first 15


@functools.lru_cache(maxsize=None)
def _detect_rows(C_per: int):
    rows = []
    for t in range(7):
        kw = {} if t in (DR.IMET4, DR.C50) else dict(cfo_max_hz=2000.0)
        rows.append(synth.make_batch(t, C_per, N_DET, seed=700 + t, ebn0_db=30.0, **kw).iq)
    return torch.cat(rows).contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def _detect_unaged(C_per: int):
    rows = _detect_rows(C_per)
    det = SondeDetector(rows.shape[0], N_DET - CUT_DET)
    det.submit(rows[:, :CUT_DET])
    det.submit(rows[:, CUT_DET:])
    res = det.results()
    streams = [det.read(c) for c in range(rows.shape[0])]
    det.close()
    return res, streams


@pytest.mark.parametrize("boundary", [1 << 32, 1 << 33, 1 << 35], ids=["n:2^32", "n/2:2^32", "n/8:2^32"])
def test_detector_crosses_its_boundaries_inside_a_submit_with_a_sync(boundary):
    C_per = 32
    rows = _detect_rows(C_per)
    C = rows.shape[0]
    want, streams = _detect_unaged(C_per)
    det = SondeDetector(C, N_DET - CUT_DET)
    det.submit(rows[:, :CUT_DET])
    shift = A.samples_below(boundary, CUT_DET)
    assert CUT_DET + shift < boundary <= CUT_DET + shift + A.Q
    det.test_shift_age(np.arange(C), [shift] * C)
    det.submit(rows[:, CUT_DET:])
    got = det.results()
    assert np.array_equal(got["type"], want["type"]) and np.array_equal(got["inverted"], want["inverted"])
    assert np.array_equal(got["best"], want["best"])                   # the exact doubles
    assert np.array_equal(got["pos"] - np.uint64(shift), want["pos"])   # every type of every channel has a match by now
    assert (want["best"] > 0).all()
    for c in range(C):
        for u, v in zip(det.read(c), streams[c]):
            assert np.array_equal(u, v), c
    det.close()
    # a winning sync of every type lies behind the boundary, in the submit in which n crossed
    for t in range(7):
        assert (got["pos"][C_per * t:C_per * (t + 1), t] >= np.uint64(boundary)).any(), t
        assert (got["type"][C_per * t:C_per * (t + 1)] == t).all(), t


def test_detector_at_2_40_equals_the_reference():
    C_per = 2
    rows = _detect_rows(C_per)
    C = rows.shape[0]
    det = SondeDetector(C, N_DET - CUT_DET)
    det.submit(rows[:, :CUT_DET])
    first = [det.read(c) for c in range(C)]
    shift = A.samples_below(1 << 40, CUT_DET)
    det.test_shift_age(np.arange(C), [shift] * C)
    det.submit(rows[:, CUT_DET:])
    got = det.results()
    for c in range(C):
        Ds, Ai, Ac = (np.concatenate([u, v]).astype(np.int64) for u, v in zip(first[c], det.read(c)))
        best, inv, pos = DR.detect_streams(Ds, Ai, Ac)
        assert np.array_equal(got["best"][c], best), c
        assert np.array_equal(got["pos"][c] - np.uint64(shift), pos), c
        assert np.array_equal(got["inverted"][c], inv), c
        assert got["type"][c] == DR.decide(best) == c // C_per, c
    assert (got["pos"] >= np.uint64(shift)).all() and shift + CUT_DET > (1 << 40) - A.Q
    det.close()
