"""Stage 3 of RS41 on the GPU (the sync search K4 of sd_rs41.h in its plain form and in the four-chunk register form of
bins_kernel.hip, the frame-length decision, de-whitening K5 and RS(255,231) K6 of sd_rsdec.h, in the tile loop, in the epilogue and as
sd_rsdec_rs41_kernel) against the independent reference of tests/framer_reference.py (type 0, written from DESIGN SPEC 3.3), on the
designed streams of tests/framer_streams.py (rs41_streams).  The scheme is test_gpu_framer_reference.py's: for every channel the bits
the GPU produced (collected after every submit) go through reference(), and the result must equal the GPU's frame records of that
channel, concatenated over the submits, byte for byte; the demodulated bits over every planted frame and decoy must equal the planted
ones, no channel may overflow, the plan of every stream must hold on the GPU's records and every decision the streams were built for
is counted on those records (framer_streams.required_coverage_rs41): a path that was not taken fails the test.  No frame is left out
but each channel's first, and no comparison has a tolerance.

Launch shapes, all on the same designed rows: one submit of 144 tiles (the in-loop decoder, see IN_LOOP_TILES below, and descriptors
beyond the 8th from HBM), submits of 24 tiles (the epilogue alone), tile-sized submits (every frame, header and length byte cut by a
submit boundary, extended frames over 20 submits, the bit ring wrapping), SONDE_FLAG_SPLIT_FEC, forced time slices, SONDE_FLAG_WIDE
(the 2:1 modem in front of the same framer), and the rows interleaved with DFM and M10 rows: under default flags (the one-launch
mixed kernel), and pipelined and late-joined, where the RS41 rows are a launch unit of their own, unsliced and sliced, with the frames
fetched by ticket.  One test is on noise: RS41 bins of the
channelizer at four levels, fused and unfused, with the header-distance and gap streams planted in six more bins."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import torch

import framer_reference as R
import framer_streams as S
from sdrpp_radiosonde_amd._lib import FLAG_LATE_JOIN, FLAG_PIPELINE, FLAG_SPLIT_FEC, FLAG_WIDE
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeChannelizer

pytestmark = pytest.mark.gpu
TILE = 2048
SD_K4_LIST = 8                       # csrc/sd_rs41.h: frames of a launch whose descriptors stay in LDS


@pytest.fixture(scope="module")
def state():
    """what the tests of this file share (the scene on the device, the wideband scene, the reference's results per distinct input)"""
    st: dict = {}
    yield st
    st.clear()
    torch.cuda.empty_cache()


class Scene:
    """every designed RS41 stream in one batch, the rows of the streams interleaved"""

    def __init__(self):
        self.names = sorted(S.rs41_streams())
        self.streams = [S.rs41_streams()[nm]() for nm in self.names]
        rows = [(k, c) for k, d in enumerate(self.streams) for c in range(d.iq.shape[0])]
        perm = np.random.default_rng(41).permutation(len(rows))
        self.rows = [rows[i] for i in perm]                              # batch row -> (stream, channel of the stream)
        self.n = S.NT * TILE
        iq = torch.empty((len(self.rows), self.n, 2), dtype=torch.float32)
        for r, (k, c) in enumerate(self.rows):
            iq[r] = self.streams[k].iq[c]
        for d in self.streams:
            d.iq = d.iq[:0]
        self.dev = iq.cuda()
        self.ref = {}


def scene(state) -> Scene:
    if "scene" not in state:
        state["scene"] = Scene()
    return state["scene"]


def reference(sc: Scene, bits: np.ndarray, row: int, info=None) -> np.ndarray:
    """reference() once per distinct input: the launch shapes mostly produce the same bits"""
    key = (row, hashlib.sha1(bits.tobytes()).digest())
    if key not in sc.ref:
        inf = {}
        sc.ref[key] = (R.reference(R.RS41, bits, row, info=inf), inf)
    if info is not None:
        info.update(sc.ref[key][1])
    return sc.ref[key][0]


def _by_row(frames: np.ndarray, nrows: int):
    frames = frames[np.lexsort((frames["bitpos"], frames["channel"]))]
    cut = np.searchsorted(frames["channel"], np.arange(nrows + 1))
    return [frames[cut[r]:cut[r + 1]] for r in range(nrows)]


def run(x: torch.Tensor, step: int, flags: int = 0, time_slices: int = 0, types=None):
    """submit the rows `step` samples at a time: (bits per row, records per row, most frames one submit listed for a row)"""
    C, n = x.shape[0], x.shape[1]
    b = SondeBatch(C, step, types=types, flags=flags, time_slices=time_slices)
    bits = [[] for _ in range(C)]
    nb = [0] * C
    parts, most = [], 0
    for off in range(0, n, step):
        b.submit(x[:, off:off + step].contiguous())
        fr = b.frames()
        parts.append(fr)
        if len(fr):
            most = max(most, int(np.bincount(fr["channel"]).max()))
        for c in range(C):
            k = b.nbits(c)
            if k > nb[c]:
                bits[c].append(b.read_bits(c, nb[c], k - nb[c]))
                nb[c] = k
    assert b.overflow() == 0
    b.close()
    bits = [np.concatenate(v) if v else np.zeros(0, np.uint8) for v in bits]
    return bits, _by_row(np.concatenate(parts), C), most


def verify(sc: Scene, bits, recs, tag: str, rows=None):
    """rows: the batch rows that hold the scene's rows 0, 1, .. (None: the batch is the scene)"""
    cover, nrec, pending = {}, 0, 0
    for i, (k, c) in enumerate(sc.rows):
        r = i if rows is None else rows[i]
        d = sc.streams[k]
        info = {}
        ref = reference(sc, bits[r], r, info)
        assert len(ref) == len(recs[r]) and ref.tobytes() == recs[r].tobytes(), (tag, d.name, c, len(ref), len(recs[r]))
        off, pol = S.check_conditions(d, c, bits[r])
        S.check_plan(d, c, recs[r], off, pol, cover)
        want = [e["pos"] + off for e in d.plan[c] if e.get("pending")]
        assert ([info["pending"]] if "pending" in info else []) == want, (tag, d.name, c, info, want)
        pending += "pending" in info
        nrec += len(ref)
    missing = [q for q in S.required_coverage_rs41(sc.names) if q not in cover]
    assert not missing, (tag, len(missing), missing[:10])
    assert pending >= 2, (tag, pending)
    print(f"FRAMER-REF gpu rs41 {tag}: rows={len(sc.rows)} records={nrec} streams={len(sc.names)} coverage keys={len(cover)} pending={pending}")
    return nrec


# Which launches decode clean frames INSIDE the tile loop (sd_rs41_loop_step): there is no public indicator of it.  The gate is in
# csrc/demod_kernel.hip:
#     const bool fec_loop = fec_here && n_tiles >= 48 && grid_wg <= fo->loop_fec_max_wg && !sliced;
# (fec_here: not SONDE_FLAG_SPLIT_FEC; loop_fec_max_wg: one residency of the GPU, far above this scene's few dozen workgroups).  So the
# one-submit shape (144 tiles, unsliced) takes the in-loop decoder for the clean frames among the first SD_K4_LIST of the launch and
# hands the dirty ones and all later ones to the epilogue; submits of 24 tiles and of one tile, sliced launches and SPLIT_FEC never do.
# That "the in-loop decoder ran" rests on this reading of the gate, not on an observation.
IN_LOOP_TILES = S.NT
assert IN_LOOP_TILES >= 48


def test_one_submit_in_loop_decoder_and_hbm_descriptors(state):
    sc = scene(state)
    bits, recs, most = run(sc.dev, IN_LOOP_TILES * TILE)
    verify(sc, bits, recs, "one-submit")
    assert most > SD_K4_LIST                       # the 9th and later frames of a launch: descriptors from HBM
    for i, (k, c) in enumerate(sc.rows):           # the first frame was found too, so "dirty as 8th / 9th / 11th of the launch" is what the order stream says
        if sc.streams[k].name == "rs41-order":
            assert len(recs[i]) == 11, (c, len(recs[i]))


def test_submits_of_24_tiles(state):
    """the epilogue alone (below the in-loop decoder's 48 tiles)"""
    sc = scene(state)
    bits, recs, most = run(sc.dev, 24 * TILE)
    verify(sc, bits, recs, "24-tile submits")
    assert most <= SD_K4_LIST


def test_tile_sized_submits(state):
    """2048-sample submits: every frame, every header and every length byte is cut by a submit boundary in some row; an extended
    frame spans 20 submits; the batch is created for one tile, so its bit ring wraps many times"""
    sc = scene(state)
    bits, recs, _ = run(sc.dev, TILE)
    verify(sc, bits, recs, "2048-sample submits")


def test_split_fec_kernel(state):
    """sd_rsdec_rs41_kernel (SONDE_FLAG_SPLIT_FEC), two submit sizes"""
    sc = scene(state)
    for step in (sc.n // 2, 8 * TILE):
        bits, recs, _ = run(sc.dev, step, flags=FLAG_SPLIT_FEC)
        verify(sc, bits, recs, f"split-fec step {step}")


@pytest.mark.parametrize("slices", [2, 5])
def test_forced_time_slices(state, slices):
    """segments of a submit as workgroups of their own (an RS41-only batch with default flags is one launch and takes
    SondeBatchConfig.time_slices as told): nout0 and the hand-over between segments, in submits of 144 and of 48 tiles"""
    sc = scene(state)
    for step in (sc.n, sc.n // 3):
        assert slices <= step // TILE
        bits, recs, _ = run(sc.dev, step, time_slices=slices)
        verify(sc, bits, recs, f"time-slices x{slices} step {step}")


def mixed(sc: Scene, state):
    """the RS41 rows interleaved with designed DFM and M10 rows: (IQ on the device, types, batch row of every scene row)"""
    if "mixed" not in state:
        others = [S.all_streams()[nm]() for nm in ("sync-1-norm", "sync-3-norm")]
        extra = torch.cat([d.iq for d in others]).cuda()
        types_extra = np.concatenate([np.full(d.iq.shape[0], d.stype, dtype=np.uint8) for d in others])
        C = len(sc.rows) + len(types_extra)
        where = np.random.default_rng(43).permutation(C)                # batch row of scene row i: where[i]; of extra row j: where[len + j]
        x = torch.empty((C, sc.n, 2), dtype=torch.float32, device="cuda")
        x[torch.from_numpy(where).cuda()] = torch.cat([sc.dev, extra])
        types = np.zeros(C, dtype=np.uint8)
        types[where[len(sc.rows):]] = types_extra
        state["mixed"] = (x, types, where[:len(sc.rows)])
    return state["mixed"]


# Which batches have launch units (csrc/batch.hip, sonde_batch_create; no public indicator): with SONDE_FLAG_PIPELINE / SONDE_FLAG_LATE_JOIN a
# batch of ONE sonde type below 512 channels stays one plain launch (`one_class_units` = 1, `need_lists` false: no unit is made), so the
# RS41 rows alone would never reach launch_unit_demod.  A batch of several types gets one unit per type: the RS41 rows run as a unit of
# their own through the channel list (`d_chlist[type] + u.off`), on the unit's stream with its join, with launch_decoders per unit.
# Hence the mixed rows here; forced time slices in the same batch give sliced units.
@pytest.mark.parametrize("slices", [0, 2], ids=["unsliced", "sliced"])
@pytest.mark.parametrize("flags", [FLAG_PIPELINE, FLAG_LATE_JOIN], ids=["pipeline", "late-join"])
def test_frames_by_ticket_in_launch_units(state, flags, slices):
    """the RS41 rows as a launch unit of their own beside a DFM and an M10 unit: three submits queued back to back, the frames fetched
    per ticket; the bits of all three are read afterwards (the batch is created for the whole length, so its ring holds them) and go
    through reference().  Only the RS41 rows are checked here."""
    sc = scene(state)
    x, types, where = mixed(sc, state)
    step = sc.n // 3
    C = x.shape[0]
    b = SondeBatch(C, sc.n, types=types, flags=flags, time_slices=slices)
    st = torch.cuda.current_stream().cuda_stream
    b.ticket()
    parts = []
    for k in range(3):
        b.submit(x[:, k * step:(k + 1) * step].contiguous(), st)
        if k >= 1:
            parts.append(b.frames_of(k))
    parts.append(b.frames_of(3))
    recs = _by_row(np.concatenate(parts), C)
    assert b.overflow() == 0
    bits = [b.read_bits(r, 0, b.nbits(r)) if types[r] == 0 else None for r in range(C)]
    b.close()
    verify(sc, bits, recs, f"tickets in launch units flags={flags} time_slices={slices}", rows=where)


def test_wide_modem(state):
    """SONDE_FLAG_WIDE: the 2:1 modem in front of the same framer (tests/test_framer_reference.py checks the conditions behind it on
    the CPU)"""
    sc = scene(state)
    bits, recs, _ = run(sc.dev, 24 * TILE, flags=FLAG_WIDE)
    verify(sc, bits, recs, "wide")


def test_mixed_batch_with_dfm_and_m10_rows(state):
    """the RS41 rows interleaved with designed DFM and M10 rows under default flags: the one-launch mixed kernel.  Only the RS41 rows
    are checked here (the others are test_gpu_framer_reference.py's)"""
    sc = scene(state)
    x, types, where = mixed(sc, state)
    for step in (sc.n, 24 * TILE):
        bits, recs, _ = run(x, step, types=types)
        verify(sc, bits, recs, f"mixed batch step {step}", rows=where)


BIN_HZ = 10_000_000 / 512
# (bin, Eb/N0 dB): from mostly failing to mostly clean.  The levels come from a CPU run of the oracle's bins path on this scene
# (or_chan_block2 and one oracle channel per bin, tests/test_channelizer.py _oracle_decode_wideband, composite and 48 kS/s rows alike;
# the scene built on the CPU, so with the CPU generator's noise samples instead of the GPU generator's), where reference() equalled
# the oracle in every bin and the planted rows met their conditions and plans.  Codewords clean / corrected / rejected seen there:
#     9.0 dB: 0 / 0 / 20     10.5 dB: 0 / 18 / 0     12.0 dB: 5 / 13 / 0     14.0 dB: 17 / 1 / 0     (all: 22 / 32 / 20)
# The scene the test builds (the same signals, the GPU generator's noise; building it on the host takes two minutes) gave, fused and
# unfused alike, as the test prints per bin:
#     9.0 dB: 0 / 0 / 20     10.5 dB: 0 / 18 / 0     12.0 dB: 2 / 16 / 0     14.0 dB: 18 / 0 / 0     (all: 20 / 34 / 20)
WB_RS41 = [(9, 9.0), (60, 10.5), (333, 12.0), (480, 14.0)]
# (bin, designed stream, its channel) at 40 dB: all header distances (four rows) and all gaps (two rows)
WB_PLANTED = [(150, "rs41-header", 0), (190, "rs41-header", 1), (230, "rs41-header", 2), (290, "rs41-header", 3), (260, "rs41-gaps", 0), (410, "rs41-gaps", 1)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_channelizer_bins(state, fused):
    """RS41 bins of a noisy wideband scene behind the channelizer (the REG form of the sync search in bins_kernel.hip: four chunks of
    64 candidates and the straight-line fast path), against reference() per bin; clean, corrected and rejected codewords must all occur.
    Six more bins carry designed rows (header distances, gaps: hits in every lane and at the fast path's bounds); their plan must
    hold.  Levels and the codewords the oracle's bins path saw at each: 9.0 dB 0 / 0 / 20, 10.5 dB 0 / 18 / 0, 12.0 dB 5 / 13 / 0, 14.0 dB
    17 / 1 / 0 (clean / corrected / rejected); in the scene this test builds, with the GPU generator's noise: 0 / 0 / 20, 0 / 18 / 0, 2 / 16 / 0,
    18 / 0 / 0 (see WB_RS41)."""
    from sdrpp_radiosonde_amd import synth
    types = np.zeros(512, dtype=np.uint8)
    chz = SondeChannelizer(types=types, blocks_per_submit=1, fused=fused)
    assert chz.fused == fused
    blk = chz.samples_per_submit
    nblk = -(-S.NT * TILE * 10_000_000 // 48000 // blk)                 # the designed rows' 6.1 s
    made = {nm: S.rs41_streams()[nm]() for nm in sorted({nm for _, nm, _ in WB_PLANTED})}
    planted = [(k, made[nm], c) for k, nm, c in WB_PLANTED]
    sondes = [((k if k < 256 else k - 512) * BIN_HZ, 0) for k, _ in WB_RS41] + [((k if k < 256 else k - 512) * BIN_HZ, 0) for k, _, _ in planted]
    if "wb" not in state:
        state["wb"] = synth.make_wideband_scene(sondes, nblk * blk, ebn0_db=[e for _, e in WB_RS41] + [40.0] * len(planted), seed=78, device="cuda:0",
                                                bits=[None] * len(WB_RS41) + [np.concatenate([d.chips[c], np.arange(256, dtype=np.uint8) & 1]) for _, d, c in planted])[0]
    iq = state["wb"]
    watch = [k for k, _ in WB_RS41] + [k for k, _, _ in planted]
    bits = {k: [] for k in watch}
    nb = {k: 0 for k in watch}
    parts = []
    for i in range(nblk):
        chz.submit(iq[i * blk:(i + 1) * blk].contiguous())
        parts.append(chz.frames())
        for k in watch:
            n = chz.batch.nbits(k)
            if n > nb[k]:
                bits[k].append(chz.batch.read_bits(k, nb[k], n - nb[k]))
                nb[k] = n
    assert chz.batch.overflow() == 0
    chz.close()
    recs = _by_row(np.concatenate(parts), 512)
    assert sum(len(recs[k]) for k in range(512)) == sum(len(recs[k]) for k in watch)
    seen, noisy, per_level = [0, 0, 0], {k for k, _ in WB_RS41}, {}
    for k in watch:
        ref = R.reference(R.RS41, np.concatenate(bits[k]), k)
        assert len(ref) == len(recs[k]) and ref.tobytes() == recs[k].tobytes(), (fused, k, len(ref), len(recs[k]))
        if k in noisy:                                                   # the planted rows do not count towards what the noise must bring
            per_level[k] = [int((ref["nerr"] == 0).sum()), int((ref["nerr"] > 0).sum()), int((ref["nerr"] < 0).sum())]
            seen = [a + v for a, v in zip(seen, per_level[k])]
    cover = {}
    for k, d, c in planted:
        b = np.concatenate(bits[k])
        off, pol = S.check_conditions(d, c, b)
        S.check_plan(d, c, recs[k], off, pol, cover)
    print(f"FRAMER-REF gpu rs41 channelizer fused={fused}: bins={len(watch)} records={sum(len(recs[k]) for k in watch)} "
          f"codewords of the noisy bins clean / corrected / rejected {seen} (per bin {per_level}) coverage keys={len(cover)}")
    assert min(seen) > 0, seen
    missing = [q for q in [(R.RS41, "header-distance", h, 0) for h in S.RS41_HEADER_DISTANCES] + [(R.RS41, "gap", g, 0) for g in S.RS41_GAPS] if q not in cover]
    assert not missing, missing
