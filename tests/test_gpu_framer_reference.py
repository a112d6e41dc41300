"""Stage 3 of the six non-RS41 sonde types on the GPU (sd_fixed.h, framer2_kernel.hip, afsk.hip and their callers in demod_kernel.hip
and bins_kernel.hip) against the independent reference of tests/framer_reference.py, on the designed streams of
tests/framer_streams.py.  For every channel the bits the GPU produced (collected after every submit) go through reference(), and the
result must equal the GPU's frame records of that channel, concatenated over the submits, byte for byte: no frame is left out and the
GPU need not be bit-exact to the oracle.  The demodulated chips over every planted frame must equal the planted ones, no channel may
overflow, the plan of every stream must hold on the GPU's records, and every decision path the streams were built for is counted on
those records (framer_streams.required_coverage): a path that was not taken fails the test.

Launch shapes: one submit of 6.1 s (descriptors from the LDS list and, from the 9th frame of a launch on, from HBM), tile-sized
submits (frames and syncs cut by submit boundaries), SONDE_FLAG_SPLIT_FEC (the sync and decode kernels of their own), forced time
slices in the batch configurations that the library really slices (see SLICED below), pipelined and late-joined submits with the
frames fetched by ticket, the other modem class (SONDE_FLAG_WIDE_AUTO), and the
channelizer's bins (the four-chunk register form of the sync search in bins_kernel.hip), fused and unfused.

The wideband test works on whatever errors the noise brings (the scene builder takes no planted chips): it requires that corrected
and rejected frames both occur and cannot reach the designed paths (a given word in a given lane, padding roots, S1 = 0, planted
syncs); M10 does not fit a bin, and the AFSK types run in bins only unfused and are left to the batch shapes."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import torch

import framer_reference as R
import framer_streams as S
from sdrpp_radiosonde_amd._lib import FLAG_LATE_JOIN, FLAG_PIPELINE, FLAG_SPLIT_FEC, FLAG_WIDE_AUTO
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeChannelizer

pytestmark = pytest.mark.gpu
TILE = 2048
SD_K4_LIST = 8                       # csrc: frames of a launch whose descriptors stay in LDS


@pytest.fixture(scope="module")
def state():
    """what the tests of this file share (the scene on the device, the verified one-submit launch, the wideband scene, the reference's
    results per distinct input): freed when the file is done"""
    st: dict = {"ref": {}}
    yield st
    st.clear()
    torch.cuda.empty_cache()


class Scene:
    """every designed stream in one batch, the rows of the streams interleaved"""

    def __init__(self):
        names = sorted(S.all_streams())
        self.streams = [S.all_streams()[nm]() for nm in names]
        rows = [(k, c) for k, d in enumerate(self.streams) for c in range(d.iq.shape[0])]
        perm = np.random.default_rng(7).permutation(len(rows))
        self.rows = [rows[i] for i in perm]                              # batch row -> (stream, channel of the stream)
        self.types = np.array([self.streams[k].stype for k, _ in self.rows], dtype=np.uint8)
        self.n = S.NT * TILE
        iq = torch.empty((len(self.rows), self.n, 2), dtype=torch.float32)
        for r, (k, c) in enumerate(self.rows):
            iq[r] = self.streams[k].iq[c]
        for d in self.streams:
            d.iq = d.iq[:0]
        self.dev = iq.cuda()
        self.names = names


def scene(state) -> Scene:
    if "scene" not in state:
        state["scene"] = Scene()
        state["scene"].ref = state["ref"]
    return state["scene"]


def reference(sc: Scene, stype: int, bits: np.ndarray, row: int) -> np.ndarray:
    """reference() once per distinct input: the launch shapes mostly produce the same bits"""
    key = (stype, row, hashlib.sha1(bits.tobytes()).digest())
    if key not in sc.ref:
        sc.ref[key] = R.reference(stype, bits, row)
    return sc.ref[key]


def _by_row(frames: np.ndarray, nrows: int):
    frames = frames[np.lexsort((frames["bitpos"], frames["channel"]))]
    cut = np.searchsorted(frames["channel"], np.arange(nrows + 1))
    return [frames[cut[r]:cut[r + 1]] for r in range(nrows)]


def run(sc: Scene, rows, step: int, flags: int = 0, time_slices: int = 0):
    """submit the chosen rows `step` samples at a time: (bits per row, records per row, most frames one submit listed for a row)"""
    sel = torch.from_numpy(np.asarray(rows))
    x = sc.dev[sel.cuda()] if len(rows) != len(sc.rows) else sc.dev
    C = len(rows)
    b = SondeBatch(C, step, types=sc.types[rows], flags=flags, time_slices=time_slices)
    bits = [[] for _ in range(C)]
    nb = [0] * C
    parts, most = [], 0
    for off in range(0, sc.n, step):
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


def verify(sc: Scene, rows, bits, recs, tag: str, coverage: bool = True):
    cover, nrec, taken = {}, 0, set()
    for i, r in enumerate(rows):
        k, c = sc.rows[r]
        d = sc.streams[k]
        ref = reference(sc, d.stype, bits[i], i)
        assert len(ref) == len(recs[i]) and ref.tobytes() == recs[i].tobytes(), (tag, d.name, c, len(ref), len(recs[i]))
        off, pol = S.check_conditions(d, c, bits[i])
        S.check_plan(d, c, recs[i], off, pol, cover)
        info = {}
        if d.stype in (S.IMET, S.C50):
            R.afsk_packets(d.stype, bits[i], info=info)
            for why in info["drops"]:
                cover[(d.stype, "drop", why)] = 1
        nrec += len(ref)
        taken.add(d.name)
    if coverage:
        req = S.required_coverage(taken) + (S.required_drops() if "imet-cases" in taken else [])
        missing = [q for q in req if q not in cover]
        assert not missing, (tag, len(missing), missing[:10])
    print(f"FRAMER-REF gpu {tag}: rows={len(rows)} records={nrec} streams={len(taken)} coverage keys={len(cover)}")
    return nrec


def _rows(sc: Scene, types):
    return [r for r in range(len(sc.rows)) if sc.types[r] in types]


GFSK = (S.DFM, S.IMS, S.M10, S.MRZ)
ALL = GFSK + (S.IMET, S.C50)


def test_one_submit_lds_and_hbm_descriptors(state):
    sc = scene(state)
    rows = _rows(sc, ALL)
    bits, recs, most = run(sc, rows, sc.n)
    verify(sc, rows, bits, recs, "one-submit")
    assert most > SD_K4_LIST                       # the 9th and later frames of a launch: descriptors from HBM
    for t in ALL:
        assert max(len(recs[r]) for r in range(len(recs)) if sc.types[r] == t) > SD_K4_LIST, t


def test_tile_sized_submits(state):
    """2048-sample submits for the GFSK rows: every frame and many syncs are cut by a submit boundary, `collecting` is carried over"""
    sc = scene(state)
    rows = _rows(sc, GFSK)
    bits, recs, _ = run(sc, rows, TILE)
    verify(sc, rows, bits, recs, "2048-sample submits")


def test_granule_sized_submits_with_afsk_rows(state):
    sc = scene(state)
    rows = _rows(sc, ALL)
    bits, recs, _ = run(sc, rows, 8 * TILE)
    verify(sc, rows, bits, recs, "16384-sample submits")


def test_split_fec_kernels(state):
    """sd_sync_fixed_kernel + sd_dec_fixed_kernel (the LDS-staged ring, 32 offsets per lane), two submit sizes"""
    sc = scene(state)
    rows = _rows(sc, ALL)
    for step in (sc.n // 2, 8 * TILE):
        bits, recs, _ = run(sc, rows, step, flags=FLAG_SPLIT_FEC)
        verify(sc, rows, bits, recs, f"split-fec step {step}")


# Which launches csrc/batch.hip really slices (launch_plain / launch_unit_demod: slice_of / choose_segments; there is no public indicator of it):
#  * a batch of ONE demodulator class with default flags is one launch (`units` empty) and takes SondeBatchConfig.time_slices as told,
#    if the count is <= the submit's tiles: "class2" (DFM + iMS-100 + MRZ-N1: the 4:1 class) and "m10" (M10 / M20: the 2:1 class);
#  * a batch with launch units slices every GFSK unit when time_slices is forced: "all-rows" (default flags; the AFSK rows keep the
#    batch from the one-launch mixed kernel, the units are the two classes and the two tone chains) and "late-join" / "pipeline" (one
#    unit per sonde type);
#  * the GFSK rows alone with default flags are NOT sliced: both classes without AFSK rows run as sd_demod_mixed_kernel, which takes no
#    slices and ignores time_slices.  That shape is test_tile_sized_submits' (and no case here).
SLICED = {
    "class2": ((S.DFM, S.IMS, S.MRZ), 0),
    "m10": ((S.M10,), 0),
    "all-rows": (ALL, 0),
    "late-join": (GFSK, FLAG_LATE_JOIN),
    "pipeline": (GFSK, FLAG_PIPELINE),
}


@pytest.mark.parametrize("slices", [2, 5])
@pytest.mark.parametrize("config", sorted(SLICED))
def test_forced_time_slices(state, config, slices):
    """segments of a submit as workgroups of their own: nout0 and the hand-over between segments, in submits of 144 and of 48 tiles
    (with 5 slices the last segment is shorter than the others)"""
    sc = scene(state)
    types, flags = SLICED[config]
    rows = _rows(sc, types)
    for step in (sc.n, sc.n // 3):
        assert slices <= step // TILE
        bits, recs, _ = run(sc, rows, step, flags=flags, time_slices=slices)
        verify(sc, rows, bits, recs, f"time-slices {config} x{slices} step {step}")


@pytest.mark.parametrize("flags", [FLAG_PIPELINE, FLAG_LATE_JOIN], ids=["pipeline", "late-join"])
def test_frames_by_ticket(state, flags):
    """three submits queued back to back, the frames fetched per ticket (those of submit k once submit k + 1 is queued); the bits of
    all three are read afterwards (the batch is created for the whole length, so its ring holds them) and go through reference()"""
    sc = scene(state)
    rows = _rows(sc, ALL)
    step = sc.n // 3
    b = SondeBatch(len(rows), sc.n, types=sc.types[rows], flags=flags)
    st = torch.cuda.current_stream().cuda_stream
    b.ticket()
    parts = []
    for k in range(3):
        b.submit(sc.dev[:, k * step:(k + 1) * step].contiguous(), st)
        if k >= 1:
            parts.append(b.frames_of(k))
    parts.append(b.frames_of(3))
    recs = _by_row(np.concatenate(parts), len(rows))
    assert b.overflow() == 0
    bits = [b.read_bits(r, 0, b.nbits(r)) for r in range(len(rows))]
    b.close()
    verify(sc, rows, bits, recs, f"tickets flags={flags}")


def test_wide_auto_modem_class(state):
    """SONDE_FLAG_WIDE_AUTO: iMS-100, M10 / M20 and MRZ-N1 behind the other modem class, the same framers"""
    sc = scene(state)
    rows = _rows(sc, (S.IMS, S.M10, S.MRZ))
    bits, recs, _ = run(sc, rows, 24 * TILE, flags=FLAG_WIDE_AUTO)
    verify(sc, rows, bits, recs, "wide-auto")


BIN_HZ = 10_000_000 / 512
# (bin, type, Eb/N0 dB): per type from where most frames fail to where most are clean
WB_SONDES = [(5, S.DFM, 7.5), (40, S.DFM, 9.0), (350, S.DFM, 10.5), (444, S.DFM, 13.0),
             (77, S.IMS, 7.5), (130, S.IMS, 9.0), (420, S.IMS, 10.5), (490, S.IMS, 13.0),
             (200, S.MRZ, 7.5), (301, S.MRZ, 9.0), (470, S.MRZ, 10.5), (23, S.MRZ, 13.0)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_channelizer_bins(state, fused):
    """sd_fixed_sync_step<T, true> behind the channelizer: DFM / iMS-100 / MRZ-N1 bins of a noisy wideband scene"""
    from sdrpp_radiosonde_amd import synth
    types = np.zeros(512, dtype=np.uint8)
    for k, t, _ in WB_SONDES:
        types[k] = t
    chz = SondeChannelizer(types=types, blocks_per_submit=1, fused=fused)
    assert chz.fused == fused
    blk = chz.samples_per_submit
    nblk = 40                                                            # 5.1 s
    sondes = [((k if k < 256 else k - 512) * BIN_HZ, t) for k, t, _ in WB_SONDES]
    if "wb" not in state:
        state["wb"] = synth.make_wideband_scene(sondes, nblk * blk, ebn0_db=[e for _, _, e in WB_SONDES], seed=77, device="cuda:0")[0]
    iq = state["wb"]
    bits = {k: [] for k, _, _ in WB_SONDES}
    nb = {k: 0 for k, _, _ in WB_SONDES}
    parts = []
    for i in range(nblk):
        chz.submit(iq[i * blk:(i + 1) * blk].contiguous())
        parts.append(chz.frames())
        for k in bits:
            n = chz.batch.nbits(k)
            if n > nb[k]:
                bits[k].append(chz.batch.read_bits(k, nb[k], n - nb[k]))
                nb[k] = n
    assert chz.batch.overflow() == 0
    recs = _by_row(np.concatenate(parts), 512)
    seen = {t: [0, 0, 0] for t in (S.DFM, S.IMS, S.MRZ)}                 # records, with corrections / clean checks, with rejects
    for k, t, _ in WB_SONDES:
        ref = R.reference(t, np.concatenate(bits[k]), k)
        assert len(ref) == len(recs[k]) and ref.tobytes() == recs[k].tobytes(), (fused, k, t, len(ref), len(recs[k]))
        seen[t][0] += len(ref)
        if t == S.MRZ:
            seen[t][1] += int((ref["nerr"][:, 0] == 0).sum())
            seen[t][2] += int((ref["nerr"][:, 0] < 0).sum())
        else:
            seen[t][1] += int((ref["nerr"][:, 0] > 0).sum())
            seen[t][2] += int((ref["nerr"][:, 1] > 0).sum())
    chz.close()
    print(f"FRAMER-REF gpu channelizer fused={fused}: (records, corrected or clean, rejected) per type {seen}")
    for t, (n, good, bad) in seen.items():
        assert n > 0 and good > 0 and bad > 0, (t, n, good, bad)
