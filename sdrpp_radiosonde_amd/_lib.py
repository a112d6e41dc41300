"""ctypes binding of libsonde_mi355.so (include/sonde_abi.h).

The HIP library is the product: if it is missing or cannot be loaded this module raises --
there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# SONDE_MI355_LIB: developer override used for A/B timing of kernel variants (still a HIP build of this tree)
LIB_PATH = os.environ.get("SONDE_MI355_LIB") or os.path.join(PKG_DIR, "libsonde_mi355.so")

TILE = 2048
FRAME_MAX = 528
(RS41, DFM09, IMS100, M10, IMET4, C50, MRZN1) = range(7)
INPUT_IQ, INPUT_REAL, INPUT_IQ16, INPUT_IQ8 = 0, 1, 2, 3
PROCEED, PARSED = 0, 1
DATA_SEQ, DATA_POS, DATA_SPEED, DATA_TIME, DATA_PTU, DATA_SERIAL, DATA_SHUTDOWN, DATA_OZONE = (1 << i for i in range(8))


class SondeError(RuntimeError):
    """what every refusal of this package raises: the library's sonde_last_error() text, or the Python face's own (batch.SondeError)"""


class SondeFrame(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("type", C.c_uint32), ("len", C.c_int32), ("nerr", C.c_int32 * 2),
                ("flags", C.c_uint32), ("bitpos", C.c_uint64), ("data", C.c_uint8 * FRAME_MAX)]


FRAME_DTYPE = np.dtype([("channel", "<u4"), ("type", "<u4"), ("len", "<i4"), ("nerr", "<i4", (2,)),
                        ("flags", "<u4"), ("bitpos", "<u8"), ("data", "u1", (FRAME_MAX,))])
assert FRAME_DTYPE.itemsize == C.sizeof(SondeFrame)


class SondeData(C.Structure):
    _fields_ = [("fields", C.c_int), ("seq", C.c_int), ("lat", C.c_float), ("lon", C.c_float), ("alt", C.c_float),
                ("speed", C.c_float), ("heading", C.c_float), ("climb", C.c_float), ("time", C.c_int64),
                ("calib_percent", C.c_float), ("temp", C.c_float), ("rh", C.c_float), ("pressure", C.c_float),
                ("serial", C.c_char * 32), ("shutdown", C.c_int), ("o3_mpa", C.c_float)]


class SondeDetection(C.Structure):
    _fields_ = [("type", C.c_int32), ("inverted", C.c_uint32), ("best", C.c_double * 7), ("pos", C.c_uint64 * 7)]


DETECTION_DTYPE = np.dtype([("type", "<i4"), ("inverted", "<u4"), ("best", "<f8", (7,)), ("pos", "<u8", (7,))])
assert DETECTION_DTYPE.itemsize == C.sizeof(SondeDetection)


class SondeRs41Layout(C.Structure):
    _fields_ = [("n_blocks", C.c_uint32), ("offset", C.c_uint16 * 16), ("type", C.c_uint8 * 16), ("len", C.c_uint8 * 16)]


class SondeTunerVfo(C.Structure):
    _fields_ = [("offset_hz", C.c_int32), ("bandwidth_hz", C.c_uint32)]


class SondeScanParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("smooth_hz", C.c_uint32), ("min_sep_hz", C.c_uint32), ("centroid_hz", C.c_uint32),
                ("threshold", C.c_float)]


class SondeScanCandidate(C.Structure):
    _fields_ = [("offset_hz", C.c_int32), ("bandwidth_hz", C.c_uint32), ("cn0_dbhz", C.c_float), ("excess_db", C.c_float),
                ("bin", C.c_uint32)]


class SondeTrackLook(C.Structure):
    _fields_ = [("row", C.c_uint32), ("reserved", C.c_uint32), ("look", C.c_uint64), ("a_re", C.c_double), ("a_im", C.c_double),
                ("p", C.c_double)]


class SondeTrackParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("deadband_hz", C.c_uint32), ("max_step_hz", C.c_uint32)]


LOOK_DTYPE = np.dtype([("row", "<u4"), ("reserved", "<u4"), ("look", "<u8"), ("a_re", "<f8"), ("a_im", "<f8"), ("p", "<f8")])
assert LOOK_DTYPE.itemsize == C.sizeof(SondeTrackLook)
TRACK_DEADBAND_HZ, TRACK_MAX_STEP_HZ = 400, 4000          # SONDE_TRACK_DEADBAND_HZ, SONDE_TRACK_MAX_STEP_HZ


class SondeCombineBlock(C.Structure):
    _fields_ = [("sonde", C.c_uint32), ("reserved", C.c_uint32), ("block", C.c_uint64), ("m", C.c_double * 16), ("w", C.c_double * 8),
                ("wf", C.c_float * 8)]


COMBINE_DTYPE = np.dtype([("sonde", "<u4"), ("reserved", "<u4"), ("block", "<u8"), ("m", "<f8", (16,)), ("w", "<f8", (8,)), ("wf", "<f4", (8,))])
assert COMBINE_DTYPE.itemsize == C.sizeof(SondeCombineBlock)
COMBINE_MAX_ANTENNAS, COMBINE_BLOCK = 4, 1024          # SONDE_COMBINE_MAX_ANTENNAS, SONDE_COMBINE_BLOCK


CANDIDATE_DTYPE = np.dtype([("offset_hz", "<i4"), ("bandwidth_hz", "<u4"), ("cn0_dbhz", "<f4"), ("excess_db", "<f4"), ("bin", "<u4")])
assert CANDIDATE_DTYPE.itemsize == C.sizeof(SondeScanCandidate)


class SondeBatchConfig(C.Structure):
    _fields_ = [("n_channels", C.c_uint32), ("types", C.POINTER(C.c_uint8)), ("max_samples", C.c_uint32),
                ("input_kind", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32), ("launch_units", C.c_uint32),
                ("struct_size", C.c_uint32), ("time_slices", C.c_uint32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(SondeBatchConfig)      # SONDE_BATCH_CONFIG_INIT: sonde_batch_create refuses any other value


FLAG_WIDE = 1            # one decimation step less for every GFSK sonde (SONDE_FLAG_WIDE)
FLAG_RS41_WIDE = FLAG_WIDE
FLAG_SPLIT_FEC = 2
FLAG_PIPELINE = 4        # launch units never joined into the caller's stream (SONDE_FLAG_PIPELINE; opt-in)
FLAG_JOIN = 16           # accepted and ignored: joining at every submit is the default since round 6 (SONDE_FLAG_JOIN)
FLAG_LATE_JOIN = 32      # launch units joined into the caller's stream ONE SUBMIT LATE (SONDE_FLAG_LATE_JOIN; opt-in: round 5's default)
FLAG_WIDE_AUTO = 8       # SONDE_FLAG_WIDE for the types whose reference channel is >= 20 kHz only (iMS-100, MRZ-N1, M10)
FLAG_RS41_RESCUE = 64    # RS41: second pass over frames whose RS stage failed, block CRCs as erasure hints (SONDE_FLAG_RS41_RESCUE; opt-in)
FLAG_IMS_DIVERSITY = 2048  # iMS-100 channels may be members of set_diversity groups (SONDE_FLAG_IMS_DIVERSITY, DESIGN SPEC 3.3n; opt-in)
FLAG_AFSK_DIVERSITY = 4096  # iMet and C50 channels may be members of set_diversity groups (SONDE_FLAG_AFSK_DIVERSITY, DESIGN SPEC 3.3o; opt-in)
FRAME_RESCUED = 2        # SondeFrame.flags bit of a frame a second pass completed (SONDE_FRAME_RESCUED)
FRAME_COMBINED = 4       # SondeFrame.flags bit of an RS41, M10 / M20, MRZ-N1, DFM or iMS-100 frame set_diversity put together from several receivers' copies (SONDE_FRAME_COMBINED)
FRAME_DUPLICATE = 8      # SondeFrame.flags bit of a good frame another receiver of its diversity group has delivered (SONDE_FRAME_DUPLICATE)
DIVERSITY_LEARN = 1              # set_diversity modes (SONDE_DIVERSITY_LEARN, SONDE_DIVERSITY_MARK_DUPLICATES)
DIVERSITY_MARK_DUPLICATES = 2
FLAG_MANCHESTER_RESCUE = 128   # M10 / M20 / MRZ-N1: second pass over frames whose check failed, Manchester violations as hints (SONDE_FLAG_MANCHESTER_RESCUE; opt-in)
FLAG_DFM_RESCUE = 256         # DFM: second pass over frames with a Hamming word given up on, Manchester violations as erasures (SONDE_FLAG_DFM_RESCUE; opt-in)
FLAG_IMS_RESCUE = 512         # iMS-100: second pass over frames with a BCH block rejected, biphase-S boundary violations as hints (SONDE_FLAG_IMS_RESCUE; opt-in)
FLAG_AFSK_RESCUE = 1024       # iMet / C50: second pass over packets whose check failed, one bit or an adjacent pair repaired (SONDE_FLAG_AFSK_RESCUE; opt-in)


def rescue_flags(rescue=False, manchester_rescue=False, dfm_rescue=False, ims_rescue=False, afsk_rescue=False) -> int:
    """The batch flags of a receiver's rescue keywords: rescue=True: FLAG_RS41_RESCUE, the second pass over RS41 frames whose RS stage
    failed (SPEC 3.3c; a channel's restart clears its layout); manchester_rescue: FLAG_MANCHESTER_RESCUE, the one over M10 / M20 / MRZ-N1
    frames whose check failed (3.3f); dfm_rescue: FLAG_DFM_RESCUE, DFM frames with a Hamming word given up on (3.3g); ims_rescue:
    FLAG_IMS_RESCUE, iMS-100 frames with a BCH block rejected (3.3h); afsk_rescue: FLAG_AFSK_RESCUE, iMet / C50 packets whose check
    failed (3.3i)."""
    return ((FLAG_RS41_RESCUE if rescue else 0) | (FLAG_MANCHESTER_RESCUE if manchester_rescue else 0) | (FLAG_DFM_RESCUE if dfm_rescue else 0) |
            (FLAG_IMS_RESCUE if ims_rescue else 0) | (FLAG_AFSK_RESCUE if afsk_rescue else 0))


def frame_blocks(flags):
    """BCH blocks SONDE_FLAG_IMS_RESCUE decoded in a rescued iMS-100 frame (SONDE_FRAME_BLOCKS); an int or a numpy array of SondeFrame.flags"""
    return (flags >> 8) & 0xF


def frame_words(flags):
    """codewords SONDE_FLAG_DFM_RESCUE decoded in a rescued DFM frame (SONDE_FRAME_WORDS); an int or a numpy array of SondeFrame.flags"""
    return (flags >> 8) & 0xF


def frame_copies(flags):
    """copies a combined frame was made from (SONDE_FRAME_COPIES); an int or a numpy array of SondeFrame.flags"""
    return (flags >> 8) & 0xF


def frame_joint(flags):
    """words of a combined DFM frame that failed in every copy and were decoded jointly -- of a combined iMS-100 frame: the BCH blocks
    rejected in every copy and decoded from the copies' majority --, capped at 15 (SONDE_FRAME_JOINT); an int or a numpy array of
    SondeFrame.flags"""
    return (flags >> 12) & 0xF


def frame_unknowns(flags):
    """bits on which the copies of a combined M10 / M20 / MRZ-N1 frame differed, capped at 15 (SONDE_FRAME_UNKNOWNS); an int or a
    numpy array of SondeFrame.flags"""
    return (flags >> 12) & 0xF


def frame_flips(flags):
    """data bits SONDE_FLAG_MANCHESTER_RESCUE or SONDE_FLAG_AFSK_RESCUE flipped in a rescued frame (SONDE_FRAME_FLIPS); an int or a numpy
    array of SondeFrame.flags"""
    return (flags >> 8) & 0xF


# every symbol include/sonde_abi.h declares; tests check the .so exports all of them
ABI_SYMBOLS = [
    "sonde_batch_create", "sonde_batch_destroy", "sonde_batch_submit", "sonde_batch_submit_host",
    "sonde_row_stride", "sonde_sample_bytes", "sonde_batch_wait_input", "sonde_batch_sync", "sonde_batch_frames", "sonde_batch_frames_of", "sonde_batch_ticket", "sonde_batch_overflow", "sonde_batch_kernel_ms", "sonde_batch_set_timing", "sonde_batch_class_ms", "sonde_batch_read_bits",
    "sonde_batch_launch_info", "sonde_batch_nbits", "sonde_batch_read_state", "sonde_batch_test_rs255", "sonde_batch_poll", "sonde_get_taps", "sonde_get_afsk_table", "sonde_parse_frame",
    "sonde_parser_create", "sonde_parser_feed", "sonde_parser_destroy", "sonde_rs41_temp", "sonde_rs41_rh", "sonde_dfm_temp", "sonde_rs41_pressure", "sonde_ozone_mpa",
    "sonde_m10_temp", "sonde_m10_rh", "sonde_m20_temp", "sonde_ims100_temp",
    "sonde_last_error", "sonde_version", "sonde_hbm_read_probe", "sonde_dewpt", "sonde_altitude_to_pressure",
    "sonde_gpx_open", "sonde_gpx_close", "sonde_gpx_start_track", "sonde_gpx_stop_track", "sonde_gpx_add_point",
    "sonde_ptu_open", "sonde_ptu_close", "sonde_ptu_add_point",
    "sonde_chan_create", "sonde_chan_create_multi", "sonde_chan_create_dual", "sonde_chan_streams", "sonde_chan_channels", "sonde_chan_set_fused", "sonde_chan_set_input", "sonde_chan_set_overlap", "sonde_chan_destroy", "sonde_chan_samples_per_submit", "sonde_chan_submit", "sonde_chan_batch",
    "sonde_chan_read", "sonde_chan_tables", "sonde_chan_kernel_ms",
    "sonde_vfo_create", "sonde_vfo_destroy", "sonde_vfo_ratio", "sonde_vfo_out_samples", "sonde_vfo_process", "sonde_vfo_process_host", "sonde_vfo_taps",
    "sonde_detect_create", "sonde_detect_destroy", "sonde_detect_submit", "sonde_detect_results", "sonde_detect_reset", "sonde_detect_thresholds",
    "sonde_detect_read", "sonde_detect_templates",
    "sonde_tuner_ratio", "sonde_tuner_taps", "sonde_tuner_create", "sonde_tuner_destroy", "sonde_tuner_out_samples", "sonde_tuner_retune",
    "sonde_tuner_process", "sonde_tuner_retune_continuous",
    "sonde_track_defaults", "sonde_track_create", "sonde_track_destroy", "sonde_track_look_samples", "sonde_track_lag", "sonde_track_ring",
    "sonde_track_submit", "sonde_track_results", "sonde_track_restart", "sonde_track_err_hz", "sonde_track_level_db", "sonde_track_quality",
    "sonde_track_step",
    "sonde_scan_create", "sonde_scan_destroy", "sonde_scan_fft_size", "sonde_scan_submit", "sonde_scan_reset", "sonde_scan_segments",
    "sonde_scan_spectrum", "sonde_scan_candidates", "sonde_scan_search", "sonde_scan_window", "sonde_scan_auto_fft_size",
    "sonde_tuner_create_slots", "sonde_tuner_slot_set", "sonde_tuner_slot_clear", "sonde_tuner_slot_active",
    "sonde_batch_restart_channels", "sonde_detect_restart_channels", "sonde_live_match",
    "sonde_batch_test_rs255_erasures", "sonde_batch_rescue_info", "sonde_batch_manchester_rescue_info",
    "sonde_batch_dfm_rescue_info", "sonde_batch_test_hamming84_erasures",
    "sonde_batch_ims_rescue_info", "sonde_batch_test_ims_block",
    "sonde_batch_afsk_rescue_info", "sonde_batch_test_afsk_repair",
    "sonde_batch_set_diversity", "sonde_batch_diversity_info", "sonde_batch_test_rs41_combine", "sonde_batch_test_check_combine",
    "sonde_batch_test_dfm_combine", "sonde_batch_test_ims_combine", "sonde_batch_test_afsk_combine",
    "sonde_batch_set_diversity_auto", "sonde_batch_diversity_offsets", "sonde_batch_test_diversity_align",
    "sonde_batch_test_diversity_align_kind",
    "sonde_batch_test_shift_age", "sonde_detect_test_shift_age", "sonde_tuner_test_set_base",
    "sonde_combine_defaults", "sonde_combine_create", "sonde_combine_destroy", "sonde_combine_block", "sonde_combine_process",
    "sonde_combine_restart", "sonde_combine_readout", "sonde_combine_weights", "sonde_combine_share",
] + [f"{x}_{fn}" for x in ("rs41", "dfm09", "ims100", "m10", "imet4", "c50", "mrzn1")
     for fn in ("decoder_init", "decoder_deinit", "decode")]

_lib = None


def load() -> C.CDLL:
    """Load libsonde_mi355.so; raises if it was not built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        # a fresh checkout: build the HIP library in-tree (hipcc cross-compiles gfx950 without a GPU); there is no
        # CPU fallback -- if this fails, so does everything that needs the library
        import subprocess
        csrc = os.path.join(os.path.dirname(LIB_PATH), "csrc")
        try:
            subprocess.check_call(["make", "-s", "-C", csrc])
        except (OSError, subprocess.CalledProcessError) as e:
            raise RuntimeError(f"{LIB_PATH} is missing and `make -C {csrc}` failed ({e}); there is no CPU fallback") from e
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.sonde_hbm_read_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float)]
    L.sonde_hbm_read_probe.restype = C.c_int
    L.sonde_last_error.restype = C.c_char_p
    L.sonde_version.restype = C.c_char_p
    L.sonde_batch_create.argtypes = [C.POINTER(SondeBatchConfig), C.POINTER(vp)]
    L.sonde_batch_destroy.argtypes = [vp]
    L.sonde_batch_destroy.restype = None
    L.sonde_batch_submit.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    L.sonde_batch_submit_host.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.sonde_batch_sync.argtypes = [vp]
    L.sonde_batch_sync.restype = C.c_long
    if hasattr(L, "sonde_batch_wait_input"):              # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_wait_input.argtypes = [vp, vp]
    L.sonde_batch_frames.argtypes = [vp, vp, C.c_size_t]
    L.sonde_batch_frames.restype = C.c_long
    if hasattr(L, "sonde_batch_frames_of"):
        L.sonde_batch_frames_of.argtypes = [vp, C.c_uint64, vp, C.c_size_t]
        L.sonde_batch_frames_of.restype = C.c_long
        L.sonde_batch_ticket.argtypes = [vp]
        L.sonde_batch_ticket.restype = C.c_uint64
        L.sonde_batch_overflow.argtypes = [vp]
        L.sonde_batch_overflow.restype = C.c_long
    L.sonde_batch_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(L, "sonde_batch_set_timing"):          # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_set_timing.argtypes = [vp, C.c_int]
    L.sonde_batch_read_bits.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_size_t, vp]
    L.sonde_batch_nbits.argtypes = [vp, C.c_uint32]
    L.sonde_batch_nbits.restype = C.c_uint64
    L.sonde_batch_read_state.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(L, "sonde_batch_test_rs255"):
        L.sonde_batch_test_rs255.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    if hasattr(L, "sonde_batch_rescue_info"):             # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_rs255_erasures.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, vp]
        L.sonde_batch_rescue_info.argtypes = [vp, C.c_uint32, C.POINTER(SondeRs41Layout), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    # the four counter passes: the counters query, and the entry that runs a step of the pass alone (Manchester has none)
    for who, unit, unit_args in (("manchester", None, None), ("dfm", "hamming84_erasures", [vp, vp, vp, C.c_size_t, vp]),
                                 ("ims", "ims_block", [vp, C.c_size_t, vp, vp, vp]), ("afsk", "afsk_repair", [vp, vp, C.c_size_t, vp])):
        if hasattr(L, f"sonde_batch_{who}_rescue_info"):  # absent only in older A/B builds loaded through SONDE_MI355_LIB
            getattr(L, f"sonde_batch_{who}_rescue_info").argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
            if unit:
                getattr(L, f"sonde_batch_test_{unit}").argtypes = unit_args
    if hasattr(L, "sonde_batch_set_diversity"):           # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_set_diversity.argtypes = [vp, vp, vp, C.c_uint32]
        L.sonde_batch_diversity_info.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.sonde_batch_test_rs41_combine.argtypes = [vp, C.c_size_t, vp, vp, vp, vp]
    if hasattr(L, "sonde_batch_test_check_combine"):      # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_check_combine.argtypes = [vp, C.c_size_t, vp, vp, vp, vp]
    if hasattr(L, "sonde_batch_test_dfm_combine"):        # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_dfm_combine.argtypes = [vp, C.c_size_t, vp, vp, vp, vp]
    if hasattr(L, "sonde_batch_test_ims_combine"):        # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_ims_combine.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, vp]
    if hasattr(L, "sonde_batch_test_afsk_combine"):       # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_afsk_combine.argtypes = [vp, C.c_size_t, vp, vp, vp, vp]
    if hasattr(L, "sonde_batch_set_diversity_auto"):      # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_set_diversity_auto.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
        L.sonde_batch_diversity_offsets.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.sonde_batch_test_diversity_align.argtypes = [vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "sonde_batch_test_diversity_align_kind"):   # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_diversity_align_kind.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sonde_get_taps.argtypes = [C.c_int, vp]
    L.sonde_parse_frame.argtypes = [vp, C.POINTER(SondeData), C.c_int]
    L.sonde_batch_poll.argtypes = [vp, C.POINTER(SondeData), C.POINTER(C.c_uint32), C.c_size_t]
    L.sonde_batch_poll.restype = C.c_long
    L.sonde_parser_create.argtypes = [C.c_int]
    L.sonde_parser_create.restype = vp
    L.sonde_parser_feed.argtypes = [vp, vp, C.POINTER(SondeData), C.c_int]
    L.sonde_parser_feed.restype = C.c_int
    L.sonde_parser_destroy.argtypes = [vp]
    L.sonde_parser_destroy.restype = None
    L.sonde_rs41_pressure.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_float)]
    L.sonde_rs41_pressure.restype = C.c_float
    L.sonde_ozone_mpa.argtypes = [C.c_float, C.c_float]
    L.sonde_ozone_mpa.restype = C.c_float
    L.sonde_m10_temp.argtypes = [C.c_uint, C.c_uint]
    L.sonde_m10_temp.restype = C.c_float
    L.sonde_m10_rh.argtypes = [C.c_uint32, C.c_uint32, C.c_float]
    L.sonde_m10_rh.restype = C.c_float
    L.sonde_m20_temp.argtypes = [C.c_uint]
    L.sonde_m20_temp.restype = C.c_float
    L.sonde_ims100_temp.argtypes = [C.c_uint32, C.c_float, C.c_float, C.c_float]
    L.sonde_ims100_temp.restype = C.c_float
    L.sonde_rs41_temp.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.sonde_rs41_temp.restype = C.c_float
    L.sonde_rs41_rh.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float]
    L.sonde_rs41_rh.restype = C.c_float
    L.sonde_dfm_temp.argtypes = [C.c_float, C.c_float, C.c_float]
    L.sonde_dfm_temp.restype = C.c_float
    L.sonde_dewpt.restype = C.c_float
    L.sonde_dewpt.argtypes = [C.c_float, C.c_float]
    L.sonde_altitude_to_pressure.restype = C.c_float
    L.sonde_altitude_to_pressure.argtypes = [C.c_float]
    L.sonde_chan_create.argtypes = [vp, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.sonde_chan_create_multi.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.sonde_chan_set_fused.argtypes = [vp, C.c_int]
    L.sonde_chan_set_overlap.argtypes = [vp, C.c_int]
    L.sonde_row_stride.argtypes = [C.c_size_t, C.c_int]
    L.sonde_row_stride.restype = C.c_size_t
    L.sonde_sample_bytes.argtypes = [C.c_int]
    L.sonde_sample_bytes.restype = C.c_size_t
    L.sonde_chan_streams.argtypes = [vp]
    L.sonde_chan_streams.restype = C.c_uint32
    L.sonde_chan_destroy.argtypes = [vp]
    L.sonde_chan_destroy.restype = None
    L.sonde_chan_samples_per_submit.argtypes = [vp]
    L.sonde_chan_samples_per_submit.restype = C.c_uint32
    L.sonde_chan_submit.argtypes = [vp, vp, C.c_size_t, vp]
    L.sonde_chan_kernel_ms.argtypes = [vp] + [C.POINTER(C.c_float)] * 4
    L.sonde_chan_batch.argtypes = [vp]
    L.sonde_chan_batch.restype = vp
    L.sonde_chan_read.argtypes = [vp, vp, vp]
    L.sonde_chan_tables.argtypes = [vp, vp, vp]
    if hasattr(L, "sonde_vfo_create"):
        L.sonde_vfo_create.argtypes = [C.c_uint32, C.c_int, C.c_size_t, C.c_int, C.POINTER(vp)]
        L.sonde_vfo_destroy.argtypes = [vp]
        L.sonde_vfo_destroy.restype = None
        L.sonde_vfo_ratio.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.sonde_vfo_out_samples.argtypes = [vp, C.c_size_t]
        L.sonde_vfo_out_samples.restype = C.c_size_t
        L.sonde_vfo_process.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp]
        L.sonde_vfo_process_host.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.sonde_vfo_taps.argtypes = [C.c_int, vp]
    if hasattr(L, "sonde_detect_create"):
        L.sonde_detect_create.argtypes = [C.c_uint32, C.c_uint32, C.c_int, vp, C.c_int, C.POINTER(vp)]
        L.sonde_detect_destroy.argtypes = [vp]
        L.sonde_detect_destroy.restype = None
        L.sonde_detect_submit.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
        L.sonde_detect_results.argtypes = [vp, vp, C.c_size_t]
        L.sonde_detect_reset.argtypes = [vp]
        L.sonde_detect_thresholds.argtypes = [vp]
        L.sonde_detect_read.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.sonde_detect_templates.argtypes = [C.c_int, vp, C.c_int]
    if hasattr(L, "sonde_tuner_create"):
        L.sonde_tuner_ratio.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.sonde_tuner_taps.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t]
        L.sonde_tuner_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SondeTunerVfo), C.c_size_t, C.c_int, C.c_int, C.POINTER(vp)]
        L.sonde_tuner_destroy.argtypes = [vp]
        L.sonde_tuner_destroy.restype = None
        L.sonde_tuner_out_samples.argtypes = [vp, C.c_size_t]
        L.sonde_tuner_out_samples.restype = C.c_size_t
        L.sonde_tuner_retune.argtypes = [vp, C.c_uint32, C.c_int32]
        L.sonde_tuner_process.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp]
    if hasattr(L, "sonde_scan_create"):
        L.sonde_scan_create.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t, C.c_int, C.c_int, C.POINTER(vp)]
        L.sonde_scan_destroy.argtypes = [vp]
        L.sonde_scan_destroy.restype = None
        L.sonde_scan_fft_size.argtypes = [vp]
        L.sonde_scan_submit.argtypes = [vp, vp, C.c_size_t, vp]
        L.sonde_scan_reset.argtypes = [vp]
        L.sonde_scan_segments.argtypes = [vp]
        L.sonde_scan_segments.restype = C.c_longlong
        L.sonde_scan_spectrum.argtypes = [vp, vp, C.c_size_t]
        L.sonde_scan_candidates.argtypes = [vp, C.POINTER(SondeScanParams), vp, C.c_size_t]
        L.sonde_scan_search.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(SondeScanParams), vp, C.c_size_t]
        L.sonde_scan_window.argtypes = [C.c_uint32, vp, C.c_size_t]
        L.sonde_scan_auto_fft_size.argtypes = [C.c_uint32]
    if hasattr(L, "sonde_track_create"):
        u32 = C.c_uint32
        L.sonde_tuner_retune_continuous.argtypes = [vp, u32, C.c_int32]
        L.sonde_track_defaults.argtypes = [u32, C.POINTER(u32), C.POINTER(u32)]
        L.sonde_track_create.argtypes = [u32, u32, u32, u32, u32, C.c_int, C.c_int, C.POINTER(vp)]
        L.sonde_track_destroy.argtypes = [vp]
        L.sonde_track_destroy.restype = None
        L.sonde_track_look_samples.argtypes = [vp]
        L.sonde_track_lag.argtypes = [vp]
        L.sonde_track_ring.argtypes = [vp]
        L.sonde_track_submit.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
        L.sonde_track_results.argtypes = [vp, vp, C.c_size_t, vp]
        L.sonde_track_restart.argtypes = [vp, u32]
        L.sonde_track_err_hz.argtypes = [u32, u32, C.c_double, C.c_double]
        L.sonde_track_err_hz.restype = C.c_double
        L.sonde_track_level_db.argtypes = [C.c_double, u32]
        L.sonde_track_level_db.restype = C.c_double
        L.sonde_track_quality.argtypes = [C.c_double, C.c_double, C.c_double]
        L.sonde_track_quality.restype = C.c_double
        L.sonde_track_step.argtypes = [C.c_int32, u32, u32, u32, u32, C.POINTER(SondeTrackLook), C.POINTER(SondeTrackParams), C.POINTER(C.c_int32)]
    if hasattr(L, "sonde_live_match"):
        u32 = C.c_uint32
        L.sonde_tuner_create_slots.argtypes = [u32, u32, u32, vp, u32, C.c_size_t, C.c_int, C.c_int, C.POINTER(vp)]
        L.sonde_tuner_slot_set.argtypes = [vp, u32, C.c_int32, u32]
        L.sonde_tuner_slot_clear.argtypes = [vp, u32]
        L.sonde_tuner_slot_active.argtypes = [vp, u32]
        L.sonde_batch_restart_channels.argtypes = [vp, vp, C.c_size_t]
        L.sonde_detect_restart_channels.argtypes = [vp, vp, C.c_size_t]
        L.sonde_live_match.argtypes = [vp, u32, vp, u32, u32, vp, vp]
    if hasattr(L, "sonde_batch_test_shift_age"):          # absent only in older A/B builds loaded through SONDE_MI355_LIB
        L.sonde_batch_test_shift_age.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        L.sonde_detect_test_shift_age.argtypes = [vp, vp, C.c_size_t, vp]
        L.sonde_tuner_test_set_base.argtypes = [vp, C.c_int64]
    if hasattr(L, "sonde_combine_create"):                # absent only in older A/B builds loaded through SONDE_MI355_LIB
        u32 = C.c_uint32
        L.sonde_combine_defaults.argtypes = [u32, C.POINTER(u32)]
        L.sonde_combine_create.argtypes = [u32, u32, u32, u32, u32, C.c_int, C.c_int, C.POINTER(vp)]
        L.sonde_combine_destroy.argtypes = [vp]
        L.sonde_combine_destroy.restype = None
        L.sonde_combine_block.argtypes = [vp]
        L.sonde_combine_process.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp]
        L.sonde_combine_restart.argtypes = [vp, u32]
        L.sonde_combine_readout.argtypes = [vp, vp, C.c_size_t]
        L.sonde_combine_weights.argtypes = [u32, vp, vp, vp]
        L.sonde_combine_share.argtypes = [vp, u32]
        L.sonde_combine_share.restype = C.c_double
    f = C.c_float
    L.sonde_gpx_open.restype = vp
    L.sonde_gpx_open.argtypes = [C.c_char_p]
    L.sonde_gpx_close.argtypes = [vp]
    L.sonde_gpx_start_track.argtypes = [vp, C.c_char_p]
    L.sonde_gpx_stop_track.argtypes = [vp]
    L.sonde_gpx_add_point.argtypes = [vp, C.c_long, f, f, f, f, f]
    L.sonde_ptu_open.restype = vp
    L.sonde_ptu_open.argtypes = [C.c_char_p]
    L.sonde_ptu_close.argtypes = [vp]
    L.sonde_ptu_add_point.argtypes = [vp, C.c_long, f, f, f, f, f, f, f, f, f, f, C.c_char_p]
    for x in ("rs41", "dfm09", "ims100", "m10", "imet4", "c50", "mrzn1"):
        getattr(L, f"{x}_decoder_init").argtypes = [C.c_int]
        getattr(L, f"{x}_decoder_init").restype = vp
        getattr(L, f"{x}_decoder_deinit").argtypes = [vp]
        getattr(L, f"{x}_decoder_deinit").restype = None
        getattr(L, f"{x}_decode").argtypes = [vp, C.POINTER(SondeData), vp, C.c_size_t]
        getattr(L, f"{x}_decode").restype = C.c_int
    _lib = L
    return L


def last_error() -> str:
    return load().sonde_last_error().decode()
