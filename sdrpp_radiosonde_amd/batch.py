"""Python face of the B0 batch API (include/sonde_abi.h): thin, no compute -- every call goes
through the C ABI of libsonde_mi355.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._handle import Handle, channel_rows, chk, current_stream
from ._lib import SondeError  # noqa: F401  (batch.SondeError: where hosts and tests import it from)
from ._lib import FRAME_COMBINED, FLAG_AFSK_RESCUE, FLAG_DFM_RESCUE, FLAG_IMS_RESCUE, FLAG_MANCHESTER_RESCUE, FLAG_RS41_RESCUE, FRAME_DTYPE, INPUT_IQ, INPUT_IQ8, INPUT_IQ16, INPUT_REAL, TILE  # noqa: F401


class SondeBatch(Handle):
    """Many independent 48 kS/s channels on one GPU; one HIP workgroup per channel.

    submit() takes a device tensor (torch, any object with data_ptr()) shaped
    [C, n, 2] float32 (IQ) or [C, n] float32 (discriminator samples), n % 2048 == 0.
    """
    DESTROY = "sonde_batch_destroy"

    def __init__(self, n_channels: int, max_samples: int, *, types=None, input_kind: int = INPUT_IQ, device: int = 0, flags: int = 0, time_slices: int = 0):
        self.n_channels = int(n_channels)
        self.max_samples = int(max_samples)
        self.input_kind = input_kind
        self.device = int(device)
        cfg = _lib.SondeBatchConfig()
        cfg.n_channels = self.n_channels
        self._types = None
        if types is not None:
            self._types = np.ascontiguousarray(types, dtype=np.uint8)
            assert self._types.shape == (self.n_channels,)
            cfg.types = self._types.ctypes.data_as(C.POINTER(C.c_uint8))
        cfg.max_samples = self.max_samples
        cfg.flags = flags
        self.flags = int(flags)
        cfg.time_slices = time_slices          # 0: the library's choice (SondeBatchConfig.time_slices)
        cfg.input_kind = input_kind
        cfg.device = device
        self._create("sonde_batch_create", C.byref(cfg))

    def _chk(self, rc):
        return chk(rc)

    def submit(self, samples, stream: int | None = None):
        n, stride = channel_rows(samples, self.input_kind, self.n_channels, self.device, "batch")
        # keep the device buffers of the last two submits alive (Python-side lifetime only): with SONDE_FLAG_LATE_JOIN / _PIPELINE the
        # buffer of submit t may be read until submit t + 1 is queued (include/sonde_abi.h); with default flags stream order covers it
        self._keep = (samples, getattr(self, "_keep", (None, None))[0])
        self._chk(self.L.sonde_batch_submit(self.h, C.c_void_p(samples.data_ptr()), n, stride, C.c_void_p(stream or 0)))

    def submit_host(self, samples: np.ndarray):
        want = {INPUT_IQ16: np.int16, INPUT_IQ8: np.int8}.get(self.input_kind, np.float32)
        if want is not np.float32 and np.asarray(samples).dtype != want:
            raise SondeError(f"samples must be {np.dtype(want).name} for this input kind, got {np.asarray(samples).dtype} (no silent conversion)")
        samples = np.ascontiguousarray(samples, dtype=want)
        n = samples.shape[1]
        self._chk(self.L.sonde_batch_submit_host(self.h, samples.ctypes.data_as(C.c_void_p), n, n))

    def wait_input(self, stream: int | None = None):
        """Device-side: work queued on `stream` after this call may overwrite the last submit's sample buffer (sonde_batch_wait_input)."""
        self._chk(self.L.sonde_batch_wait_input(self.h, C.c_void_p(stream or 0)))

    def restart_channels(self, channels):
        """From the next submit on the listed channels decode as streams that begin there (sonde_batch_restart_channels): one launch
        behind the last submit, no host synchronisation; earlier frames stay readable."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        self._chk(self.L.sonde_batch_restart_channels(self.h, ch.ctypes.data_as(C.c_void_p), len(ch)))

    def test_shift_age(self, channels, samples, ring_turns) -> np.ndarray:
        """Test introspection, not for hosts (sonde_batch_test_shift_age): the listed channels become the same streams, begun
        samples[i] input samples (a multiple of 30720) and ring_turns[i] whole turns of the bit ring earlier.  Ordered like
        restart_channels.  Returns the bits added per channel."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        sm = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, dtype=np.uint64), ch.shape))
        tr = np.ascontiguousarray(np.broadcast_to(np.asarray(ring_turns, dtype=np.uint32), ch.shape))
        added = np.zeros(len(ch), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        self._chk(self.L.sonde_batch_test_shift_age(self.h, p(ch), len(ch), p(sm), p(tr), p(added)))
        return added

    def sync(self) -> int:
        return self._chk(self.L.sonde_batch_sync(self.h))

    def frames(self) -> np.ndarray:
        n = self.sync()
        out = np.zeros(n, dtype=FRAME_DTYPE)
        if n:
            got = self._chk(self.L.sonde_batch_frames(self.h, out.ctypes.data_as(C.c_void_p), n))
            out = out[:got]
        return out

    def ticket(self) -> int:
        """Number of the last submit (1-based)."""
        return int(self.L.sonde_batch_ticket(self.h))

    def frames_of(self, ticket: int) -> np.ndarray:
        """Frames of submit `ticket` (one of the last two): waits for that submit only, not for later ones."""
        n = self._chk(self.L.sonde_batch_frames_of(self.h, ticket, None, 0))       # count first: the buffer is sized from it
        out = np.zeros(n, dtype=FRAME_DTYPE)
        if n:
            out = out[:self._chk(self.L.sonde_batch_frames_of(self.h, ticket, out.ctypes.data_as(C.c_void_p), n))]
        return out

    def overflow(self) -> int:
        return self._chk(self.L.sonde_batch_overflow(self.h))

    def poll(self, cap: int = 4096):
        """SondeData fragments of the last submit with their channels: list of (channel, SondeData)."""
        out = (_lib.SondeData * cap)()
        chan = (C.c_uint32 * cap)()
        res = []
        while True:
            n = self._chk(self.L.sonde_batch_poll(self.h, out, chan, cap))
            if n == 0:
                return res
            for i in range(n):
                d = _lib.SondeData()
                C.memmove(C.byref(d), C.byref(out[i]), C.sizeof(d))
                res.append((int(chan[i]), d))

    def kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        self._chk(self.L.sonde_batch_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def class_ms(self) -> dict:
        """Mixed batches: {class index: average ms of that demodulator class's kernel alone} over the timed submits
        (sonde_batch_class_ms); {} for a batch of one class."""
        v = (C.c_float * 4)()
        self.L.sonde_batch_class_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        n = self._chk(self.L.sonde_batch_class_ms(self.h, v))
        return {k: float(v[k]) for k in range(4) if n > 0 and v[k] >= 0.0}

    def launch_info(self) -> dict:
        """{'units': launch units per submit, 'join': 0 at every submit (default) / 1 one submit late (FLAG_LATE_JOIN) / 2 never (FLAG_PIPELINE)} (sonde_batch_launch_info)"""
        u, j = C.c_uint32(), C.c_int32()
        self.L.sonde_batch_launch_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        self._chk(self.L.sonde_batch_launch_info(self.h, C.byref(u), C.byref(j)))
        return {"units": int(u.value), "join": int(j.value)}

    def set_timing(self, every_n: int):
        """Record kernel-timing events on every n-th submit only (0: never); the next submit is timed."""
        self._chk(self.L.sonde_batch_set_timing(self.h, int(every_n)))

    def rescue_info(self, channel: int) -> dict:
        """FLAG_RS41_RESCUE: what an RS41 channel has learned and done (sonde_batch_rescue_info): {'layouts': {320: [(offset, type,
        len), ...], 518: [...]}, 'tried': frames with a failed codeword it had a layout for, 'rescued': frames it filled in}."""
        lay = (_lib.SondeRs41Layout * 2)()
        tried, rescued = C.c_uint32(), C.c_uint32()
        self._chk(self.L.sonde_batch_rescue_info(self.h, channel, lay, C.byref(tried), C.byref(rescued)))
        layouts = {flen: [(int(l.offset[i]), int(l.type[i]), int(l.len[i])) for i in range(l.n_blocks)] for flen, l in ((320, lay[0]), (518, lay[1]))}
        return {"layouts": layouts, "tried": int(tried.value), "rescued": int(rescued.value)}

    def _counters(self, query, channel: int) -> dict:
        tried, rescued = C.c_uint32(), C.c_uint32()
        self._chk(query(self.h, channel, C.byref(tried), C.byref(rescued)))
        return {"tried": int(tried.value), "rescued": int(rescued.value)}

    def manchester_rescue_info(self, channel: int) -> dict:
        """FLAG_MANCHESTER_RESCUE: what the second pass has done on an M10 / M20 / MRZ-N1 channel (sonde_batch_manchester_rescue_info):
        {'tried': frames whose check failed that reached the solver, 'rescued': frames it corrected}."""
        return self._counters(self.L.sonde_batch_manchester_rescue_info, channel)

    def dfm_rescue_info(self, channel: int) -> dict:
        """FLAG_DFM_RESCUE: what the second pass has done on a DFM channel (sonde_batch_dfm_rescue_info): {'tried': frames with a
        failed Hamming word that reached the erasure decoder, 'rescued': frames it completed}."""
        return self._counters(self.L.sonde_batch_dfm_rescue_info, channel)

    def test_hamming84_erasures(self, words: np.ndarray, erased: np.ndarray):
        """FLAG_DFM_RESCUE's word decoder alone (sonde_batch_test_hamming84_erasures): words, erased [n] uint8 (erased: mask of the
        erased bits, 0x80 = the first).  Returns (decoded words, status [n]): status = bits changed, -1 = no decode."""
        w = np.ascontiguousarray(words, dtype=np.uint8).copy()
        er = np.ascontiguousarray(erased, dtype=np.uint8)
        assert w.ndim == 1 and er.shape == w.shape
        status = np.zeros(len(w), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_hamming84_erasures(self.h, w.ctypes.data_as(C.c_void_p), er.ctypes.data_as(C.c_void_p), len(w),
                                                             status.ctypes.data_as(C.c_void_p)))
        return w, status

    def ims_rescue_info(self, channel: int) -> dict:
        """FLAG_IMS_RESCUE: what the second pass has done on an iMS-100 channel (sonde_batch_ims_rescue_info): {'tried': frames with a
        rejected BCH block that reached the block decoder, 'rescued': frames it completed}."""
        return self._counters(self.L.sonde_batch_ims_rescue_info, channel)

    def test_ims_block(self, blocks: np.ndarray, viol: np.ndarray):
        """FLAG_IMS_RESCUE's block decoder alone (sonde_batch_test_ims_block): blocks, viol [n] uint64 (blocks: bit b of the block is bit
        45 - b; viol: bit k = boundary k of the block is violated, 0..46).  Returns (decoded blocks, status [n]): status = bits flipped,
        -1 = no decode."""
        blk = np.ascontiguousarray(blocks, dtype=np.uint64).copy()
        v = np.ascontiguousarray(viol, dtype=np.uint64)
        assert blk.ndim == 1 and v.shape == blk.shape
        status = np.zeros(len(blk), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_ims_block(self.h, len(blk), blk.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                                    status.ctypes.data_as(C.c_void_p)))
        return blk, status

    def afsk_rescue_info(self, channel: int) -> dict:
        """FLAG_AFSK_RESCUE: what the second pass has done on an iMet / C50 channel (sonde_batch_afsk_rescue_info): {'tried': packets whose
        check failed that reached the pattern search, 'rescued': packets it repaired}."""
        return self._counters(self.L.sonde_batch_afsk_rescue_info, channel)

    def test_afsk_repair(self, records: np.ndarray):
        """FLAG_AFSK_RESCUE's per-record routine alone (sonde_batch_test_afsk_repair): records [n] FRAME_DTYPE, caller-made.  Returns
        (records after the routine, status [n]): status = 0 untouched, 1 rescued, 2 several patterns fit."""
        rec = np.ascontiguousarray(records, dtype=FRAME_DTYPE).copy()
        assert rec.ndim == 1
        status = np.zeros(len(rec), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_afsk_repair(self.h, rec.ctypes.data_as(C.c_void_p), len(rec), status.ctypes.data_as(C.c_void_p)))
        return rec, status

    def set_diversity(self, groups, offsets=None, window_bits: int = 0, *, learn: bool = False, mark_duplicates: bool = False):
        """The receivers of one sonde (sonde_batch_set_diversity): groups = [[channel, ...], ...], 2..4 channels of one type each -- RS41
        (DESIGN SPEC 3.3j), M10 / M20 or MRZ-N1 (SPEC 3.3l: failed copies are combined by their 16-bit check), DFM (SPEC 3.3m: word by
        word, the better copy per Hamming codeword; bit counts are chips there), iMS-100 on a batch created with FLAG_IMS_DIVERSITY (SPEC
        3.3n: BCH block by block, from the chips of the members' bit rings; bit counts are chips, window_bits 0: 576), iMet or C50 on a
        batch created with FLAG_AFSK_DIVERSITY (SPEC 3.3o: by their 16-bit check; bit counts are on-air symbols, window_bits 0: 160 for
        iMet, 40 for C50 and at most 44 with a C50 group; C50 groups take given offsets only: no learn, no mark_duplicates) --; offsets[ch] =
        the channel's bit count when the group's common clock reads 0 (None: zeros); window_bits: how far apart two copies of a frame may
        lie on that clock (0: 960).  Once, before the first submit.
        learn=True (sonde_batch_set_diversity_auto, SONDE_DIVERSITY_LEARN): the GPU finds the offsets itself from frames that are good
        in two members and keeps following them; offsets=None then means that nothing is known (every member starts unlocked), else
        they are where the members start.  mark_duplicates=True (SONDE_DIVERSITY_MARK_DUPLICATES): all but one good copy of a
        transmitted frame get FRAME_DUPLICATE, and poll() leaves their fragments out."""
        gid = np.full(self.n_channels, -1, dtype=np.int32)
        for g, members in enumerate(groups):
            for ch in members:
                if not 0 <= int(ch) < self.n_channels or gid[int(ch)] >= 0:
                    raise SondeError(f"set_diversity: channel {ch} is out of range or in two groups")
                gid[int(ch)] = g
            if len(members) == 0:
                raise SondeError("set_diversity: an empty group")
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            assert off.shape == (self.n_channels,)
        offp = off.ctypes.data_as(C.c_void_p) if off is not None else None
        mode = (_lib.DIVERSITY_LEARN if learn else 0) | (_lib.DIVERSITY_MARK_DUPLICATES if mark_duplicates else 0)
        if mode:
            self._chk(self.L.sonde_batch_set_diversity_auto(self.h, gid.ctypes.data_as(C.c_void_p), offp, int(window_bits), mode))
        else:
            self._chk(self.L.sonde_batch_set_diversity(self.h, gid.ctypes.data_as(C.c_void_p), offp, int(window_bits)))

    def diversity_offsets(self, g: int) -> dict:
        """set_diversity: where group g stands (sonde_batch_diversity_offsets): {'offsets': [bit offset of each of the four member slots on
        the group's clock], 'locked': a bit per member that has an offset, 'learned': offsets the align step set or changed,
        'duplicates': records it marked FRAME_DUPLICATE}."""
        off = np.zeros(4, dtype=np.int64)
        locked, learned, dups = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.sonde_batch_diversity_offsets(self.h, int(g), off.ctypes.data_as(C.c_void_p), C.byref(locked), C.byref(learned), C.byref(dups)))
        return {"offsets": [int(v) for v in off], "locked": int(locked.value), "learned": int(learned.value), "duplicates": int(dups.value)}

    def test_diversity_align(self, records: np.ndarray, counts: np.ndarray, n_members: np.ndarray, carried: np.ndarray, off: np.ndarray,
                             locked: np.ndarray, mode: np.ndarray, kind: int | None = None):
        """set_diversity's align step alone (sonde_batch_test_diversity_align): records [n, 4, R] FRAME_DTYPE, caller-made, counts [n, 4]
        of them in use; n_members [n] = 2..4; carried [n, 4] (len 0: none); off [n, 4] int64, locked [n], mode [n].  kind: the sonde
        type whose predicates the step uses (sonde_batch_test_diversity_align_kind; None: RS41, the older entry).  Returns (records
        with their flags as the step left them, off, locked, learned [n], duplicates [n])."""
        rec = np.ascontiguousarray(records, dtype=FRAME_DTYPE).copy()
        assert rec.ndim == 3 and rec.shape[1] == 4
        n, R = rec.shape[0], rec.shape[2]
        cnt = np.ascontiguousarray(counts, dtype=np.uint32)
        nm = np.ascontiguousarray(n_members, dtype=np.uint32)
        car = np.ascontiguousarray(carried, dtype=FRAME_DTYPE)
        o = np.ascontiguousarray(off, dtype=np.int64).copy()
        lk = np.ascontiguousarray(locked, dtype=np.uint32).copy()
        md = np.ascontiguousarray(mode, dtype=np.uint32)
        assert cnt.shape == (n, 4) and nm.shape == (n,) and car.shape == (n, 4) and o.shape == (n, 4) and lk.shape == (n,) and md.shape == (n,)
        learned, dups = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        if kind is None:
            self._chk(self.L.sonde_batch_test_diversity_align(self.h, n, R, p(nm), p(rec), p(cnt), p(car), p(o), p(lk), p(md), p(learned), p(dups)))
        else:
            self._chk(self.L.sonde_batch_test_diversity_align_kind(self.h, int(kind), n, R, p(nm), p(rec), p(cnt), p(car), p(o), p(lk), p(md),
                                                                   p(learned), p(dups)))
        return rec, o, lk, learned, dups

    def diversity_info(self, g: int) -> dict:
        """set_diversity: what the pass has done for group g (sonde_batch_diversity_info): {'tried': failed frames that found partners
        none of which was good, 'combined': frames put together from the copies}."""
        tried, combined = C.c_uint32(), C.c_uint32()
        self._chk(self.L.sonde_batch_diversity_info(self.h, int(g), C.byref(tried), C.byref(combined)))
        return {"tried": int(tried.value), "combined": int(combined.value)}

    def test_rs41_combine(self, copies: np.ndarray, n_copies: np.ndarray):
        """set_diversity's combining rule alone (sonde_batch_test_rs41_combine): copies [n, 4] FRAME_DTYPE, caller-made, copy 0 the record
        to rewrite; n_copies [n] = 2..4.  Returns (copy 0 after the rule [n], status [n]): status = the copies used, -1 too many
        erasures, -2 no decode, -3 rejected."""
        cp = np.ascontiguousarray(copies, dtype=FRAME_DTYPE)
        nc = np.ascontiguousarray(n_copies, dtype=np.uint32)
        assert cp.ndim == 2 and cp.shape[1] == 4 and nc.shape == (len(cp),)
        out = np.zeros(len(cp), dtype=FRAME_DTYPE)
        status = np.zeros(len(cp), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_rs41_combine(self.h, len(cp), cp.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                                                       out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return out, status

    def test_check_combine(self, copies: np.ndarray, n_copies: np.ndarray):
        """set_diversity's combining rule for M10 / M20 / MRZ-N1 alone (sonde_batch_test_check_combine): copies [n, 4] FRAME_DTYPE,
        caller-made, copy 0 the failed record to rewrite; n_copies [n] = 2..4.  Returns (copy 0 after the rule [n], status [n]): status =
        the copies used, -1 not attempted, -2 no subset fits, -3 several fit."""
        cp = np.ascontiguousarray(copies, dtype=FRAME_DTYPE)
        nc = np.ascontiguousarray(n_copies, dtype=np.uint32)
        assert cp.ndim == 2 and cp.shape[1] == 4 and nc.shape == (len(cp),)
        out = np.zeros(len(cp), dtype=FRAME_DTYPE)
        status = np.zeros(len(cp), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_check_combine(self.h, len(cp), cp.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                                                        out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return out, status

    def test_dfm_combine(self, copies: np.ndarray, n_copies: np.ndarray):
        """set_diversity's combining rule for DFM alone (sonde_batch_test_dfm_combine, SPEC 3.3m steps 3 to 6): copies [n, 4] FRAME_DTYPE,
        caller-made DFM records of 33 bytes, copy 0 the failed record to rewrite; n_copies [n] = 2..4.  Returns (copy 0 after the rule
        [n], status [n]): status = the copies used, -1 the pairing guard refuses, -2 a word has no solution, -3 a word has several."""
        cp = np.ascontiguousarray(copies, dtype=FRAME_DTYPE)
        nc = np.ascontiguousarray(n_copies, dtype=np.uint32)
        assert cp.ndim == 2 and cp.shape[1] == 4 and nc.shape == (len(cp),)
        out = np.zeros(len(cp), dtype=FRAME_DTYPE)
        status = np.zeros(len(cp), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_dfm_combine(self.h, len(cp), cp.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                                                      out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return out, status

    def test_ims_combine(self, records: np.ndarray, n_copies: np.ndarray, blocks: np.ndarray):
        """set_diversity's combining rule for iMS-100 alone (sonde_batch_test_ims_combine, SPEC 3.3n steps 4 to 7): records [n] FRAME_DTYPE,
        copy 0's record of each case (iMS-100, 51 bytes, nerr[1] > 0); n_copies [n] = 2..4; blocks [n, 4, 12] uint64, block L of copy j as
        received (bit b of the block is bit 45 - b).  Returns (the record after the rule [n], status [n]): status = the copies used, 0 the
        record's nerr[1] is not what copy 0's blocks say, -1 the pairing guard refuses, -2 a block has no solution, -3 a block has several."""
        rec = np.ascontiguousarray(records, dtype=FRAME_DTYPE)
        nc = np.ascontiguousarray(n_copies, dtype=np.uint32)
        bl = np.ascontiguousarray(blocks, dtype=np.uint64)
        assert rec.ndim == 1 and nc.shape == (len(rec),) and bl.shape == (len(rec), 4, 12)
        out = np.zeros(len(rec), dtype=FRAME_DTYPE)
        status = np.zeros(len(rec), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_ims_combine(self.h, len(rec), rec.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                                                      bl.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return out, status

    def test_afsk_combine(self, copies: np.ndarray, n_copies: np.ndarray):
        """set_diversity's combining rule for iMet and C50 alone (sonde_batch_test_afsk_combine, SPEC 3.3o steps 3 to 6): copies [n, 4]
        FRAME_DTYPE, caller-made, copy 0 the failed record to rewrite; n_copies [n] = 2..4.  Returns (copy 0 after the rule [n], status
        [n]): status = the copies used, -1 not attempted, -2 no subset fits, -3 several fit."""
        cp = np.ascontiguousarray(copies, dtype=FRAME_DTYPE)
        nc = np.ascontiguousarray(n_copies, dtype=np.uint32)
        assert cp.ndim == 2 and cp.shape[1] == 4 and nc.shape == (len(cp),)
        out = np.zeros(len(cp), dtype=FRAME_DTYPE)
        status = np.zeros(len(cp), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_afsk_combine(self.h, len(cp), cp.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                                                       out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        return out, status

    def test_rs255_erasures(self, cw_pairs: np.ndarray, erased: np.ndarray, n: int):
        """The errors-and-erasures RS(255,231) corrector alone (sonde_batch_test_rs255_erasures): cw_pairs, erased [P, 2, 256] uint8
        (erased != 0: the position is an erasure).  Returns (corrected pairs, status [P, 2]): status = bytes changed, -1 = undecodable."""
        cw = np.ascontiguousarray(cw_pairs, dtype=np.uint8).copy()
        er = np.ascontiguousarray(erased, dtype=np.uint8)
        assert cw.ndim == 3 and cw.shape[1:] == (2, 256) and er.shape == cw.shape
        status = np.zeros((len(cw), 2), dtype=np.int32)
        self._chk(self.L.sonde_batch_test_rs255_erasures(self.h, cw.ctypes.data_as(C.c_void_p), len(cw), int(n), er.ctypes.data_as(C.c_void_p),
                                                         status.ctypes.data_as(C.c_void_p)))
        return cw, status

    def nbits(self, channel: int) -> int:
        return int(self.L.sonde_batch_nbits(self.h, channel))

    def read_bits(self, channel: int, start: int, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=np.uint8)
        self._chk(self.L.sonde_batch_read_bits(self.h, channel, start, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def state(self, channel: int) -> dict:
        t, p = C.c_int64(), C.c_int32()
        b, a, y = C.c_float(), C.c_float(), C.c_float()
        self._chk(self.L.sonde_batch_read_state(self.h, channel, C.byref(t), C.byref(p), C.byref(b), C.byref(a), C.byref(y)))
        # afc_u: the newest AFC state (SPEC 3.0b); `yprev` is the key's name of rounds 1-3 (the same value), kept for the oracle binding's sake
        return dict(t_next=t.value, period=p.value, bias=b.value, amp=a.value, afc_u=y.value, yprev=y.value)


def row_stride(n_samples: int, iq: bool = True, kind: int | None = None) -> int:
    """Channel stride (in samples) the library recommends for rows of n_samples: the next power of two in bytes (HBM channel
    spread of rows streamed side by side; include/sonde_abi.h sonde_row_stride).  kind: an INPUT_* value (overrides iq)."""
    if kind is None:
        kind = INPUT_IQ if iq else INPUT_REAL
    return int(_lib.load().sonde_row_stride(int(n_samples), kind))


def strided_rows(x, stride: int | None = None):
    """A copy of the device tensor x = [C, n, 2] (or [C, n]) whose rows lie `stride` samples apart (default: row_stride), as a
    view of the padded allocation: what submit() takes."""
    import torch
    n = x.shape[1]
    st = stride or row_stride(n, kind={torch.int16: INPUT_IQ16, torch.int8: INPUT_IQ8}.get(x.dtype, INPUT_IQ) if x.dim() == 3 else INPUT_REAL)
    if st == n:
        return x
    buf = torch.empty((x.shape[0], st) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
    buf[:, :n] = x
    return buf[:, :n]


class SondeChannelizer(Handle):
    """Wideband front-end (BASELINE config 4): n_streams x 10 MS/s complex IQ -> 512 bins each (20 kS/s, one phase sample per
    step) -> per-bin decode; every stage is one launch over all streams.  submit() takes [samples_per_submit, 2] (one stream) or
    [n_streams, samples_per_submit, 2].  Bins carry the 12 kS/s sondes (RS41, DFM, iMS-100, MRZ-N1) and, unfused, the AFSK
    sondes; an M10 channel (50 kHz wide) does not fit a 19.5 kHz bin: use SondeVfo for those."""
    DESTROY = "sonde_chan_destroy"

    def __init__(self, types=None, blocks_per_submit: int = 1, device: int = 0, n_streams: int = 1, fused: bool | None = None, overlap: bool | None = None,
                 dual: bool = False, input_kind: int = INPUT_IQ):
        """dual: both stackings of every stream (SPEC 3.5c): 1024 channels per stream, 1024 p + k = even bin k (centre k x 19531.25 Hz),
        1024 p + 512 + k = odd bin k (centre (k + 1/2) x 19531.25 Hz): every carrier lies within 4.9 kHz of a bin centre."""
        self._types = None
        self.n_streams = int(n_streams)
        self.dual = bool(dual)
        self.n_channels = (1024 if dual else 512) * self.n_streams
        tp = None
        if types is not None:
            self._types = np.ascontiguousarray(types, dtype=np.uint8)
            assert self._types.shape == (self.n_channels,)
            tp = self._types.ctypes.data_as(C.c_void_p)
        self._create("sonde_chan_create_dual" if dual else "sonde_chan_create_multi", tp, blocks_per_submit, self.n_streams, device)
        # fused (default where possible): discriminator + resampler inside the decoder kernel; fused=False keeps the 48 kS/s rows
        # (read()); fused=None leaves the library's choice alone
        self.fused = bool(self.L.sonde_chan_set_fused(self.h, 1 if fused else 0)) if fused is not None else bool(self.L.sonde_chan_set_fused(self.h, -1))
        # overlap (an option, off by default): filter bank of submit k+1 beside the decoder of submit k, on internal streams
        self.overlap = bool(self.L.sonde_chan_set_overlap(self.h, 1)) if overlap else False
        # input_kind: INPUT_IQ (complex64 blocks), INPUT_IQ16 (int16 I, Q pairs) or INPUT_IQ8 (int8 pairs): the receiver's own format
        self.input_kind = int(self.L.sonde_chan_set_input(self.h, input_kind))
        if self.input_kind != input_kind:
            raise SondeError("sonde_chan_set_input: input kind not accepted")
        self.samples_per_submit = int(self.L.sonde_chan_samples_per_submit(self.h))
        self.n_steps = self.samples_per_submit // 500
        self.batch = SondeBatch.__new__(SondeBatch)          # borrowed view of the embedded 512-channel batch
        self.batch.L = self.L
        self.batch.h = C.c_void_p(self.L.sonde_chan_batch(self.h))
        self.batch.n_channels = self.n_channels
        self.batch.close = lambda: None

    def submit(self, iq, stream: int | None = None):
        assert tuple(iq.shape) in ((self.samples_per_submit, 2), (self.n_streams, self.samples_per_submit, 2)) and iq.is_contiguous()
        assert self.n_streams == 1 or iq.dim() == 3
        want = {INPUT_IQ16: "int16", INPUT_IQ8: "int8"}.get(self.input_kind, "float32")
        if not str(iq.dtype).endswith(want) or str(iq.dtype).endswith("u" + want):
            raise SondeError(f"wideband block must be {want}, got {iq.dtype}")
        self._keep = iq
        chk(self.L.sonde_chan_submit(self.h, C.c_void_p(iq.data_ptr()), self.samples_per_submit, C.c_void_p(stream or 0)))

    def frames(self) -> np.ndarray:
        return SondeBatch.frames(self.batch)

    def kernel_ms(self):
        """(filter bank, discriminator + resampler, demodulator, framers) average ms over the timed submits."""
        v = [C.c_float() for _ in range(4)]
        chk(self.L.sonde_chan_kernel_ms(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def read(self):
        """(phases [bins, n_steps] in quadrants, 48 kS/s rows [bins, n_steps * 12 / 5] or None in fused mode) of the last submit."""
        bins = np.zeros((self.n_channels, self.n_steps), dtype=np.float32)
        out48 = None if self.fused else np.zeros((self.n_channels, self.n_steps * 12 // 5), dtype=np.float32)
        chk(self.L.sonde_chan_read(self.h, bins.ctypes.data_as(C.c_void_p), out48.ctypes.data_as(C.c_void_p) if out48 is not None else None))
        return bins, out48

    def close(self):
        if self.h:
            self.batch.h = None          # the borrowed view first: the embedded batch goes with the channelizer
        super().close()


def get_taps(sonde_type: int) -> np.ndarray:
    out = np.zeros((32, 32), dtype=np.float32)
    chk(_lib.load().sonde_get_taps(sonde_type, out.ctypes.data_as(C.c_void_p)))
    return out


# the reference's VFO bandwidth = sample rate per sonde type (/root/reference/src/main.hpp:44-52)
VFO_RATE = {0: 10000, 1: 15000, 2: 20000, 3: 50000, 4: 20000, 5: 20000, 6: 20000}


class SondeVfo(Handle):
    """VFO front-end (SURVEY 8 a1 + a2): IQ at the sonde type's VFO rate -> discriminator -> rational resampler -> 48 kS/s
    FM audio rows for a SondeBatch created with INPUT_REAL (/root/reference/src/main.cpp:55-60)."""
    DESTROY = "sonde_vfo_destroy"

    def __init__(self, n_channels: int, rate_in: int, max_in: int, device: int = 0):
        self._create("sonde_vfo_create", n_channels, rate_in, max_in, device)
        self.n_channels, self.rate_in, self.max_in = n_channels, rate_in, max_in
        up, down = C.c_int(), C.c_int()
        self.L.sonde_vfo_ratio(rate_in, C.byref(up), C.byref(down))
        self.up, self.down = up.value, down.value

    def out_samples(self, n_in: int) -> int:
        return int(self.L.sonde_vfo_out_samples(self.h, n_in))

    def process(self, iq, out=None, stream: int | None = None):
        """iq: CUDA float32 tensor [C, n_in, 2] (rows may be strided); returns the [C, n_out] float32 rows."""
        import torch
        assert iq.is_cuda and iq.dtype == torch.float32 and iq.shape[0] == self.n_channels and iq.shape[2] == 2 and iq.stride(1) == 2
        n_in = iq.shape[1]
        n_out = self.out_samples(n_in)
        if out is None:
            out = torch.empty((self.n_channels, n_out), dtype=torch.float32, device=iq.device)
        if stream is None:
            stream = current_stream(iq.device)
        chk(self.L.sonde_vfo_process(self.h, C.c_void_p(iq.data_ptr()), n_in, iq.stride(0) // 2, C.c_void_p(out.data_ptr()), out.stride(0),
                                     C.c_void_p(stream)))
        return out

    def taps(self) -> np.ndarray:
        g = np.zeros((self.up, 16), dtype=np.float32)
        chk(self.L.sonde_vfo_taps(self.rate_in, g.ctypes.data_as(C.c_void_p)))
        return g

