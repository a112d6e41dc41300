"""Python face of the wideband tuner (include/sonde_abi.h, DESIGN SPEC 3.9): thin, no compute -- every call goes through the C ABI of
libsonde_mi355.so.

    SondeTuner          a bank of VFOs at any integer-Hz offset over one wideband stream -> complex rows at rate_out
    WidebandReceiver    wideband stream -> tuner -> decoders, for a list of (offset, sonde type): the chain of the reference
                        (VFO -> FM -> resampler -> decoder, /root/reference/src/main.cpp:55-68) or the tuner straight to 48 kHz IQ;
                        the block arithmetic, the batch and its rows and the tracking loop are _chain's, shared with the
                        diversity and the live receiver

Use the tuner when the frequencies are known (any sonde type, M10 / M20 included; the cost grows with the number of VFOs), the
channelizer (batch.SondeChannelizer) to decode every 19.53 kHz bin of the band at once (fixed cost, no M10 / M20)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _chain, _lib
from ._chain import AFSK_TILE, IQ48_MAX_BW, ratio  # noqa: F401
from ._chain import lcm as _lcm, multiple_for as _multiple_for  # noqa: F401  (the names they had here)
from ._handle import Handle, chk, current_stream, wideband_block
from ._lib import C50, IMET4, INPUT_IQ, INPUT_REAL, SondeError  # noqa: F401
from .batch import SondeVfo


def tuner_taps(rate_in: int, rate_out: int, bandwidth_hz: int = 0) -> np.ndarray:
    """the float32 taps g[p][t] of one bandwidth (SPEC 3.9): [up, T]"""
    L = _lib.load()
    n = chk(L.sonde_tuner_taps(int(rate_in), int(rate_out), int(bandwidth_hz), None, 0))
    g = np.zeros(n, np.float32)
    chk(L.sonde_tuner_taps(int(rate_in), int(rate_out), int(bandwidth_hz), g.ctypes.data_as(C.c_void_p), n))
    up, _ = ratio(rate_in, rate_out)
    return g.reshape(up, n // up)


class SondeTuner(Handle):
    """A bank of VFOs over one wideband complex stream.  vfos: [(offset_hz, bandwidth_hz), ...] or [offset_hz, ...]
    (bandwidth 0 = rate_out).  process() takes a device block [n_in, 2] (float32; int16 for INPUT_IQ16, int8 for INPUT_IQ8),
    n_in a multiple of `down`, and returns [V, n_out, 2] float32 rows or writes them into `out` (a [V, >= n_out, 2] float32 view
    whose rows may lie any stride apart).

    SondeTuner.slots(...) makes a tuner of idle slots instead (SPEC 3.12): slot_set() / slot_clear() tune and idle them between
    two process() calls; an idle slot costs no mixing and its row is zeros.  `offsets[k]` / `bandwidths[k]` are None while idle."""
    DESTROY = "sonde_tuner_destroy"

    def __init__(self, rate_in: int, rate_out: int, vfos, max_in: int, *, input_kind: int = INPUT_IQ, device: int = 0):
        spec = [(v, 0) if np.isscalar(v) else (v[0], v[1]) for v in vfos]
        self.n_vfos = len(spec)
        arr = (_lib.SondeTunerVfo * max(1, self.n_vfos))()
        for i, (f, b) in enumerate(spec):
            arr[i].offset_hz, arr[i].bandwidth_hz = int(f), int(b)
        self._create("sonde_tuner_create", int(rate_in), int(rate_out), self.n_vfos, arr, int(max_in), int(input_kind), int(device))
        self.rate_in, self.rate_out, self.max_in = int(rate_in), int(rate_out), int(max_in)
        self.input_kind, self.device = int(input_kind), int(device)
        self.offsets = [int(f) for f, _ in spec]
        self.bandwidths = [int(b) or int(rate_out) for _, b in spec]
        self.up, self.down = ratio(rate_in, rate_out)

    @classmethod
    def slots(cls, rate_in: int, rate_out: int, n_slots: int, bandwidths, max_in: int, *, input_kind: int = INPUT_IQ, device: int = 0):
        """n_slots idle slots with one tap set per listed bandwidth (sonde_tuner_create_slots)"""
        self = cls.__new__(cls)
        self.n_vfos = int(n_slots)
        bws = np.ascontiguousarray([int(b) for b in bandwidths], dtype=np.uint32)
        self._create("sonde_tuner_create_slots", int(rate_in), int(rate_out), self.n_vfos, bws.ctypes.data_as(C.c_void_p), len(bws), int(max_in),
                     int(input_kind), int(device))
        self.rate_in, self.rate_out, self.max_in = int(rate_in), int(rate_out), int(max_in)
        self.input_kind, self.device = int(input_kind), int(device)
        self.offsets = [None] * self.n_vfos
        self.bandwidths = [None] * self.n_vfos
        self.up, self.down = ratio(rate_in, rate_out)
        return self

    def slot_set(self, k: int, hz: int, bandwidth_hz: int = 0):
        """slot k to offset hz at a listed bandwidth from the next process() on, as if tuned there since create (theta = 0)"""
        chk(self.L.sonde_tuner_slot_set(self.h, int(k), int(hz), int(bandwidth_hz)))
        self.offsets[k], self.bandwidths[k] = int(hz), int(bandwidth_hz) or self.rate_out

    def slot_clear(self, k: int):
        """slot k idle from the next process() on: its row is zeros"""
        chk(self.L.sonde_tuner_slot_clear(self.h, int(k)))
        self.offsets[k] = self.bandwidths[k] = None

    def slot_active(self, k: int) -> bool:
        return bool(chk(self.L.sonde_tuner_slot_active(self.h, int(k))))

    def out_samples(self, n_in: int) -> int:
        return int(self.L.sonde_tuner_out_samples(self.h, int(n_in)))

    def retune(self, k: int, hz: int, continuous: bool = False):
        """VFO k to offset hz from the next process() on.  continuous=False restarts the mixer's phase "as if tuned there since
        create" (a phase jump in the row at the boundary); continuous=True keeps the mixer's phase at the boundary (SPEC 3.9)"""
        chk((self.L.sonde_tuner_retune_continuous if continuous else self.L.sonde_tuner_retune)(self.h, int(k), int(hz)))
        self.offsets[k] = int(hz)

    def test_set_base(self, n_base: int):
        """Test introspection, not for hosts (sonde_tuner_test_set_base): the absolute input index of the first sample, for a tuner
        that has not processed or been retuned yet; a multiple of `down`, 0 .. 2^62."""
        chk(self.L.sonde_tuner_test_set_base(self.h, int(n_base)))

    def process(self, block, out=None, stream: int | None = None):
        import torch
        n_in = wideband_block(block, self.input_kind, self.device, "tuner")
        n_out = self.out_samples(n_in)
        if out is None:
            out = torch.empty((self.n_vfos, n_out, 2), dtype=torch.float32, device=block.device)
        elif (out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != self.n_vfos or out.shape[1] < n_out or out.shape[2] != 2
              or out.stride(1) != 2 or out.stride(2) != 1 or out.device != block.device):
            raise SondeError("out must be a float32 device view [n_vfos, >= n_out, 2], contiguous inside a row")
        if stream is None:
            stream = current_stream(block.device)
        self._keep = block
        chk(self.L.sonde_tuner_process(self.h, C.c_void_p(block.data_ptr()), n_in, C.c_void_p(out.data_ptr()), out.stride(0) // 2,
                                       C.c_void_p(stream)))
        return out[:, :n_out]


class WidebandReceiver:
    """Decode sondes at known offsets from one wideband stream.  sondes: [(offset_hz, sonde type), ...]; the `channel` of a frame
    (and of a poll() fragment) is the index into `sondes`.

      chain="iq48"       one tuner at 48 kHz, VFO k at B = VFO_RATE[type] (M10 / M20: 40 kHz), into one SondeBatch(INPUT_IQ)
      chain="reference"  the reference's chain: one tuner per distinct VFO_RATE at R = B, SondeVfo(B), the 48 kHz FM rows of every
                         sonde in one SondeBatch(INPUT_REAL) buffer

    submit() takes a device block [n, 2] (float32 / int16 / int8 by input_kind), n a multiple of `granule` and <= max_in
    (default: one granule): the smallest block that leaves whole decoder tiles at 48 kHz.

    track=True follows drifting carriers (SPEC 3.11): a SondeTracker meters the tuner's rows of every submit; at the start of the
    next submit the newest look of each VFO goes through track.step(), and the VFOs that moved are retuned continuously and their
    meter rows restarted.  track_params: {"deadband_hz", "max_step_hz", "look_samples"} (absent / 0 = default).  `sondes[i]` follows
    the retunes; `track_log[i]` lists (first input sample of the submit the offset applies from, offset_hz, err_hz, level_db) per
    look acted on.  With track=True the granule of the "reference" chain also leaves whole 256-sample blocks at every VFO rate."""

    def __init__(self, rate_in: int, sondes, *, chain: str = "iq48", input_kind: int = INPUT_IQ, device: int = 0, max_in: int | None = None,
                 track: bool = False, track_params: dict | None = None, rescue: bool = False,
                 manchester_rescue: bool = False, dfm_rescue: bool = False, ims_rescue: bool = False,
                 afsk_rescue: bool = False):
        if chain not in ("iq48", "reference"):
            raise SondeError('chain must be "iq48" or "reference"')
        self.rate_in, self.chain, self.device, self.input_kind = int(rate_in), chain, int(device), int(input_kind)
        self.sondes = [(int(f), int(t)) for f, t in sondes]
        if not self.sondes:
            raise SondeError("no sondes")
        types = [t for _, t in self.sondes]
        fs = self.rate_in
        p = _chain.plan(fs, types, max_in, chain, track)
        self.granule, self.max_in = p.granule, p.max_in
        # batch channel c = order[c]: the sondes grouped by tuner, so that every group's rows are evenly spaced
        self.order = np.array([i for g in p.groups.values() for i in g], dtype=np.int64)
        self.stages = []          # (tuner, SondeVfo or None, first batch channel, sonde indices)
        self.track = bool(track)
        self.track_params = dict(track_params or {})
        self.track_log = [[] for _ in self.sondes]
        self.trackers = {}        # id(tuner) -> SondeTracker (track=True only)
        self._n_in = 0            # input samples submitted so far
        c0 = 0
        for rate, idx in p.groups.items():
            bws = [_chain.iq48_bandwidth(types[i]) if chain == "iq48" else rate for i in idx]
            tu = SondeTuner(fs, rate, [(self.sondes[i][0], b) for i, b in zip(idx, bws)], self.max_in, input_kind=input_kind, device=device)
            vo = SondeVfo(len(idx), rate, tu.out_samples(self.max_in), device=device) if chain == "reference" else None
            self.stages.append((tu, vo, c0, idx))
            if self.track:
                from .track import SondeTracker
                self.trackers[id(tu)] = SondeTracker(len(idx), tu.rate_out, tu.out_samples(self.max_in), device=device,
                                                     look_samples=int(self.track_params.get("look_samples", 0)))
            c0 += len(idx)
        kind = INPUT_IQ if chain == "iq48" else INPUT_REAL
        self.batch = _chain.batch(len(types), p.n48, [types[i] for i in self.order], device,
                                  (rescue, manchester_rescue, dfm_rescue, ims_rescue, afsk_rescue), kind)
        self._rows = _chain.rows(len(types), p.n48, device, kind)
        self._tmp = {}
        self._n48 = 0
        self._inv = np.empty(len(types), dtype=np.int64)
        self._inv[:] = self.order          # batch channel -> sonde index

    def _where(self, i: int):
        for tu, _, _, idx in self.stages:
            if i in idx:
                return tu, idx.index(i)
        raise SondeError("no such sonde")

    def retune(self, i: int, hz: int, continuous: bool = False):
        """sonde i's VFO to offset hz from the next submit on (SondeTuner.retune)"""
        tu, k = self._where(int(i))
        tu.retune(k, hz, continuous)
        if self.track:
            self.trackers[id(tu)].restart(k)          # no look straddles two offsets
        self.sondes[i] = (int(hz), self.sondes[i][1])

    def _track_update(self):
        """the loop (SPEC 3.11): the newest look of every VFO -> step -> continuous retune + restart for those that moved"""
        for tu, _, _, idx in self.stages:
            for k, new, err, level in _chain.track_looks(self.trackers[id(tu)], tu, self.rate_in, self.track_params):
                if new != tu.offsets[k]:
                    self.retune(idx[k], new, continuous=True)
                self.track_log[idx[k]].append((self._n_in, new, err, level))

    def rows(self):
        """the 48 kHz rows of the last submit, in batch-channel order (IQ [C, n, 2] for iq48, FM [C, n] for reference)"""
        return self._rows[:, :self._n48]

    def submit(self, block, stream: int | None = None):
        import torch
        n = int(block.shape[0])
        _chain.check_block(n, self.granule, self.max_in)
        if stream is None:
            stream = current_stream(self.device)
        n48 = _chain.out48(self.rate_in, n)
        if self.track and self._n_in:
            self._track_update()
        for tu, vo, c0, idx in self.stages:
            nv = len(idx)
            if vo is None:
                tu.process(block, out=self._rows[c0:c0 + nv], stream=stream)
                if self.track:
                    self.trackers[id(tu)].submit(self._rows[c0:c0 + nv, :n48], stream)
            else:
                m = tu.out_samples(n)
                buf = self._tmp.get(id(tu))
                if buf is None or buf.shape[1] < m:
                    buf = self._tmp[id(tu)] = torch.empty((nv, tu.out_samples(self.max_in), 2), dtype=torch.float32, device=block.device)
                tu.process(block, out=buf, stream=stream)
                if self.track:
                    self.trackers[id(tu)].submit(buf[:, :m], stream)
                vo.process(buf[:, :m], out=self._rows[c0:c0 + nv], stream=stream)
        self._n48 = n48
        self._n_in += n
        self.batch.submit(self._rows[:, :n48], stream)

    def frames(self) -> np.ndarray:
        f = self.batch.frames()
        f["channel"] = self._inv[f["channel"]]
        return f

    def poll(self):
        """[(sonde index, SondeData), ...] of the last submit (SondeBatch.poll)"""
        return [(int(self._inv[c]), d) for c, d in self.batch.poll()]

    def close(self):
        for tu, vo, _, _ in self.stages:
            tu.close()
            if id(tu) in self.trackers:
                self.trackers.pop(id(tu)).close()
            if vo is not None:
                vo.close()
        self.stages = []
        self.batch.close()
