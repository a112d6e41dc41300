"""Python face of a receiver with several antennas (DESIGN SPEC 3.3k): thin, no compute -- every call goes through the C ABI of
libsonde_mi355.so.

    DiversityReceiver   K wideband streams (one per antenna or polarisation, started whenever) -> K tuners with the same VFO list ->
                        one SondeBatch in which the K channels of each sonde are a diversity group that learns its own offsets and
                        marks duplicates -> one frame list per sonde

    combine="coherent"  the same K tuners -> one SondeCombiner (combine.py, SPEC 3.14), which adds the K rows of each sonde before
                        detection -> one SondeBatch of one channel per sonde: any sonde type, the antennas on one sample clock

The chain is WidebandReceiver's "iq48" (tuner.py): a tuner per antenna straight to 48 kHz IQ rows.  combine="frames" (the default):
RS41 sondes only.  No tracking, no reference chain."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import FRAME_DUPLICATE, INPUT_IQ, TILE
from .batch import VFO_RATE, SondeBatch, SondeError
from .tuner import AFSK_TILE, C50, IMET4, IQ48_MAX_BW, SondeTuner, _lcm, _multiple_for, ratio

RS41 = 0


class DiversityReceiver:
    """sondes: [(offset_hz, sonde type), ...], every type RS41; antennas = K = 2..4 wideband streams at rate_in that hear them.
    Batch channel a * len(sondes) + i is sonde i on antenna a; the K channels of sonde i are diversity group i, antenna a its member a,
    set with learn=True, mark_duplicates=True and no offsets: the streams need not start together, the group finds out where they
    stand from the first frame that is good on two antennas (SondeBatch.set_diversity).

    submit(blocks) takes K device blocks [n, 2] of equal length (float32 / int16 / int8 by input_kind), n a multiple of `granule`
    and <= max_in.  frames() returns (records, antenna): the last submit's records without the duplicates, `channel` = the sonde
    index, antenna[j] = the antenna that record j was received on (a combined record: the antenna whose copy was rewritten).  poll()
    returns [(sonde index, SondeData)], duplicates left out.  offsets(i) = SondeBatch.diversity_offsets of sonde i: where each
    antenna's bit count stands, which antennas are locked, the counters.

    combine="coherent" (SPEC 3.14): sondes of any type; the K streams come from one coherent SDR, on one sample clock, started together,
    with equal noise floors.  Each tuner's VFO k has the bandwidth WidebandReceiver's "iq48" chain picks for its type; one
    SondeCombiner (block length combine_block, 0 = default) adds the K rows of each sonde, weights per block from the block itself,
    into the input rows of a SondeBatch of len(sondes) channels with these types and no diversity groups; the rescue keywords are
    WidebandReceiver's.  frames() returns (records, antenna) with antenna -1 everywhere, poll() [(sonde index, SondeData)];
    offsets() is refused; weights(i) returns the last submit's shares |w_a|^2 of sonde i, [blocks, K]."""

    def __init__(self, rate_in: int, sondes, antennas: int = 2, *, input_kind: int = INPUT_IQ, device: int = 0, max_in: int | None = None,
                 window_bits: int = 0, rescue: bool = False, chain: str = "iq48", track: bool = False, combine: str = "frames",
                 combine_block: int = 0, manchester_rescue: bool = False, dfm_rescue: bool = False, ims_rescue: bool = False,
                 afsk_rescue: bool = False):
        import torch
        if chain != "iq48":
            raise SondeError('DiversityReceiver: only the "iq48" chain')
        if track:
            raise SondeError("DiversityReceiver: no tracking")
        if combine not in ("frames", "coherent"):
            raise SondeError('combine must be "frames" or "coherent"')
        self.combine = combine
        self.sondes = [(int(f), int(t)) for f, t in sondes]
        if not self.sondes:
            raise SondeError("no sondes")
        if combine == "coherent":
            self._init_coherent(rate_in, antennas, input_kind, device, max_in, combine_block,
                                _lib.rescue_flags(rescue, manchester_rescue, dfm_rescue, ims_rescue, afsk_rescue))
            return
        if manchester_rescue or dfm_rescue or ims_rescue or afsk_rescue:
            raise SondeError('DiversityReceiver: combine="frames" is RS41 only and takes no rescue pass but rescue=')
        if any(t != RS41 for _, t in self.sondes):
            raise SondeError("DiversityReceiver: RS41 sondes only (the diversity pass is RS41's)")
        self.antennas = int(antennas)
        if not 2 <= self.antennas <= 4:
            raise SondeError("DiversityReceiver: 2..4 antennas")
        self.rate_in, self.device, self.input_kind = int(rate_in), int(device), int(input_kind)
        fs, S, K = self.rate_in, len(self.sondes), self.antennas
        self.granule = _lcm(ratio(fs, 48000)[1], _multiple_for(48000, fs, TILE))
        self.max_in = int(max_in or self.granule)
        if self.max_in % self.granule:
            raise SondeError(f"max_in must be a multiple of the granule ({self.granule})")
        n48 = self.max_in * 48000 // fs
        vfos = [(f, min(VFO_RATE[RS41], IQ48_MAX_BW)) for f, _ in self.sondes]
        self.tuners = [SondeTuner(fs, 48000, vfos, self.max_in, input_kind=input_kind, device=device) for _ in range(K)]
        self.batch = SondeBatch(K * S, n48, types=np.zeros(K * S, dtype=np.uint8), input_kind=INPUT_IQ, device=device,
                                flags=_lib.FLAG_RS41_RESCUE if rescue else 0)
        self.batch.set_diversity([[a * S + i for a in range(K)] for i in range(S)], None, window_bits, learn=True, mark_duplicates=True)
        stride = int(_lib.load().sonde_row_stride(n48, INPUT_IQ))
        self._rows = torch.empty((K * S, stride, 2), dtype=torch.float32, device=f"cuda:{device}")
        self._n48 = 0

    def _init_coherent(self, rate_in, antennas, input_kind, device, max_in, combine_block, flags):
        import torch
        from .combine import SondeCombiner
        self.antennas = int(antennas)
        if not 2 <= self.antennas <= 4:
            raise SondeError("DiversityReceiver: 2..4 antennas")
        self.rate_in, self.device, self.input_kind = int(rate_in), int(device), int(input_kind)
        fs, S, K = self.rate_in, len(self.sondes), self.antennas
        types = [t for _, t in self.sondes]
        tile = AFSK_TILE if any(t in (IMET4, C50) for t in types) else TILE
        self.granule = _lcm(ratio(fs, 48000)[1], _multiple_for(48000, fs, tile))
        self.max_in = int(max_in or self.granule)
        if self.max_in % self.granule:
            raise SondeError(f"max_in must be a multiple of the granule ({self.granule})")
        n48 = self.max_in * 48000 // fs
        vfos = [(f, min(VFO_RATE[t], IQ48_MAX_BW)) for f, t in self.sondes]
        self.tuners = [SondeTuner(fs, 48000, vfos, self.max_in, input_kind=input_kind, device=device) for _ in range(K)]
        self.combiner = SondeCombiner(S, K, 48000, n48, combine_block, device)
        g48 = self.granule * 48000 // fs
        if g48 % self.combiner.block:
            raise SondeError(f"combine_block must divide the granule's {g48} samples at 48 kHz")
        self.batch = SondeBatch(S, n48, types=np.array(types, dtype=np.uint8), input_kind=INPUT_IQ, device=device, flags=flags)
        stride = int(_lib.load().sonde_row_stride(n48, INPUT_IQ))
        self._ant = torch.empty((K * S, n48, 2), dtype=torch.float32, device=f"cuda:{device}")      # the tuners' rows
        self._rows = torch.empty((S, stride, 2), dtype=torch.float32, device=f"cuda:{device}")      # the combined rows: the batch's input
        self._n48 = 0

    def submit(self, blocks, stream: int | None = None):
        import torch
        if len(blocks) != self.antennas:
            raise SondeError(f"submit takes {self.antennas} blocks, one per antenna")
        n = int(blocks[0].shape[0])
        if any(int(b.shape[0]) != n for b in blocks):
            raise SondeError("the antennas' blocks must be of equal length")
        if n == 0 or n % self.granule or n > self.max_in:
            raise SondeError(f"the blocks must hold a positive multiple of the granule ({self.granule}) samples, at most max_in ({self.max_in})")
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        S = len(self.sondes)
        self._n48 = n * 48000 // self.rate_in
        if self.combine == "coherent":
            for a, (tu, block) in enumerate(zip(self.tuners, blocks)):
                tu.process(block, out=self._ant[a * S:(a + 1) * S], stream=stream)
            self.combiner.process(self._ant[:, :self._n48], out=self._rows, stream=stream)
            self.batch.submit(self._rows[:, :self._n48], stream)
            return
        for a, (tu, block) in enumerate(zip(self.tuners, blocks)):
            tu.process(block, out=self._rows[a * S:(a + 1) * S], stream=stream)
        self.batch.submit(self._rows[:, :self._n48], stream)

    def frames(self):
        f = self.batch.frames()
        if self.combine == "coherent":
            return f, np.full(len(f), -1, dtype=np.int64)
        f = f[(f["flags"] & FRAME_DUPLICATE) == 0]
        S = len(self.sondes)
        antenna = (f["channel"] // S).astype(np.int64)
        f["channel"] = f["channel"] % S
        return f, antenna

    def poll(self):
        S = len(self.sondes)
        return [(int(c) % S, d) for c, d in self.batch.poll()]

    def offsets(self, i: int) -> dict:
        if self.combine == "coherent":
            raise SondeError('DiversityReceiver: combine="coherent" has no offsets (the antennas start together); see weights()')
        if not 0 <= int(i) < len(self.sondes):
            raise SondeError("no such sonde")
        return self.batch.diversity_offsets(int(i))

    def weights(self, i: int) -> np.ndarray:
        """combine="coherent": the shares |w_a|^2 of sonde i over the last submit's blocks, [blocks, antennas] (this synchronises)"""
        if self.combine != "coherent":
            raise SondeError('DiversityReceiver: combine="frames" has no weights; see offsets()')
        if not 0 <= int(i) < len(self.sondes):
            raise SondeError("no such sonde")
        from .combine import share
        r = self.combiner.readout()
        r = r[r["sonde"] == int(i)]
        w = r["w"][:, 0::2] + 1j * r["w"][:, 1::2]
        return np.array([[share(wb, a) for a in range(self.antennas)] for wb in w]).reshape(len(w), self.antennas)

    def close(self):
        for tu in self.tuners:
            tu.close()
        self.tuners = []
        if getattr(self, "combiner", None) is not None:
            self.combiner.close()
            self.combiner = None
        self.batch.close()
