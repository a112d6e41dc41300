"""Python face of a receiver with several antennas (DESIGN SPEC 3.3k): thin, no compute -- every call goes through the C ABI of
libsonde_mi355.so.

    DiversityReceiver   K wideband streams (one per antenna or polarisation, started whenever) -> K tuners with the same VFO list ->
                        one SondeBatch in which the K channels of each sonde are a diversity group that learns its own offsets and
                        marks duplicates -> one frame list per sonde

The chain is WidebandReceiver's "iq48" (tuner.py): a tuner per antenna straight to 48 kHz IQ rows.  RS41 sondes only; no tracking, no
reference chain."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import FRAME_DUPLICATE, INPUT_IQ, TILE
from .batch import VFO_RATE, SondeBatch, SondeError
from .tuner import IQ48_MAX_BW, SondeTuner, _lcm, _multiple_for, ratio

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
    antenna's bit count stands, which antennas are locked, the counters."""

    def __init__(self, rate_in: int, sondes, antennas: int = 2, *, input_kind: int = INPUT_IQ, device: int = 0, max_in: int | None = None,
                 window_bits: int = 0, rescue: bool = False, chain: str = "iq48", track: bool = False):
        import torch
        if chain != "iq48":
            raise SondeError('DiversityReceiver: only the "iq48" chain')
        if track:
            raise SondeError("DiversityReceiver: no tracking")
        self.sondes = [(int(f), int(t)) for f, t in sondes]
        if not self.sondes:
            raise SondeError("no sondes")
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
        for a, (tu, block) in enumerate(zip(self.tuners, blocks)):
            tu.process(block, out=self._rows[a * S:(a + 1) * S], stream=stream)
        self._n48 = n * 48000 // self.rate_in
        self.batch.submit(self._rows[:, :self._n48], stream)

    def frames(self):
        f = self.batch.frames()
        f = f[(f["flags"] & FRAME_DUPLICATE) == 0]
        S = len(self.sondes)
        antenna = (f["channel"] // S).astype(np.int64)
        f["channel"] = f["channel"] % S
        return f, antenna

    def poll(self):
        S = len(self.sondes)
        return [(int(c) % S, d) for c, d in self.batch.poll()]

    def offsets(self, i: int) -> dict:
        if not 0 <= int(i) < len(self.sondes):
            raise SondeError("no such sonde")
        return self.batch.diversity_offsets(int(i))

    def close(self):
        for tu in self.tuners:
            tu.close()
        self.tuners = []
        self.batch.close()
