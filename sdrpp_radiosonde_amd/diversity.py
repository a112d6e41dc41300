"""Python face of a receiver with several antennas (DESIGN SPEC 3.3k, 3.3l, 3.3m, 3.3n, 3.3o): thin, no compute -- every call goes through the C ABI of
libsonde_mi355.so.

    DiversityReceiver   K wideband streams (one per antenna or polarisation, started whenever) -> K tuners with the same VFO list ->
                        one SondeBatch in which the K channels of each sonde are a diversity group that learns its own offsets and
                        marks duplicates -> one frame list per sonde

    combine="coherent"  the same K tuners -> one SondeCombiner (combine.py, SPEC 3.14), which adds the K rows of each sonde before
                        detection -> one SondeBatch of one channel per sonde: any sonde type, the antennas on one sample clock

The chain is the "iq48" chain of _chain.py, which WidebandReceiver (tuner.py) and LiveReceiver share: a tuner per antenna straight to
48 kHz IQ rows.  combine="frames" (the default): RS41, M10 / M20 and MRZ-N1 sondes, in any mix, and with dfm_diversity=True DFM sondes, with
ims_diversity=True iMS-100 sondes, with afsk_diversity=True iMet sondes too.  No tracking, no reference chain."""
from __future__ import annotations

import numpy as np

from . import _chain
from ._handle import current_stream
from ._lib import DFM09, FLAG_AFSK_DIVERSITY, FLAG_IMS_DIVERSITY, FRAME_DUPLICATE, IMET4, IMS100, INPUT_IQ, M10, MRZN1, RS41, SondeError
from .tuner import SondeTuner


class DiversityReceiver:
    """sondes: [(offset_hz, sonde type), ...], every type RS41, M10 (M10 and M20) or MRZN1, with dfm_diversity=True DFM09, with ims_diversity=True IMS100, with afsk_diversity=True IMET4 too; antennas = K = 2..4 wideband streams at rate_in that hear them.
    Batch channel a * len(sondes) + i is sonde i on antenna a; the K channels of sonde i are diversity group i, antenna a its member a,
    set with learn=True, mark_duplicates=True and no offsets: the streams need not start together, the group finds out where they
    stand from the first frame that is good on two antennas (SondeBatch.set_diversity).  rescue= (RS41) and manchester_rescue= (M10 /
    M20 / MRZ-N1) are the batch's second passes in front of the diversity pass; what they complete counts as a good copy.
    dfm_diversity=True: DFM sondes are taken as well (SPEC 3.3m: failed copies are combined word by word), and dfm_rescue= is passed on
    to the batch as the DFM second pass in front of it.
    ims_diversity=True: iMS-100 / RS-11G sondes are taken as well (SPEC 3.3n: failed copies are combined BCH block by block, from the
    chips; the batch is created with FLAG_IMS_DIVERSITY), and ims_rescue= is passed on to the batch as the iMS-100 second pass in front.
    afsk_diversity=True: iMet sondes are taken as well (SPEC 3.3o: failed copies are combined by their CRC; the batch is created with
    FLAG_AFSK_DIVERSITY), and afsk_rescue= is passed on to the batch as the iMet second pass in front.  XDATA packets are never marked
    as duplicates (they may repeat byte for byte): frames() returns every good copy of them.  C50 sondes are not taken: their packets
    carry no identity, so a C50 group has no learned offsets (SondeBatch.set_diversity with given offsets serves them).

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
                 afsk_rescue: bool = False, dfm_diversity: bool = False, ims_diversity: bool = False, afsk_diversity: bool = False):
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
        coherent = combine == "coherent"
        types = [t for _, t in self.sondes]
        if not coherent:
            if (dfm_rescue and not dfm_diversity) or (ims_rescue and not ims_diversity) or (afsk_rescue and not afsk_diversity):
                raise SondeError('DiversityReceiver: combine="frames" takes no rescue pass but rescue= and manchester_rescue=')
            served = (RS41, M10, MRZN1) + ((DFM09,) if dfm_diversity else ()) + ((IMS100,) if ims_diversity else ()) + ((IMET4,) if afsk_diversity else ())
            if any(t not in served for t in types):
                raise SondeError('DiversityReceiver: the frame-level pass serves M10 / M20, MRZ-N1 and RS41 sondes only (combine="coherent" takes any type)')
        self.antennas = int(antennas)
        if not 2 <= self.antennas <= 4:
            raise SondeError("DiversityReceiver: 2..4 antennas")
        self.rate_in, self.device, self.input_kind = int(rate_in), int(device), int(input_kind)
        fs, S, K = self.rate_in, len(self.sondes), self.antennas
        p = _chain.plan(fs, types, max_in)
        self.granule, self.max_in = p.granule, p.max_in
        vfos = [(f, _chain.iq48_bandwidth(t)) for f, t in self.sondes]
        self.tuners = [SondeTuner(fs, 48000, vfos, self.max_in, input_kind=input_kind, device=device) for _ in range(K)]
        passes = (rescue, manchester_rescue, dfm_rescue, ims_rescue, afsk_rescue)
        self._n48 = 0
        if coherent:          # the K rows of each sonde added before detection: one batch channel per sonde
            import torch
            from .combine import SondeCombiner
            self.combiner = SondeCombiner(S, K, 48000, p.n48, combine_block, device)
            g48 = _chain.out48(fs, self.granule)
            if g48 % self.combiner.block:
                raise SondeError(f"combine_block must divide the granule's {g48} samples at 48 kHz")
            self.batch = _chain.batch(S, p.n48, types, device, passes)
            self._ant = torch.empty((K * S, p.n48, 2), dtype=torch.float32, device=f"cuda:{device}")      # the tuners' rows
            self._rows = _chain.rows(S, p.n48, device)                                                   # the combined rows
        else:                 # one batch channel per antenna and sonde; the K channels of a sonde are a diversity group
            self.batch = _chain.batch(K * S, p.n48, types * K, device, passes, flags=(FLAG_IMS_DIVERSITY if ims_diversity else 0) | (FLAG_AFSK_DIVERSITY if afsk_diversity else 0))
            self.batch.set_diversity([[a * S + i for a in range(K)] for i in range(S)], None, window_bits, learn=True, mark_duplicates=True)
            self._rows = _chain.rows(K * S, p.n48, device)

    def submit(self, blocks, stream: int | None = None):
        if len(blocks) != self.antennas:
            raise SondeError(f"submit takes {self.antennas} blocks, one per antenna")
        n = int(blocks[0].shape[0])
        if any(int(b.shape[0]) != n for b in blocks):
            raise SondeError("the antennas' blocks must be of equal length")
        _chain.check_block(n, self.granule, self.max_in, "blocks")
        if stream is None:
            stream = current_stream(self.device)
        S = len(self.sondes)
        self._n48 = _chain.out48(self.rate_in, n)
        coherent = self.combine == "coherent"
        ant = self._ant if coherent else self._rows          # where the tuners write: antenna a's rows at a * S
        for a, (tu, block) in enumerate(zip(self.tuners, blocks)):
            tu.process(block, out=ant[a * S:(a + 1) * S], stream=stream)
        if coherent:
            self.combiner.process(ant[:, :self._n48], out=self._rows, stream=stream)
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
