"""MI355X-native radiosonde demod + FEC path: ctypes binding of libsonde_mi355.so (include/sonde_abi.h).

    _lib      the raw C ABI (argtypes / restypes), constants, structures, SondeError
    _handle   private: what the object wrappers share (the error check, the handle with close(), the checks of the tensors they take)
    _chain    private: what the three receivers share (block arithmetic, iq48 bandwidths, batch and row buffer, the tracking loop)
    batch     SondeBatch (many 48 kS/s channels), SondeChannelizer (10 MS/s -> 512 bins), SondeVfo (VFO-rate front-end)
    detect    SondeDetector: the sonde type of each channel (sync-template correlation on the GPU); detect, then build the batch
    tuner     SondeTuner (VFOs at any offset over one wideband stream), WidebandReceiver (wideband stream -> tuner -> decoders)
    scan      SondeScanner (where in a wideband stream the carriers are: averaged power spectrum on the GPU, candidate search), survey
    diversity DiversityReceiver (K antennas' wideband streams -> one frame list per RS41, M10 / M20 or MRZ-N1 sonde: the diversity pass with learned offsets;
              combine="coherent": the antennas' rows added before detection, any sonde type)
    combine   SondeCombiner (the K antennas' IQ rows of each sonde -> one row: weights per block from the block's own statistics)
    live      LiveReceiver (a wideband receiver left running: sondes that appear are probed, typed and decoded, those that vanish dropped), LivePolicy
    node      SondeNode: the one-process node-level host (libsonde_rccl.so, include/sonde_node.h): one batch per GPU, RCCL scatter of IQ rows
    shard     channel sharding for a rank-per-GPU host on plain torch.distributed (range arithmetic, scatter, frame gather)
    synth     synthetic signal generator for all seven sonde types (tests and bench; independent of the decoders' code)

Nothing here computes on the CPU: every entry point needs the HIP library and a GPU (no fallback)."""


def __getattr__(name):          # `from sdrpp_radiosonde_amd import LiveReceiver`, without importing anything before it is asked for
    if name in ("LiveReceiver", "LivePolicy"):
        from . import live
        return getattr(live, name)
    if name == "DiversityReceiver":
        from . import diversity
        return diversity.DiversityReceiver
    if name == "SondeCombiner":
        from . import combine
        return combine.SondeCombiner
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
