"""What the object wrappers of this package share (private): the error check of a C entry, the handle every wrapper owns, and
the argument checks of the three kinds of device tensor the library takes (the C side sees only a pointer)."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import INPUT_IQ, INPUT_IQ8, INPUT_IQ16, SondeError


def chk(rc):
    """the result of an int- or long-returning entry (include/sonde_abi.h: negative = error, text via sonde_last_error())"""
    if rc < 0:
        raise SondeError(_lib.last_error())
    return rc


def current_stream(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


class Handle:
    """One library object: `L` the loaded library, `h` its handle (None once closed), DESTROY the name of the entry that frees
    it.  close() may be called any number of times; a wrapper that is dropped closes itself.

    The default stream is each object's own and differs: SondeBatch, SondeDetector and SondeChannelizer take stream=None as the
    null stream (`stream or 0`); SondeVfo, SondeTuner, SondeScanner, SondeTracker and SondeCombiner look up torch's current
    stream of the tensor's device."""
    DESTROY = ""
    h = None

    def _create(self, entry: str, *args):
        """self.h = the object `entry` makes from args (every create entry returns it through its last argument)"""
        self.L = _lib.load()
        h = C.c_void_p()
        chk(getattr(self.L, entry)(*args, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            getattr(self.L, self.DESTROY)(self.h)
            self.h = None

    def __del__(self):          # guarded: at interpreter shutdown the library or this module may be gone already
        try:
            self.close()
        except Exception:
            pass


def _dtype_name(kind: int) -> str:
    return {INPUT_IQ16: "int16", INPUT_IQ8: "int8"}.get(kind, "float32")


def channel_rows(samples, kind: int, n_channels: int, device: int, noun: str):
    """(n, channel stride in samples) of the rows a batch or a detector takes: [C, n, 2] (IQ kinds) or [C, n] (INPUT_REAL), the dtype
    of `kind`, on `device`, contiguous inside a channel"""
    shape = tuple(samples.shape)
    if shape[0] != n_channels:
        raise SondeError("first dimension must be n_channels")
    is_iq = kind in (INPUT_IQ, INPUT_IQ16, INPUT_IQ8)
    if is_iq and (len(shape) != 3 or shape[2] != 2):
        raise SondeError("IQ input must be [C, n, 2] (float32; int16 for INPUT_IQ16, int8 for INPUT_IQ8)")
    if not is_iq and len(shape) != 2:
        raise SondeError("real input must be [C, n] float32")
    dt, want = str(getattr(samples, "dtype", "")), _dtype_name(kind)
    if not dt.endswith(want) or dt.endswith("u" + want):
        raise SondeError(f"samples must be {want}, got {dt}")
    dev = getattr(samples, "device", None)
    if dev is None or getattr(dev, "type", "") != "cuda":
        raise SondeError("samples must be a device (HIP) tensor" + ("; use submit_host() for host memory" if noun == "batch" else ""))
    if dev.index is not None and dev.index != device:
        raise SondeError(f"samples live on device {dev.index}, the {noun} on device {device}")
    st = tuple(samples.stride())
    if (is_iq and st[1:] != (2, 1)) or (not is_iq and st[1] != 1):
        raise SondeError("samples must be contiguous inside a channel (only the channel stride may be padded)")
    return shape[1], st[0] // (2 if is_iq else 1)


def wideband_block(block, kind: int, device: int, noun: str) -> int:
    """n_in of the block a tuner or a scanner takes: [n_in, 2], contiguous, the dtype of `kind`, on `device`"""
    import torch
    want = getattr(torch, _dtype_name(kind))
    if block.dtype != want:
        raise SondeError(f"the wideband block must be {want}, got {block.dtype}")
    if not block.is_cuda or block.dim() != 2 or block.shape[1] != 2 or not block.is_contiguous():
        raise SondeError("the wideband block must be a contiguous device tensor [n_in, 2]")
    if block.device.index is not None and block.device.index != device:
        raise SondeError(f"the block lives on device {block.device.index}, the {noun} on device {device}")
    return block.shape[0]


def complex_stride(t):
    """the row stride, in complex samples, of a float32 device view [R, n, 2] whose rows are contiguous inside and lie any even
    number of floats apart; None for anything else"""
    import torch
    if (t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or t.shape[2] != 2 or t.stride(2) != 1 or t.stride(1) != 2
            or (t.shape[0] > 1 and t.stride(0) % 2)):
        return None
    return t.stride(0) // 2 if t.shape[0] > 1 else max(t.stride(0) // 2, t.shape[1])


def complex_rows(rows, n_rows: int, device: int, noun: str, dims: str, made_for, carries: str):
    """(n, row stride in complex samples) of the n_rows complex64 rows a meter or a combiner takes; dims, made_for and carries are
    the owner's words for its rows"""
    stride = complex_stride(rows)
    if stride is None:
        raise SondeError(f"the rows must be a float32 device view [{dims}, n, 2], contiguous inside a row (complex64: REAL rows carry no {carries})")
    if rows.shape[0] != n_rows:
        raise SondeError(f"the {noun} was created for {made_for} rows, got {rows.shape[0]}")
    if rows.device.index is not None and rows.device.index != device:
        raise SondeError(f"the rows live on device {rows.device.index}, the {noun} on device {device}")
    return rows.shape[1], stride
