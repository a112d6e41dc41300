#!/usr/bin/env python3
"""Every host-made table that has an accessor, as bytes, with a SHA-256 per table: tools/dump_tables.py OUT.bin
Run it once per library (SONDE_MI355_LIB=... selects the library, one process each) and compare the files: a change that only
moves host code must leave every table as it was, byte for byte.  Host functions only: no GPU is needed."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdrpp_radiosonde_amd import _lib  # noqa: E402

L = _lib.load()
tables = []


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


for rate in (10000, 15000, 20000, 40000, 50000):
    up, down = C.c_int(), C.c_int()
    assert L.sonde_vfo_ratio(rate, C.byref(up), C.byref(down)) == 0
    g = np.zeros(up.value * 16, dtype=np.float32)
    assert L.sonde_vfo_taps(rate, vp(g)) == 0
    tables.append((f"vfo_taps {rate}", g))

h, tw, g = np.zeros(8192, np.float32), np.zeros(512, np.float32), np.zeros(192, np.float32)
assert L.sonde_chan_tables(vp(h), vp(tw), vp(g)) == 0
tables += [("chan h", h), ("chan tw", tw), ("chan g", g)]

for fs, r, bws in ((10000000, 48000, (0, 5000, 10000, 20000, 48000)), (1000000, 48000, (10000,)), (2400000, 20000, (0,))):
    for bw in bws:
        n = L.sonde_tuner_taps(fs, r, bw, None, 0)
        assert n > 0, _lib.last_error()
        g = np.zeros(n, dtype=np.float32)
        assert L.sonde_tuner_taps(fs, r, bw, vp(g), n) == n
        tables.append((f"tuner_taps {fs} {r} {bw}", g))

for n in (1024, 16384):
    w = np.zeros(n, dtype=np.float32)
    assert L.sonde_scan_window(n, vp(w), n) == n
    tables.append((f"scan_window {n}", w))

with open(sys.argv[1], "wb") as f:
    for name, a in tables:
        assert np.isfinite(a).all() and a.any(), name
        f.write(a.tobytes())
        print(f"{hashlib.sha256(a.tobytes()).hexdigest()[:16]}  {a.size:8d}  {name}")
print("library:", _lib.LIB_PATH)
