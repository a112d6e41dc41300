"""Scenes for the SONDE_FLAG_AFSK_RESCUE tests (DESIGN SPEC 3.3i): iMet (PTU, GPS and XDATA packets) and SRS-C50 bit streams with
single bits flipped before the modulator, at 40 dB, so that every record's damage is known exactly.  Shared by the CPU tests of the
twin (test_afsk_rescue_reference.py) and the GPU tests (test_gpu_afsk_rescue.py); each scene and its oracle records are built once.
No damage goes into a channel's first packet.

Bit j (LSB index) of byte i of the packet that starts at bit `pos` is on the air at pos + 10 i + 1 + j (8N1, LSB first), so single
flips and pairs inside one byte never touch a start or stop bit and the framer records the packet with exactly that damage.

A case is a list of (byte, mask).  What each gives:
  data1   one bit of a data byte                          rescued, 1 flip
  check1  one bit of a stored check byte                  rescued, 1 flip
  pair    two neighbouring bits of one byte               rescued, 2 flips
  cross   bit 7 of byte i and bit 0 of byte i + 1         unsolved (pairs never span two bytes)
  two     iMet: two single bits in two different bytes    unsolved
          C50: a searched-for damage of two bits 6 / 7 of two data bytes that at least two patterns repair     ambiguous
C50's byte sums are weak, so its rescued cases stay where the repair is provably unique: a damage changes a byte by d, the sums by
(d, w d) mod 256 with w = 5..1 for bytes 2..6, and another byte's pattern repairs both only if (w - w') d = 0 mod 256, which needs
|d| >= 64.  The rescued cases therefore use bits 0..5 only (|d| <= 48), and cross uses bytes 3 | 4 (d = 128 + 1, w d = 4 128 + 3 = 3:
no single pattern undoes both)."""
from __future__ import annotations

import functools

import numpy as np

from sdrpp_radiosonde_amd import synth

TILE = 2048
IMET4, C50 = 4, 5
# kind -> (sonde type, channels, tiles, seed)
KINDS = {"imet": (IMET4, 3, 96, 81), "c50": (C50, 3, 96, 82)}
CASES = ["data1", "check1", "pair", "cross", "two", None]
EXPECT = {"imet": {"data1": ("rescued", 1), "check1": ("rescued", 1), "pair": ("rescued", 2), "cross": ("unsolved", 0), "two": ("unsolved", 0),
                   None: ("clean", 0)},
          "c50": {"data1": ("rescued", 1), "check1": ("rescued", 1), "pair": ("rescued", 2), "cross": ("unsolved", 0), "two": ("ambiguous", 0),
                  None: ("clean", 0)}}


def first_candidate(kind, pkt):
    return 2 if kind == "c50" else (3 if int(pkt[1]) == 3 else 2)


def c50_ok(pkt):
    """the C50 check, through the generator's own packet builder"""
    return np.array_equal(synth.c50_packet(int(pkt[2]), int.from_bytes(bytes(pkt[3:7]), "big"))[2:], pkt[2:])


def c50_fit_count(pkt):
    n = 0
    for i in range(2, 9):
        for m in [1 << j for j in range(8)] + [3 << j for j in range(7)]:
            t = pkt.copy()
            t[i] ^= m
            n += bool(c50_ok(t))
    return n


def _case_damage(kind, case, pkt, rng):
    ln, first = len(pkt), first_candidate(kind, pkt)
    top = 6 if kind == "c50" else 8                 # C50's rescued cases: bits 0..5 (module docstring)
    if case == "data1":
        return [(int(rng.integers(first, ln - 2)), 1 << int(rng.integers(0, top)))]
    if case == "check1":
        return [(int(rng.integers(ln - 2, ln)), 1 << int(rng.integers(0, top)))]
    if case == "pair":
        return [(int(rng.integers(first, ln)), 3 << int(rng.integers(0, top - 1)))]
    if case == "cross":
        i = 3 if kind == "c50" else int(rng.integers(first, ln - 1))
        return [(i, 0x80), (i + 1, 0x01)]
    if case == "two":
        if kind == "imet":
            i, k = sorted(int(v) for v in rng.choice(np.arange(first, ln), size=2, replace=False))
            return [(i, 1 << int(rng.integers(0, 8))), (k, 1 << int(rng.integers(0, 8)))]
        found = []
        for i in range(2, 7):
            for k in range(i + 1, 7):
                for mi in (0x40, 0x80):
                    for mk in (0x40, 0x80):
                        t = pkt.copy()
                        t[i] ^= mi
                        t[k] ^= mk
                        if not c50_ok(t) and c50_fit_count(t) >= 2:
                            found.append([(i, mi), (k, mk)])
        assert found, "no ambiguous two-bit damage for this packet"
        return found[int(rng.integers(0, len(found)))]
    raise KeyError(case)


class Scene:
    """iq [C, n, 2] float32 numpy; frames[c] = [(tx bit position of the first start bit, transmitted packet bytes)];
    plan[(c, pos)] = case or None"""


def _modulate(kind, bits, n, seed, snr_db):
    if kind == "c50":
        return synth.afsk_modulate(bits, n, seed=seed, snr_db=snr_db, baud=synth.C50_BAUD, mark_hz=synth.C50_MARK_HZ, space_hz=synth.C50_SPACE_HZ,
                                   fm_dev_hz=4000.0)[0]
    return synth.afsk_modulate(bits, n, seed=seed, snr_db=snr_db)[0]


def _build(kind, clean):
    typ, C, tiles, seed = KINDS[kind]
    n = TILE * tiles
    if kind == "c50":
        bits, frames = synth.c50_bitstreams(seed, np.arange(C), int(n * synth.C50_BAUD / 48000) + 16)
    else:
        bits, frames = synth.imet_bitstreams(seed, np.arange(C), int(n * synth.IMET_BAUD / 48000) + 16, xdata=True)
    bits = bits.copy()
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.plan = {}
    slot = 0
    for c in range(C):
        for k, (pos, pkt) in enumerate(frames[c]):
            case = None
            if not clean and k >= 1:
                case = CASES[slot % len(CASES)]
                slot += 1
            if case:
                for i, m in _case_damage(kind, case, pkt, rng):
                    for j in range(8):
                        if (m >> j) & 1:
                            bits[c, pos + 10 * i + 1 + j] ^= 1
            sc.plan[(c, pos)] = case
    iq = _modulate(kind, bits, n, seed, 40.0)
    sc.iq = iq.numpy() if hasattr(iq, "numpy") else np.asarray(iq)
    sc.frames, sc.kind, sc.type, sc.C, sc.n = frames, kind, typ, C, n
    return sc


@functools.lru_cache(maxsize=None)
def scene(kind, clean=False):
    return _build(kind, clean)


# ---- the noisy scenes.  iMet at 6 dB: over the oracle's records the brute-force search rescues 182 packets and every one of them was
# sent (checked on the CPU for this seed), so the test can assert both.  C50 at 6 dB: agreement with the twin only -- its weak check
# lets wrong repairs through.
NOISY = {"noisy_imet": dict(type=IMET4, channels=16, tiles=192, snr_db=6.0, seed=5),
         "noisy_c50": dict(type=C50, channels=4, tiles=96, snr_db=6.0, seed=5)}


@functools.lru_cache(maxsize=None)
def noisy_scene(kind):
    p = NOISY[kind]
    make = synth.make_imet_batch if p["type"] == IMET4 else synth.make_c50_batch
    sb = make(p["channels"], TILE * p["tiles"], seed=p["seed"], snr_db=p["snr_db"])
    sc = Scene()
    sc.iq = sb.iq.numpy()
    sc.frames, sc.kind, sc.type, sc.C, sc.n, sc.plan = sb.frames, kind, p["type"], p["channels"], TILE * p["tiles"], {}
    return sc


def scene_of(kind, clean=False):
    return noisy_scene(kind) if kind in NOISY else scene(kind, clean)


@functools.lru_cache(maxsize=None)
def oracle_run(kind, clean=False):
    """the records of the scene from the CPU oracle, in (channel, time) order (read-only)"""
    import oracle_lib
    oracle_lib.build()
    sc = scene_of(kind, clean)
    fr = oracle_lib.batch_run(sc.type, sc.iq, nthreads=4, cap_per_channel=sc.n // 2048 + 64)
    fr = fr[np.lexsort((fr["bitpos"], fr["channel"]))]
    fr.setflags(write=False)
    return fr


def tx_of(sc, f):
    """(tx bit position, transmitted bytes) of the record f; None: no transmitted packet starts there (a false sync).  The demodulators
    deliver a bit 6..13 bit times after it was sent; packets are 90 bits or more apart."""
    c = int(f["channel"])
    d, pos, tx = min(((abs(int(f["bitpos"]) - p), p, t) for p, t in sc.frames[c]), key=lambda t: t[0])
    return (pos, tx) if d <= 24 else None


# ---- caller-made records for the per-record routine (the twin on the CPU, sonde_batch_test_afsk_repair on the GPU): for every length
# the framer can record a kind of packet with, a valid packet of random content and EVERY pattern (8 single bits, 7 adjacent pairs) in
# EVERY byte, the bytes the pass must not touch included.  len 5: an XDATA packet without payload (only the CRC bytes are candidates);
# len 64: the longest record, a lane of the kernel's wave per byte.
EXHAUSTIVE = [("imet", 5), ("imet", 6), ("imet", 13), ("imet", 14), ("imet", 18), ("imet", 20), ("imet", 64), ("c50", 9)]
MASKS = [1 << j for j in range(8)] + [3 << j for j in range(7)]


def valid_packet(kind, ln, rng):
    if kind == "c50":
        return synth.c50_packet(int(rng.integers(0, 256)), int(rng.integers(0, 1 << 32)))
    ptype = {14: 1, 18: 2, 20: 4}.get(ln, 3)
    body = np.concatenate([np.array([1, ptype], dtype=np.uint8), rng.integers(0, 256, size=ln - 4, dtype=np.uint8)])
    if ptype == 3:
        body[2] = ln - 5
    c = synth.imet_crc(body)
    return np.concatenate([body, np.array([c >> 8, c & 0xFF], dtype=np.uint8)])


@functools.lru_cache(maxsize=None)
def exhaustive_records():
    """(records [n] FRAME_DTYPE with nerr[0] = -1, originals [n] of them with nerr[0] = 0, [(kind, len, byte, mask)])"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(83)
    what = [(kind, ln, i, m) for kind, ln in EXHAUSTIVE for i in range(ln) for m in MASKS]
    rec = np.zeros(len(what), dtype=FRAME_DTYPE)
    orig = np.zeros(len(what), dtype=FRAME_DTYPE)
    pkts = {(kind, ln): valid_packet(kind, ln, rng) for kind, ln in EXHAUSTIVE}
    for k, (kind, ln, i, m) in enumerate(what):
        for r in (rec, orig):
            r[k]["channel"], r[k]["type"], r[k]["len"], r[k]["bitpos"] = k % 7, KINDS[kind][0], ln, 1000 + k
            r[k]["flags"] = k & 1
            r[k]["data"][:ln] = pkts[(kind, ln)]
        rec[k]["data"][i] ^= m
        rec[k]["nerr"][0] = -1
    rec.setflags(write=False)
    orig.setflags(write=False)
    return rec, orig, what
