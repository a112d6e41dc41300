"""What the stream-age tests share (DESIGN "Stream age"): the scenes, the arithmetic of a shift that puts an absolute position just
below a boundary, and the comparison helpers that judge an aged stream B against the unaged stream A of the same input.  The helpers
are plain numpy: tests/test_stream_age_reference.py runs them on the CPU oracle's output (and shows that they reject the bugs they
exist for), tests/test_gpu_stream_age.py on two SondeBatch objects."""
from __future__ import annotations

import functools

import numpy as np

import demod_reference as D
from test_demod_reference import Scene, make_input, scene_modem

Q = 30720                       # lcm(2048, 480): a shift by a multiple keeps the tile phase and both tone-mixer phases
WARM = 4                        # tiles before the first shift: SPEC 3.2b's acquisition rule is keyed on n0 <= 3 tiles
STAGE = 24                      # tiles per stage of the per-tile tests
SUBMIT = 24                     # tiles per submit (= max_samples) of the batches
MIXED, AFSK = (0, 1, 2, 3, 6), (4, 5)
# the shortest frame of each type in ring bits (chips for the Manchester / biphase types; iMet and C50: characters of 10 bits)
MIN_FRAME_BITS = {0: 320 * 8, 1: 560, 2: 1152, 3: 1648, 4: 140, 5: 90, 6: 768}


def tile_in(S) -> int:
    return D.TILE * (8 if any(s.stype in AFSK for s in S) else 1)


def div_of(s: Scene) -> int:
    """input samples per internal sample of the scene's channel: the class decimation, 8 behind the tone front-end"""
    m = scene_modem(s)
    return m.decim * m.pre


def ring_bits(S, max_samples: int = SUBMIT * D.TILE) -> int:
    """the bit ring's length of a batch of the scenes S"""
    return ring_bits_of([scene_modem(s) for s in S], max_samples)


def ring_bits_of(modems, max_samples: int) -> int:
    """the bit ring's length as sonde_batch_create sizes it: a submit of the fastest type at the fastest clock the loop allows, a
    frame and 1024 bits, rounded up to a power of two of 32-bit words"""
    most = 0
    for m in modems:
        pmin = m.period0 - (m.period0 >> 8)
        most = max(most, ((max_samples // (m.decim * m.pre)) << 16) // pmin + 2)
    words = (most + 8 * 528 + 1024 + 31) // 32
    p = 1
    while p < words:
        p <<= 1
    return 32 * p


def submits_to_cross(S, max_samples: int = SUBMIT * D.TILE) -> int:
    """submits of max_samples after which every channel has produced a ring's length of bits and one more frame of its type (at the
    slowest clock the loop allows), so that a position less than a ring below a boundary has crossed it with a whole frame behind"""
    worst = 0
    for s in S:
        m = scene_modem(s)
        pmax = m.period0 + (m.period0 >> 8)
        per_submit = ((max_samples // (m.decim * m.pre)) << 16) // pmax
        worst = max(worst, -(-(ring_bits(S, max_samples) + 2 * MIN_FRAME_BITS[s.stype]) // per_submit))
    return worst


@functools.lru_cache(maxsize=None)
def scene_set(name: str):
    """(scenes, inputs) of one configuration: the 35-channel mixed set of test_gpu_demod_reference.scenes() as iq, iq with
    SONDE_FLAG_WIDE, iq16 and real, and the 32-channel AFSK set; long enough for the longest stage (the wpos stage; the per-tile
    stages use a prefix)"""
    from test_gpu_demod_reference import scenes
    if name == "afsk":
        S = scenes(AFSK, 32, "iq", seed=23)
    else:
        kind, wide = {"iq": ("iq", False), "iq-wide": ("iq", True), "iq16": ("iq16", False), "real": ("real", False)}[name]
        S = scenes(MIXED, 35, kind, wide=wide, seed=7)
    import dataclasses
    per = tile_in(S) // D.TILE
    # input tiles of 2048: the wpos stage (a warm-up submit and the submits to cross), the per-tile stages (the AFSK set has one more)
    tiles = max(SUBMIT * (1 + submits_to_cross(S)), WARM * per + (STAGE * 3 if per == 1 else 6 * per * 4))
    S = [dataclasses.replace(s, ntiles=-(-tiles // per)) for s in S]
    return S, [make_input(s) for s in S]


def samples_below(boundary: int, now: int, div: int = 1) -> int:
    """the largest shift (input samples, a multiple of Q) that leaves a position counted in units of `div` input samples, now at `now`,
    below `boundary`: it lands less than Q / div below it"""
    assert now < boundary
    return (boundary - 1 - now) * div // Q * Q


def turns_below(boundary: int, nbits: int, ring: int) -> int:
    """whole ring turns that leave a bit position now at `nbits` below `boundary`: it lands less than a ring's length below it"""
    assert nbits < boundary
    return (boundary - 1 - nbits) // ring


# ---------------------------------------------------------------- the comparisons
def state_diff(a: dict, b: dict, dt: int) -> list:
    """what distinguishes the aged channel's state b from the unaged a: t_next must be a's plus dt (Q16), the rest equal exactly"""
    why = [k for k in ("period", "bias", "amp", "afc_u") if a[k] != b[k]]
    if b["t_next"] != a["t_next"] + dt:
        why.append(f"t_next {b['t_next']} != {a['t_next']} + {dt}")
    return why


def frames_diff(fa: np.ndarray, fb: np.ndarray, added) -> list:
    """what distinguishes the aged records fb from the unaged fa once added[channel] bits are taken off bitpos: byte for byte"""
    if len(fa) != len(fb):
        return [f"{len(fb)} records, not {len(fa)}"]
    if not len(fa):
        return []
    fb = fb.copy()
    add = np.asarray([int(added[int(c)]) for c in fb["channel"]], dtype=np.uint64)
    early = fb["bitpos"] < add
    if early.any():
        return [f"channel {int(fb['channel'][early][0])}: bitpos {int(fb['bitpos'][early][0])} below the shift"]
    fb["bitpos"] -= add
    fa = fa[np.lexsort((fa["bitpos"], fa["channel"]))]
    fb = fb[np.lexsort((fb["bitpos"], fb["channel"]))]
    return [f"channel {int(a['channel'])} bitpos {int(a['bitpos'])}" for a, b in zip(fa, fb) if a.tobytes() != b.tobytes()]


def frame_bits(f) -> int:
    """ring bits a record's frame takes at least (the record's own length where the type's frames vary)"""
    t = int(f["type"])
    return max(MIN_FRAME_BITS[t], (8 if t == 0 else 10 if t in AFSK else 0) * int(f["len"]))


def spanning_types(frames: np.ndarray, added, boundary: int) -> set:
    """the sonde types with a record whose bits, at bitpos + added[channel], span `boundary` (first bit below it, last bit at or
    beyond it)"""
    out = set()
    for f in frames:
        p = int(f["bitpos"]) + int(added[int(f["channel"])])
        if p < boundary <= p + frame_bits(f) - 1:
            out.add(int(f["type"]))
    return out
