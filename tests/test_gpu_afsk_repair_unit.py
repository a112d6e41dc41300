"""-m gpu: the per-record routine of SONDE_FLAG_AFSK_RESCUE alone (sonde_batch_test_afsk_repair, DESIGN SPEC 3.3i steps 1..5) against the
twin (tests/afsk_rescue_reference.py) on caller-made records: for iMet lengths 5 (only the CRC bytes are candidates), 6, 13, 14, 18,
20 and 64 (a lane per byte) and for C50, every single-bit and adjacent-pair pattern in every byte, the bytes the pass must not touch
included; records that are not eligible; and records with more damage than one pattern.  Statuses and whole records must be the
twin's."""
import numpy as np
import pytest

import afsk_rescue_reference as ar
import afsk_rescue_scenes as sc
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu


def _repair(records):
    b = SondeBatch(1, sc.TILE)                              # any batch: the probe needs no flag and no AFSK channel
    got, status = b.test_afsk_repair(records)
    b.close()
    return got, status


def _same_as_twin(records):
    want, outcomes, _ = ar.rescue(records)
    got, status = _repair(records)
    want_status = np.array([ar.STATUS[oc] for oc in outcomes], dtype=np.int32)
    bad = np.nonzero(status != want_status)[0]
    assert len(bad) == 0, (int(bad[0]), int(status[bad[0]]), outcomes[bad[0]])
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), (k, outcomes[k])
    return got, status, outcomes


def test_every_pattern_in_every_byte_of_every_length():
    rec, orig, what = sc.exhaustive_records()
    got, status, outcomes = _same_as_twin(rec)
    assert len(rec) == 15 * (140 + 9)
    for k, (kind, ln, i, m) in enumerate(what):
        first = 2 if kind == "c50" else (3 if int(orig[k]["data"][1]) == 3 else 2)
        if kind == "imet":
            assert status[k] == (1 if i >= first else 0), (ln, i, m)
        if status[k] == 1 and i >= first:
            assert np.array_equal(got[k]["data"], orig[k]["data"]) and int(_lib.frame_flips(int(got[k]["flags"]))) == bin(m).count("1")
    c50 = np.array([w[0] == "c50" for w in what])
    assert (status[c50] == 1).sum() >= 60 and (status[c50] == 2).sum() >= 1


def test_records_that_are_not_eligible_stay():
    rec, orig, what = sc.exhaustive_records()
    pick = np.array([k for k, w in enumerate(what) if w[2] == w[1] - 3 and w[3] == 4])      # one damaged record per (kind, length)
    assert len(pick) == len(sc.EXHAUSTIVE)
    variants = []
    for field, value in (("nerr0", 0), ("nerr0", 1), ("type", 0), ("type", 3), ("type", 6), ("len", 4), ("len", 65), ("len", 528), ("len", 0), ("len", -1)):
        r = rec[pick].copy()
        if field == "nerr0":
            r["nerr"][:, 0] = value
        elif field == "len":
            r["len"] = value
        else:
            r["type"] = value
        variants.append(r)
    swapped = rec[pick].copy()                               # an iMet record marked C50 and the other way round
    swapped["type"] = np.where(swapped["type"] == sc.IMET4, sc.C50, sc.IMET4)
    variants.append(swapped)
    records = np.concatenate(variants)
    got, status = _repair(records)
    want, outcomes, _ = ar.rescue(records)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(status, np.array([ar.STATUS[oc] for oc in outcomes], dtype=np.int32))
    assert (status[:10 * len(pick)] == 0).all() and got[:10 * len(pick)].tobytes() == records[:10 * len(pick)].tobytes()


def test_random_damage_follows_the_twin():
    """1..4 random bit flips anywhere in random packets of every length: rescued, unsolved, and for C50 ambiguous and wrongly rescued
    records all occur, and the routine agrees with the twin on each"""
    from sdrpp_radiosonde_amd._lib import FRAME_DTYPE
    rng = np.random.default_rng(84)
    n_each = 60
    rec = np.zeros(n_each * len(sc.EXHAUSTIVE), dtype=FRAME_DTYPE)
    k = 0
    for kind, ln in sc.EXHAUSTIVE:
        for _ in range(n_each):
            pkt = sc.valid_packet(kind, ln, rng).copy()
            for _ in range(int(rng.integers(1, 5))):
                pkt[int(rng.integers(0, ln))] ^= 1 << int(rng.integers(0, 8))
            rec[k]["channel"], rec[k]["type"], rec[k]["len"], rec[k]["bitpos"] = k % 5, sc.KINDS[kind][0], ln, 77 + k
            rec[k]["nerr"][0] = -1
            rec[k]["data"][:ln] = pkt
            k += 1
    got, status, outcomes = _same_as_twin(rec)
    assert {"rescued", "unsolved", "ambiguous"} <= set(outcomes)
