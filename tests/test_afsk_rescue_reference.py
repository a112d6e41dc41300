"""The twin of SONDE_FLAG_AFSK_RESCUE (tests/afsk_rescue_reference.py, DESIGN SPEC 3.3i) against the definition, on the CPU: over the
oracle's records of the designed scenes every planned damage gives its planned outcome and every rescued packet is the transmitted
one; exhaustively, every pattern in every candidate byte of every packet length is repaired to the original and the same patterns in
the bytes the framer relied on are never repaired; iMet never yields `ambiguous`; mutations of the rule are told apart by the scenes;
and the noisy iMet scene rescues 150 packets or more, each of them a transmitted one."""
import collections

import numpy as np
import pytest

import afsk_rescue_reference as ar
import afsk_rescue_scenes as sc

KINDS = ["imet", "c50"]


def _planned(kind):
    s = sc.scene(kind)
    fr = sc.oracle_run(kind)
    out, outcomes, state = ar.rescue(fr)
    rows = []
    for f, r, oc in zip(fr, out, outcomes):
        hit = sc.tx_of(s, f)
        assert hit is not None, (int(f["channel"]), int(f["bitpos"]))
        rows.append((f, r, oc, s.plan[(int(f["channel"]), hit[0])], hit[1]))
    return s, rows, state


@pytest.mark.parametrize("kind", KINDS)
def test_every_planned_case_gives_its_planned_outcome(kind):
    s, rows, state = _planned(kind)
    seen = collections.Counter()
    for f, r, oc, case, tx in rows:
        want, flips = sc.EXPECT[kind][case]
        assert oc == want, (case, oc, int(f["channel"]), int(f["bitpos"]))
        seen[case] += 1
        if oc == "rescued":
            assert np.array_equal(r["data"][:len(tx)], tx) and not r["data"][len(tx):].any()
            assert int(r["nerr"][0]) == 0 and int(r["nerr"][1]) == 0
            assert int(r["flags"]) == (int(f["flags"]) | ar.FRAME_RESCUED | (flips << 8))
            for k in ("channel", "type", "len", "bitpos"):
                assert r[k] == f[k]
        else:
            assert r.tobytes() == f.tobytes()
    assert all(seen[c] >= 8 for c in sc.CASES), seen
    # the oracle recorded every damaged packet with exactly its damage: nearly every packet sent has a record (the last may be cut)
    assert len(rows) >= sum(len(x) for x in s.frames) - 2 * s.C
    for c in range(s.C):
        n_try = sum(1 for f, _, oc, _, _ in rows if int(f["channel"]) == c and oc not in ("clean", "other"))
        n_res = sum(1 for f, _, oc, _, _ in rows if int(f["channel"]) == c and oc == "rescued")
        assert state[c] == {"tried": n_try, "rescued": n_res}


def test_no_damage_goes_into_a_channels_first_packet():
    for kind in KINDS:
        s = sc.scene(kind)
        assert all(s.plan[(c, s.frames[c][0][0])] is None for c in range(s.C))


def test_clean_scene_has_nothing_to_rescue():
    for kind in KINDS:
        fr = sc.oracle_run(kind, True)
        out, outcomes, state = ar.rescue(fr)
        assert len(fr) >= 70 and set(outcomes) == {"clean"} and out.tobytes() == fr.tobytes() and state == {}


def test_exhaustive_every_pattern_in_a_candidate_byte_is_repaired_and_none_in_the_header():
    rec, orig, what = sc.exhaustive_records()
    out, outcomes, _ = ar.rescue(rec)
    n_fixed = n_header = 0
    for r, o, f, oc, (kind, ln, i, m) in zip(out, orig, rec, outcomes, what):
        first = 2 if kind == "c50" else (3 if int(o["data"][1]) == 3 else 2)
        if i < first:
            # SOH / sync, the type byte, XDATA's length byte: never touched, whatever else fits
            assert oc in ("unsolved", "ambiguous", "rescued"), (kind, ln, i, m, oc)
            assert np.array_equal(r["data"][:first], f["data"][:first])
            if kind == "imet":
                assert oc == "unsolved", (ln, i, m, oc)
                assert r.tobytes() == f.tobytes()
            n_header += 1
            continue
        if kind == "imet":
            assert oc == "rescued", (ln, i, m, oc)
        else:
            assert oc in ("rescued", "ambiguous"), (i, m, oc)       # C50: the true repair always fits; it may not be the only one
        if oc == "rescued":
            want = o.copy()
            want["flags"] = int(o["flags"]) | ar.FRAME_RESCUED | (bin(m).count("1") << 8)
            assert r.tobytes() == want.tobytes(), (kind, ln, i, m)
            n_fixed += 1
        else:
            assert r.tobytes() == f.tobytes()
    assert "ambiguous" not in [oc for oc, w in zip(outcomes, what) if w[0] == "imet"]
    assert n_header == 15 * (3 * 4 + 2 * 3 + 2) and n_fixed >= 15 * (140 - 18) + 60       # XDATA lengths 5, 6, 13, 64; C50: 105 less the ambiguous


def test_imet_patterns_have_distinct_syndromes_within_64_bytes():
    """the reason iMet is never ambiguous (SPEC 3.3i): over the longest record, the 930 candidate patterns change the check in 930 different
    ways -- computed here from the definition, one CRC per pattern"""
    ln = 64
    base = np.zeros((1, ln), dtype=np.uint8)
    rows = np.repeat(base, 15 * ln, axis=0)
    k = 0
    for i in range(ln):
        for m in sc.MASKS:
            rows[k, i] ^= m
            k += 1
    t = rows.astype(np.uint32)
    crc = np.full(len(t), 0x1D0F, dtype=np.uint32)
    for i in range(ln - 2):
        crc = ((crc << 8) & 0xFFFF) ^ ar._CRC_TAB[(crc >> 8) ^ t[:, i]]
    syn = crc ^ ((t[:, ln - 2] << 8) | t[:, ln - 1])
    assert len(set(int(v) for v in syn)) == 15 * ln


@pytest.mark.parametrize("mutation,kind", [("first_fit", "c50"), ("pairs", "imet"), ("pairs", "c50"), ("touch_header", "c50")])
def test_scenes_tell_mutations_of_the_rule_apart(mutation, kind):
    kw = {"first_fit": dict(first_fit=True), "pairs": dict(pairs=False), "touch_header": dict(touch_header=True)}[mutation]
    if mutation == "touch_header":
        rec = sc.exhaustive_records()[0]
        assert ar.rescue(rec, **kw)[0].tobytes() != ar.rescue(rec)[0].tobytes()
        return
    fr = sc.oracle_run(kind)
    assert ar.rescue(fr, **kw)[0].tobytes() != ar.rescue(fr)[0].tobytes()


def test_state_is_carried_and_not_shared():
    fr = sc.oracle_run("imet")
    _, _, s1 = ar.rescue(fr)
    _, _, s2 = ar.rescue(fr, s1)
    assert all(s2[c]["tried"] == 2 * s1[c]["tried"] and s2[c]["rescued"] == 2 * s1[c]["rescued"] for c in s1)
    half = len(fr) // 2
    _, _, a = ar.rescue(fr[:half])
    _, _, b = ar.rescue(fr[half:], a)
    assert b == s1


def test_noisy_imet_scene_rescues_150_or_more_and_every_one_was_sent():
    s = sc.noisy_scene("noisy_imet")
    fr = sc.oracle_run("noisy_imet")
    out, outcomes, _ = ar.rescue(fr)
    n = outcomes.count("rescued")
    print("noisy iMet scene: records", len(fr), "clean", outcomes.count("clean"), "rescued", n, "unsolved", outcomes.count("unsolved"))
    assert n >= 150 and "ambiguous" not in outcomes
    for f, oc in zip(out, outcomes):
        if oc == "rescued":
            hit = sc.tx_of(s, f)
            assert hit is not None and int(f["len"]) == len(hit[1]) and np.array_equal(f["data"][:len(hit[1])], hit[1])
