"""CPU: the twin of SONDE_FLAG_DFM_RESCUE (tests/dfm_rescue_reference.py, DESIGN SPEC 3.3g).  Its word decoder against the brute-force
definition on all 256 words x 256 erasure masks; the twin over the CPU oracle's records and chips (Channel.bits()) on the designed
scenes of tests/dfm_rescue_scenes.py: every record gets the planned outcome, every rescued frame is the transmitted one, |F| is the
recorded nerr[1], the result does not depend on how the records are cut; a noisy scene gains frames and none of them is wrong; and
the scenes tell six mutations of the rule from the rule."""
import numpy as np
import pytest

import dfm_rescue_reference as dr
import dfm_rescue_scenes as ds


def _parity_ok(w):
    return all(bin(w & row).count("1") % 2 == 0 for row in (0x78, 0xB4, 0xD2, 0xE1))


def test_word_decoder_against_the_definition():
    """SPEC step 4 as it is written: among the bytes that pass all four parity checks, those that differ from the word in v positions
    outside E with 2 v + e <= 3; none when e = 0 or e > 3; never more than one"""
    code = [w for w in range(256) if _parity_ok(w)]
    assert len(code) == 16 and sorted(code) == sorted(dr.CODEWORDS)
    assert min(bin(a ^ b).count("1") for a in code for b in code if a != b) == 4
    n_dec = 0
    for word in range(256):
        for E in range(256):
            e = bin(E).count("1")
            fits = [c for c in code if 1 <= e <= 3 and 2 * bin((c ^ word) & ~E & 0xFF).count("1") + e <= 3]
            assert len(fits) <= 1
            assert dr.decode_word(word, E) == (fits[0] if fits else None), (word, E)
            n_dec += len(fits)
    assert n_dec > 0
    # the guarantee: a codeword with up to 3 marked wrong bits, or 1 marked bit (wrong or not) and 1 unmarked wrong bit, comes back
    for c in code:
        for E in range(1, 256):
            e = bin(E).count("1")
            if e > 3:
                continue
            for sub in range(256):
                if sub & ~E:
                    continue
                assert dr.decode_word(c ^ sub, E) == c
                if e == 1:
                    for j in range(8):
                        if not (0x80 >> j) & E:
                            assert dr.decode_word(c ^ sub ^ (0x80 >> j), E) == c


def _twin(name, **mut):
    fr, streams = ds.oracle_run(name)
    return dr.rescue(fr, dr.chips_of_streams(streams), **mut)


def table_mismatches(name, **mut):
    """records of the scene whose outcome, word count or bytes are not what the table of cases says, under the (mutated) twin"""
    sc = ds.scene(name)
    fr, _ = ds.oracle_run(name)
    out, outcomes, _ = _twin(name, **mut)
    bad, seen = [], {}
    for f0, f, oc in zip(fr, out, outcomes):
        pos, tx = ds.tx_of(sc, f)
        case, blk = sc.plan[(int(f["channel"]), pos)]
        want, words, is_tx = ds.EXPECT[case]
        seen[(case, blk)] = seen.get((case, blk), 0) + 1
        ok = oc == want and dr.FRAME_RESCUED * (want == "rescued") == int(f["flags"]) & dr.FRAME_RESCUED and ((int(f["flags"]) >> 8) & 0xF) == words
        ok = ok and np.array_equal(f["data"][:33], tx) == is_tx
        if want == "rescued":
            ok = ok and int(f["nerr"][1]) == 0 and int(f["nerr"][0]) == int(f0["nerr"][0]) + words and int(f0["nerr"][1]) == words
        else:
            ok = ok and f.tobytes() == f0.tobytes()
        if want == "clean":
            ok = ok and int(f["nerr"][1]) == 0
        if not ok:
            bad.append((int(f["channel"]), pos, case, blk, oc))
    return bad, seen


def test_every_case_of_the_table():
    sc = ds.scene()
    fr, streams = ds.oracle_run("designed")
    assert len(fr) == sum(len(v) for v in sc.frames) and set(fr["type"]) == {ds.DFM} and set(fr["len"]) == {33}
    bad, seen = table_mismatches("designed")
    assert not bad, bad
    for case in ds.CASES:
        for blk in range(3) if case else [0]:
            assert seen.get((case, blk), 0) >= 1, (case, blk, seen)
    # the channel with Q negated carries inverted polarity on every record, the others on none
    for c in range(sc.C):
        assert set(fr["flags"][fr["channel"] == c] & 1) == {int(c in sc.inverted)}
    # |F| is the recorded nerr[1] (SPEC step 2), and only the named fields of a rescued record change
    out, outcomes, state = _twin("designed")
    for f0, f, oc in zip(fr, out, outcomes):
        assert sum(any(dr.syndrome(w)) for w in f0["data"][:33]) == int(f0["nerr"][1])
        assert all(f[k] == f0[k] for k in ("channel", "type", "len", "bitpos")) and (f["flags"] ^ f0["flags"]) & 1 == 0
        assert np.array_equal(f["data"][33:], f0["data"][33:]) and not f["data"][33:].any()
        changed = [i for i in range(33) if f["data"][i] != f0["data"][i]]
        assert all(any(dr.syndrome(f0["data"][i])) for i in changed)
    for c in range(sc.C):
        mine = [oc for f, oc in zip(fr, outcomes) if int(f["channel"]) == c]
        st = state.get(c, dr.new_state())
        assert st == {"tried": sum(oc in ("unsolved", "rescued") for oc in mine), "rescued": mine.count("rescued")}
        assert st["rescued"] >= 4


def test_long_scene_has_work_behind_record_64():
    fr, _ = ds.oracle_run("long")
    assert len(fr) > 70
    bad, seen = table_mismatches("long")
    assert not bad, bad
    _, outcomes, _ = _twin("long")
    assert set(outcomes[:60]) == {"clean"} and outcomes[60:71] == ["rescued", "unsolved"] * 5 + ["rescued"] and set(outcomes[71:]) == {"clean"}


def test_no_chips_leaves_the_frame():
    fr, _ = ds.oracle_run("designed")
    out, outcomes, state = dr.rescue(fr, lambda c, s, n: None)
    assert out.tobytes() == fr.tobytes() and not state and "no_chips" in outcomes and "rescued" not in outcomes and "too_many" in outcomes


@pytest.mark.parametrize("name", ["designed", "long"])
def test_cut_invariance_of_the_twin(name):
    fr, streams = ds.oracle_run(name)
    get = dr.chips_of_streams(streams)
    whole, oc_whole, st_whole = dr.rescue(fr, get)
    order = np.lexsort((fr["channel"], fr["bitpos"]))              # time order: what successive submits deliver
    parts, state = [], {}
    for piece in np.array_split(order, 3):
        out, _, state = dr.rescue(fr[np.sort(piece)], get, state)
        parts.append(out)
    got = np.concatenate(parts)
    got = got[np.lexsort((got["bitpos"], got["channel"]))]
    assert got.tobytes() == whole.tobytes() and state == st_whole


@pytest.mark.parametrize("name", ["noisy", "noisy_negq"])
def test_noisy_scene_gains_frames_and_none_is_wrong(name):
    sc = ds.scene_of(name)
    fr, streams = ds.oracle_run(name)
    out, outcomes, _ = dr.rescue(fr, dr.chips_of_streams(streams))
    failed = fr[fr["nerr"][:, 1] != 0]
    n_res = wrong = 0
    for f, oc in zip(out, outcomes):
        if oc != "rescued":
            continue
        n_res += 1
        hit = ds.tx_of(sc, f)
        wrong += hit is None or not np.array_equal(f["data"][:33], hit[1])
    print(name, "records", len(fr), "valid", int((fr["nerr"][:, 1] == 0).sum()), "failed", len(failed),
          "by failed words", np.bincount(failed["nerr"][:, 1]).tolist(), "rescued", n_res, "wrong", wrong)
    assert set(int(f["flags"]) & 1 for f in fr) == {int(name == "noisy_negq")}
    assert len(failed) == 22 and np.bincount(failed["nerr"][:, 1]).tolist() == [0, 20, 2]
    assert n_res == 22 and wrong == 0


MUTATIONS = {"bound_4": dict(bound=4), "partial_write": dict(partial_write=True), "second_chip": dict(second_chip=True),
             "stride_of_block0": dict(stride_of_block0=True), "cap_off": dict(cap=None), "reopen_corrected": dict(reopen_corrected=True)}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_scenes_reject_a_mutated_rule(name):
    bad = table_mismatches("designed", **MUTATIONS[name])[0]
    assert bad, name
    # and each where it must
    must = {"bound_4": {"a_c_ac"}, "partial_write": {"one_bad_of_two"}, "cap_off": {"nine"}, "reopen_corrected": {"aaa", "a"},
            "stride_of_block0": {"aa"}, "second_chip": {"aa"}}[name]
    assert must <= {b[2] for b in bad}, (name, sorted({str(b[2]) for b in bad}))
    if name == "stride_of_block0":           # block 0 is the one the mutation leaves right
        assert all(b[3] != 0 for b in bad if b[2] == "aa") and {b[3] for b in bad if b[2] == "aa"} == {1, 2}
