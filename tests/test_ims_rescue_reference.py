"""CPU: the twin of SONDE_FLAG_IMS_RESCUE (tests/ims_rescue_reference.py, DESIGN SPEC 3.3h).  Its restatement of the first pass
reproduces the CPU oracle's records from the oracle's chips; its block decoder against the brute-force definition on a few thousand
(block, mask) pairs; the uniqueness statement (every interior mask with m <= 4 on lone-chip damage decodes to the transmitted block)
and the ambiguous case at m = 5; the twin over the oracle's records and chips (Channel.bits()) on the designed scene of
tests/ims_rescue_scenes.py: every record gets the planned outcome, every rescued frame is the transmitted one, the result does not
depend on how the records are cut; the noisy scene gives the recorded counts; and the tests tell seven mutations of the rule from the
rule."""
import numpy as np
import pytest

import ims_rescue_reference as ir
import ims_rescue_scenes as ims


def _rem(v):
    """v mod 0x1539 bit by bit from the top: the tests' own division"""
    for i in range(63, 11, -1):
        if (v >> i) & 1:
            v ^= 0x1539 << (i - 12)
    return v


def _definition(blk, viol_mask):
    """SPEC step 3 as it is written"""
    V = [v for v in range(47) if (viol_mask >> v) & 1]
    if not 1 <= len(V) <= 6:
        return None
    patterns = set()
    for h in range(1 << len(V)):
        cells = [v - 1 + ((h >> j) & 1) for j, v in enumerate(V)]
        e = 0
        for c in cells:
            if 0 <= c <= 45:
                e ^= 1 << (45 - c)
        if _rem(blk ^ e) == 0:
            patterns.add(e)
    if len(patterns) != 1:
        return None
    e = patterns.pop()
    return blk ^ e, bin(e).count("1")


def test_code_and_first_pass_restated():
    """g divides x^63 + 1 and every encoded word; the distance within 46 bits is 5 (so `within distance 2` names one codeword)"""
    assert _rem(1 << 63 | 1) == 0 and bin(ir.G).count("1") % 2 == 1
    rng = np.random.default_rng(1)
    for _ in range(200):
        cw = ir.encode(int(rng.integers(0, 1 << 34)))
        assert _rem(cw) == 0 and ir.is_codeword(cw) and not ir.first_pass_rejects(cw)
        i, j, k = (int(x) for x in rng.choice(46, size=3, replace=False))
        assert ir.first_pass_block(cw ^ 1 << i) == (cw, 1) and ir.first_pass_block(cw ^ 1 << i ^ 1 << j) == (cw, 2)
        got, n = ir.first_pass_block(cw ^ 1 << i ^ 1 << j ^ 1 << k)
        assert got != cw and (n == -1 or (n == 2 and _rem(got) == 0))          # three wrong bits: rejected, or miscorrected to a neighbour


def test_first_pass_restatement_reproduces_the_oracles_records():
    """SPEC step 2: the blocks the twin's brute force rejects are the recorded nerr[1], and its corrections the recorded bytes"""
    for name in ("designed", "noisy"):
        fr, streams = ims.oracle_run(name)
        assert len(fr) >= 60
        for f in fr:
            c, p = int(f["channel"]), int(f["bitpos"])
            mine = ims.first_pass_record(streams[c], p, c)[0]
            assert mine.tobytes() == f.tobytes(), (name, c, p, f["nerr"], mine["nerr"])


def test_block_decoder_against_the_definition():
    blocks, viols, first_amb = ims.block_pairs()
    want_blk, want_st = ims.block_pairs_decoded()
    idx = np.concatenate([np.arange(0, first_amb, 5), np.arange(first_amb, len(blocks), 20)])
    assert len(idx) > 3000
    for i in idx.tolist():
        d = _definition(int(blocks[i]), int(viols[i]))
        assert (int(want_blk[i]), int(want_st[i])) == (d if d is not None else (int(blocks[i]), -1)), i
    assert (want_st >= 0).sum() >= 1000 and (want_st == -1).sum() >= 1000


def test_interior_masks_up_to_four_lone_chips_decode_to_the_transmitted_block():
    """the uniqueness statement: two hypotheses differ by (1 + x) q, q on the boundaries where they differ; both fit only if q is a
    codeword, weight >= 5.  So with m <= 4 interior violations the decode is unique, and right when every wrong chip is a lone one."""
    rng = np.random.default_rng(2)
    n = 0
    for k in (1, 2, 3, 4):
        for _ in range(250):
            cw = ir.encode(int(rng.integers(0, 1 << 34)))
            w = ims.window_of(cw, int(rng.integers(0, 2)), int(rng.integers(0, 2)))
            # window chip 1 + 2 b is the first chip of cell b (marks boundary b), 2 + 2 b the second (marks b + 1): interior marks 1..45
            chips = sorted(int(c) for c in rng.choice(np.arange(3, 91), size=k, replace=False))
            if any(b - a == 1 for a, b in zip(chips, chips[1:])):
                continue
            for c in chips:
                w[c] ^= 1
            blk, viol = ims.pair_of_window(w)
            V = [v for v in range(47) if (viol >> v) & 1]
            assert len(V) == k and 1 <= min(V) and max(V) <= 45
            assert ir.decode_block(blk, V) == (cw, k), (hex(cw), chips)
            n += 1
    assert n > 800


def test_ambiguous_case_at_five_violations():
    qs = ims.weight5_codewords()
    assert len(qs) >= 4
    for q in qs:
        assert _rem(q) == 0 and bin(q).count("1") == 5 and q.bit_length() <= 45
        cw = ir.encode(0x2A5A5A5A5 & ((1 << 34) - 1))
        blk, viol = ims.ambiguous_pair(q, cw)
        V = [v for v in range(47) if (viol >> v) & 1]
        assert len(V) == 5 and bin(blk ^ cw).count("1") == 5
        both = {blk ^ cw, blk ^ cw ^ q ^ (q << 1)}                               # all-left and all-right: both give a codeword
        assert len(both) == 2 and all(_rem(blk ^ e) == 0 for e in both)
        assert ir.decode_block(blk, V) is None and _definition(blk, viol) is None
        assert ir.decode_block(blk, V, first_fit=True) is not None               # MUTATION first fit: caught here
        # one violation fewer: unique again, and the transmitted block
        drop = V[0]
        assert ir.decode_block(blk ^ 1 << (45 - (drop - 1)), V[1:]) == (cw, 4)


def _twin(name, **mut):
    fr, streams = ims.oracle_run(name)
    return ir.rescue(fr, ir.chips_of_streams(streams), **mut)


def table_mismatches(**mut):
    """records of the designed scene whose outcome, block count or bytes are not what the table of cases says, under the (mutated) twin"""
    sc = ims.scene()
    fr, _ = ims.oracle_run("designed")
    out, outcomes, _ = _twin("designed", **mut)
    bad, seen = [], {}
    for f0, f, oc in zip(fr, out, outcomes):
        pos, tx = ims.tx_of(sc, f)
        case, flips = sc.plan[(int(f["channel"]), pos)]
        want, blocks, is_tx = ims.EXPECT[case]
        seen[case] = seen.get(case, 0) + 1
        ok = oc == want and ir.FRAME_RESCUED * (want == "rescued") == int(f["flags"]) & ir.FRAME_RESCUED and ((int(f["flags"]) >> 8) & 0xF) == blocks * (want == "rescued")
        ok = ok and np.array_equal(f["data"][:51], tx) == is_tx
        if want == "rescued":
            flipped = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(f["data"][:51], f0["data"][:51]))
            ok = ok and int(f["nerr"][1]) == 0 and int(f0["nerr"][1]) == blocks and int(f["nerr"][0]) >= int(f0["nerr"][0]) + flipped
            ok = ok and int(f["flags"]) == ir.FRAME_RESCUED | blocks << 8
        else:
            ok = ok and f.tobytes() == f0.tobytes()
        if want == "clean":
            ok = ok and int(f["nerr"][1]) == 0
        if not ok:
            bad.append((int(f["channel"]), pos, case, oc))
    return bad, seen


def test_every_case_of_the_table():
    sc = ims.scene()
    fr, streams = ims.oracle_run("designed")
    assert len(fr) == sum(len(v) for v in sc.frames) and set(fr["type"]) == {ims.IMS} and set(fr["len"]) == {51}
    bad, seen = table_mismatches()
    assert not bad, bad
    for case in ims.CASES:
        assert seen.get(case, 0) >= 3, (case, seen)
    # the bits flipped are the wrong chips' cells: nerr[0] of a rescued record counts them, parity bits included
    out, outcomes, state = _twin("designed")
    for f0, f, oc in zip(fr, out, outcomes):
        pos, _ = ims.tx_of(sc, f)
        case, flips = sc.plan[(int(f["channel"]), pos)]
        fc = streams[int(f["channel"])][int(f["bitpos"]):int(f["bitpos"]) + 1152]
        if case == "first_cell":         # the cases that stand for a boundary really use it
            assert (0, "a") in flips and 0 in ir.violations(fc, 0)
        if case == "last_cell":
            assert (551, "c") in flips
        if case == "neighbours":
            L = min(n for n, _ in flips) // 46
            assert 46 in ir.violations(fc, L) and 0 in ir.violations(fc, L + 1)
        if oc == "rescued":
            assert int(f["nerr"][0]) - int(f0["nerr"][0]) == sum(1 for _, kind in flips if kind in ("a", "c")), (case, flips)
        assert all(f[k] == f0[k] for k in ("channel", "type", "len", "bitpos"))
        assert np.array_equal(f["data"][51:], f0["data"][51:]) and not f["data"][51:].any()
    for c in range(sc.C):
        mine = [oc for f, oc in zip(fr, outcomes) if int(f["channel"]) == c]
        st = state.get(c, ir.new_state())
        assert st == {"tried": sum(oc in ("unsolved", "rescued") for oc in mine), "rescued": mine.count("rescued")}
        assert st["rescued"] >= 4


def test_no_chips_leaves_the_frame():
    fr, _ = ims.oracle_run("designed")
    out, outcomes, state = ir.rescue(fr, lambda c, s, n: None)
    assert out.tobytes() == fr.tobytes() and not state and "no_chips" in outcomes and "rescued" not in outcomes


def test_cut_invariance_of_the_twin():
    fr, streams = ims.oracle_run("designed")
    get = ir.chips_of_streams(streams)
    whole, oc_whole, st_whole = ir.rescue(fr, get)
    order = np.lexsort((fr["channel"], fr["bitpos"]))              # time order: what successive submits deliver
    parts, state = [], {}
    for piece in np.array_split(order, 3):
        out, _, state = ir.rescue(fr[np.sort(piece)], get, state)
        parts.append(out)
    got = np.concatenate(parts)
    got = got[np.lexsort((got["bitpos"], got["channel"]))]
    assert got.tobytes() == whole.tobytes() and state == st_whole


def test_noisy_scene_gives_the_recorded_counts():
    sc = ims.scene_of("noisy")
    fr, streams = ims.oracle_run("noisy")
    out, outcomes, _ = ir.rescue(fr, ir.chips_of_streams(streams))
    failed = fr[fr["nerr"][:, 1] != 0]
    n_res = equal = 0
    for f, oc in zip(out, outcomes):
        if oc != "rescued":
            continue
        n_res += 1
        hit = ims.tx_of(sc, f)
        equal += hit is not None and np.array_equal(f["data"][:51], hit[1])
    got = dict(records=len(fr), failed=len(failed), by_blocks=np.bincount(failed["nerr"][:, 1]).tolist(), rescued=n_res, rescued_equal_tx=equal)
    print("noisy", got, "outcomes", {oc: outcomes.count(oc) for oc in set(outcomes)})
    assert got == ims.NOISY_COUNTS and got["failed"] >= 10
    assert "mismatch" not in outcomes and "no_chips" not in outcomes


def test_a_record_that_disagrees_with_the_ring_stays():
    """SPEC step 2: |F| recomputed from the chips must be the recorded nerr[1]; MUTATION no such check: caught here"""
    fr, streams = ims.oracle_run("designed")
    get = ir.chips_of_streams(streams)
    _, outcomes, _ = ir.rescue(fr, get)
    i = outcomes.index("rescued")
    rec = fr[i:i + 1].copy()
    rec["nerr"][0, 1] += 1
    out, oc, state = ir.rescue(rec, get)
    assert oc == ["mismatch"] and out.tobytes() == rec.tobytes() and not state
    out, oc, _ = ir.rescue(rec, get, check_count=False)
    assert oc == ["rescued"] and out.tobytes() != rec.tobytes()
    # the chips of another frame under the record: the blocks found there are not the recorded ones
    other = fr[outcomes.index("clean")]
    shifted = lambda c, s, n: get(int(other["channel"]), int(other["bitpos"]), n)      # noqa: E731
    out, oc, _ = ir.rescue(fr[i:i + 1], shifted)
    assert oc == ["mismatch"] and out.tobytes() == fr[i:i + 1].tobytes()


MUTATIONS = {"cap_7": dict(cap=7), "next_chip": dict(use_next_chip=True), "no_cancel": dict(cancel=False), "stride_32": dict(data_stride=32),
             "cap_4": dict(cap=4)}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_scene_rejects_a_mutated_rule(name):
    """five mutations the designed scene catches; `first fit` and `no count check` are caught by the two tests above"""
    bad = table_mismatches(**MUTATIONS[name])[0]
    assert bad, name
    must = {"cap_7": {"seven"}, "next_chip": {"last_cell"}, "no_cancel": {"ac_three"}, "stride_32": {"three", "two_blocks"}, "cap_4": {"six", "ac_three"}}[name]
    assert must <= {b[2] for b in bad}, (name, sorted({str(b[2]) for b in bad}))
    if name == "stride_32":                  # block 0 is the one the mutation leaves right
        sc = ims.scene()
        for c, pos, case, oc in bad:
            assert any(n >= 46 for n, _ in sc.plan[(c, pos)][1])
