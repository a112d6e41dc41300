"""The decoder behind the wideband filter bank (SPEC 3.5b + 3.2 on a bin's phases: oracle/or_chan.c + or_dsp.c here, sd_bins_kernel in
test_gpu_bins_reference.py) against float64 references written from DESIGN.md alone.
  (a) the composite resampler + decimator of SPEC 3.5b: the oracle's decimated rows against fe_reference.composite_rows ("resample,
      then average" from the closed-form taps), within a bound that is a formula, over 8 blocks and both stackings;
  (b) the block replay (demod_reference.replay with hidden states) is sound: narrowband pre-decimated scenes fed tile by tile, two of
      every three and five of every six states hidden: the replay accepts, and every state the oracle really had lies in the carried set;
  (c) it still has teeth: every mutation of demod_reference.MUTATIONS that acts on this path is rejected with two of three states hidden;
  (d) end to end: the wideband scene through the oracle's channels, one block per feed, replayed from the phases alone.
A bin's smallest submit is one block = 3 tiles, so (b) is what lets (d) and the GPU half stand without bit-exactness to anything."""
from __future__ import annotations

import numpy as np
import pytest

import bins_scenes as B
import demod_reference as D
import fe_reference as F
from test_demod_reference import AMB_LIMIT, DEC_SCENES, observed, reference_disc, scene_modem

ODD_WATCH = [(k, ty, e) for k, _, ty, e in B.ODD_TX]
_cache: dict = {}


def oracle_bank(oracle, odd: bool, watch, all_rs41: bool = False, late: bool = False):
    """the scene (late: bins_scenes.late_scene) through or_chan_block2 (one bank) and one oracle channel per watched bin, one block
    per feed: {bin: (q [NBLK * 2560] int64, rows [NBLK * 1536] float32, states per block, bits per block)}"""
    key = (odd, all_rs41, late)
    if key in _cache:
        return _cache[key]
    L = oracle.lib()
    x = B.late_scene() if late else B.scene()
    ch = L.or_chan_new_odd() if odd else L.or_chan_new()
    n_out = B.STEPS * 12 // 5
    decs = np.zeros(512, np.uint8)
    dec = {}
    for k, ty, _ in watch:
        decs[k] = 4
        dec[k] = oracle.Channel(0 if all_rs41 else ty, k)
    bins = np.zeros((512, B.STEPS), np.float32)
    out48 = np.zeros((512, n_out), np.float32)
    outdec = np.zeros((512, n_out // 2), np.float32)
    res = {k: ([], [], [], []) for k in dec}
    nb = {k: 0 for k in dec}
    for b in range(x.shape[0] // B.BLOCK):
        blk = np.ascontiguousarray(x[b * B.BLOCK:(b + 1) * B.BLOCK]).reshape(-1)
        L.or_chan_block2(ch, oracle.fptr(blk), B.STEPS, oracle.fptr(bins.reshape(-1)), oracle.fptr(out48.reshape(-1)), decs.ctypes.data,
                         oracle.fptr(outdec.reshape(-1)))
        for k, c in dec.items():
            row = outdec[k, :n_out // 4].copy()
            c.feed_decimated(row, 4)
            dm = L.or_channel_demod(c.h)
            n = int(L.or_demod_nbits(dm))
            out = np.zeros(n - nb[k], np.uint8)
            if n > nb[k]:
                L.or_demod_getbits(dm, nb[k], n - nb[k], oracle.u8ptr(out))
            nb[k] = n
            q, rows, states, bits = res[k]
            q.append(B.to_q16(bins[k]))
            rows.append(row)
            states.append(c.state())
            bits.append(out)
    L.or_chan_free(ch)
    _cache[key] = {k: (np.concatenate(q), np.concatenate(rows), st, bt) for k, (q, rows, st, bt) in res.items()}
    return _cache[key]


# ---------------------------------------------------------------- (a) SPEC 3.5b
def test_oracle_composite_rows_match_resample_then_average(oracle):
    """every watched bin of both banks, 8 blocks (7 block edges): |row - z| <= bound, sample by sample"""
    worst, n = 0.0, 0
    for odd, watch in ((False, B.watched_even()), (True, ODD_WATCH)):
        for k, (q, rows, _, _) in oracle_bank(oracle, odd, watch).items():
            z, bound = F.composite_rows(q)
            assert z.shape == rows.shape == (B.NBLK * F.DEC_PER_BLOCK,)
            frac = np.abs(rows.astype(np.float64) - z) / np.maximum(bound, 1e-300)
            frac[(rows == z) & (bound == 0)] = 0.0
            worst = max(worst, float(frac.max()))
            n += z.shape[0]
            assert frac.max() <= 1.0, (odd, k, int(frac.argmax()), float(frac.max()))
    print(f"FE-REF composite oracle: bins={len(B.watched_even()) + len(ODD_WATCH)} samples={n} worst={worst:.3g} of the bound")
    assert n >= 4 * F.DEC_PER_BLOCK


def test_scene_has_its_edges(oracle):
    """what the scene exists for is in it: a carrier 4.5 kHz below the centre puts d at -0.9 quadrant, and noise carries it across -2
    (it comes out beyond +1); a silent bin's d is anywhere; a centred carrier at 20 dB stays within +-1.5"""
    bank = oracle_bank(oracle, False, B.watched_even())
    d = {k: F.chan_disc(bank[k][0][None, :])[0] for k in bank}
    across = {k: int((v > 1.0).sum()) for k, v in d.items()}
    print("FE-REF composite scene: samples of d beyond +1 quadrant per bin", across)
    assert across[64] > 0 and across[400] > 0 and min(across[65], across[67]) > 1000
    assert np.abs(d[66][64:]).max() < 1.5 and np.abs(d[200][64:]).max() < 1.5       # (behind the bank's start-up)
    assert abs(np.median(d[70]) + 0.9) < 0.1 and abs(np.median(d[130]) - 0.4) < 0.1
    # every bin type at 10 and at 20 dB, and the three carrier offsets
    assert {(ty, e) for _, _, ty, e in B.EVEN_TX} == {(ty, e) for ty in (B.RS41, B.DFM, B.IMS, B.MRZ) for e in (10.0, 20.0)}
    assert {df for _, df, _, _ in B.EVEN_TX} == {0.0, 2000.0, -4500.0}
    assert len({B.bin_types()[k] for k in range(64, 72)}) == 4


@pytest.mark.parametrize("name", sorted(F.COMPOSITE_MUTATIONS))
def test_composite_mutation_is_rejected(oracle, name):
    why = None
    for k, (q, rows, _, _) in oracle_bank(oracle, False, B.watched_even()).items():
        z, bound = F.composite_rows(q, **F.COMPOSITE_MUTATIONS[name])
        bad = np.abs(rows.astype(np.float64) - z) > bound
        if bad.any():
            why = f"bin {k}: {int(bad.sum())} of {bad.shape[0]} samples outside the bound"
            break
    print(f"FE-REF composite mutation {name}: rejected by {why}")
    assert why is not None, name


# ---------------------------------------------------------------- (b) the block replay is sound
def _spans(bits: list, every: int) -> list:
    return [np.concatenate(bits[i:i + every]) for i in range(0, len(bits), every)]


def hidden_check(oracle, s, every: int, truth: bool = True, **mut) -> D.Check:
    x, states, bits = observed(oracle, s)
    d, bd = reference_disc(s, x, None, **mut)
    return D.replay(d, bd, scene_modem(s), B.hide(states, every), _spans(bits, every), afc=False, truth=states if truth else None, **mut)


@pytest.mark.parametrize("every", [3, 6])
@pytest.mark.parametrize("s", DEC_SCENES, ids=[s.name for s in DEC_SCENES])
def test_block_replay_accepts_and_carries_the_true_states(oracle, s, every):
    """the oracle fed tile by tile, then two of three (five of six) states hidden: accepted, every hidden state the oracle really had
    is in the carried set, and the unresolved spans stay under the cap of the wideband tests"""
    chk = hidden_check(oracle, s, every)
    print(chk.line(f"{s.name}/1-of-{every}") + f" hidden={chk.hidden} outside={chk.outside}")
    assert not chk.failures(), (s.name, chk.failures())
    assert chk.outside == 0 and chk.hidden > 0
    assert chk.spans == s.ntiles // every and 4 * chk.unresolved <= chk.spans
    if s.ebn0 >= 10.0:
        assert chk.amb <= AMB_LIMIT * chk.nbits


# ---------------------------------------------------------------- (c) it still has teeth
# not applicable to a bin's path (real, pre-decimated input; no AFC, no boxcar in front, no tone front-end):
NOT_APPLICABLE = {
    "afc_lag_2": "AFC (SPEC 3.0b): IQ input only", "afc_gain_quarter": "AFC", "afc_leak_64": "AFC",
    "shift_30e_flipped": "SPEC 3.0e acts with the AFC only", "shift_30e_missing": "SPEC 3.0e",
    "box_plus_u": "the boxcar's rotation (SPEC 3.0d): IQ input only", "box_front_current_u": "SPEC 3.0d",
    "imet_mixer_1800": "AFSK tone front-end (SPEC 3.6)", "boxcar_4_blocks": "AFSK", "jump_16_16": "AFSK (SPEC 3.6b)",
    "group_shifted": "the decimation groups: the rows arrive decimated (fe_reference.COMPOSITE_MUTATIONS has the bin's own)",
}
APPLICABLE = sorted(set(D.MUTATIONS) - set(NOT_APPLICABLE))


@pytest.mark.parametrize("name", APPLICABLE)
def test_block_replay_rejects_mutation(oracle, name):
    why = None
    for s in DEC_SCENES:
        chk = hidden_check(oracle, s, 3, truth=False, **D.MUTATIONS[name])
        if chk.failures():
            why = f"{s.name}: {chk.failures()}"
            break
    print(f"DEMOD-REF block mutation {name}: rejected by {why}")
    assert why is not None, name


def test_mutation_lists_cover_every_entry():
    assert set(NOT_APPLICABLE) <= set(D.MUTATIONS) and len(APPLICABLE) == len(D.MUTATIONS) - len(NOT_APPLICABLE) == 13


# ---------------------------------------------------------------- (d) end to end on the oracle
def wideband_checks(bank: dict, watch, every_blocks: int, all_rs41: bool = False):
    chks = []
    for k, ty, _ in watch:
        q, _, states, bits = bank[k]
        chks.append((f"bin{k}", B.replay_bin(q, 0 if all_rs41 else ty, states[every_blocks - 1::every_blocks], _spans(bits, every_blocks),
                                            B.TILES_PER_BLOCK * every_blocks)))
    return chks


@pytest.mark.parametrize("case", ["even-3", "even-6", "odd-3", "rs41-3"])
def test_oracle_wideband_block_replay(oracle, case):
    """the scene of (a) through the oracle's channels, one block per feed, replayed from the phases alone (d, bd = composite_rows),
    observed every 3 tiles (every 6: every other block's state dropped).  These are the scenes and the cases of the GPU half; the
    unresolved cap (bins_scenes.summarise) holds for the oracle on exactly them.
    Observed (oracle): even-3 0 of 96 spans unresolved, even-6 0 of 48, odd-3 0 of 16, rs41-3 0 of 48."""
    bank, every = case.split("-")
    if bank == "odd":
        watch, res = ODD_WATCH, oracle_bank(oracle, True, ODD_WATCH)
    elif bank == "rs41":
        watch = B.watched_even()[::2]
        res = oracle_bank(oracle, False, B.watched_even(), all_rs41=True)
    else:
        watch, res = B.watched_even(), oracle_bank(oracle, False, B.watched_even())
    chks = wideband_checks(res, watch, int(every) // 3, all_rs41=bank == "rs41")
    print(B.summarise(f"oracle {case}", chks, [e for _, _, e in watch], AMB_LIMIT))


def test_late_carrier_takes_the_one_sided_round(oracle):
    """bins_scenes.late_scene through the oracle, one block per feed: the replay accepts both spans, and the scene holds what it was made
    for: block 2's first tile (about 205 symbols, behind the three tiles of the acquisition) is sliced to one value throughout -- a
    one-sided round of SPEC 3.2 -- and the tiles after it, with the threshold at that round's mean, see both levels again."""
    k, _, ty, e = B.LATE_TX
    res = oracle_bank(oracle, False, [(k, ty, e)], late=True)
    print(B.summarise("oracle late-3", wideband_checks(res, [(k, ty, e)], 1), [e], AMB_LIMIT))
    _, _, states, bits = res[k]
    print("late carrier: bits per block", [len(b) for b in bits], "ones among block 2's first 190 bits:", int(bits[1][:190].sum()),
          "share of ones behind them: %.3f" % bits[1][230:].mean())
    assert len(bits) == B.LATE_NBLK
    assert len(set(bits[1][:190].tolist())) == 1 and 0.25 < bits[1][230:].mean() < 0.75
