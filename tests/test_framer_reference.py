"""The CPU oracle's stage 3 (oracle/or_framers.c for the six non-RS41 sonde types, oracle/or_fec.c for RS41) against the independent
reference of tests/framer_reference.py: unit by unit (BCH against the remainder table, Hamming on all 256 words in all 33 lanes, the checksums),
on every designed stream of tests/framer_streams.py and on noisy mixed scenes; the plan of every designed stream holds on the oracle's
records and every decision path it was built for is counted; and every mutation of the reference is rejected by at least one designed
stream, so the streams can see those bugs in a kernel (tests/test_gpu_framer_reference.py runs the same streams through the GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import framer_reference as R
import framer_streams as S
import oracle_lib
from sdrpp_radiosonde_amd import synth

_CACHE = {}


def decoded(name: str):
    """(Designed, [bits per channel], [records per channel]) of a designed stream through the oracle, built once per session"""
    if name not in _CACHE:
        d = (S.rs41_streams() if name in S.rs41_streams() else S.all_streams())[name]()
        x = d.iq.numpy()
        bits, recs = [], []
        for c in range(x.shape[0]):
            ch = oracle_lib.Channel(d.stype, c)
            ch.feed(x[c])
            bits.append(ch.bits())
            recs.append(ch.frames())
        d.iq = None                                                      # the IQ is the bulk of it and is not needed again
        _CACHE[name] = (d, bits, recs)
    return _CACHE[name]


STREAMS = sorted(S.all_streams())
RS41_STREAMS = sorted(S.rs41_streams())          # a list of their own: what the tests below select from STREAMS stays as it was


# ------------------------------------------------------------------------------------------------ units
def _lib():
    L = oracle_lib.lib()
    L.or_bch_decode.restype = C.c_uint64
    L.or_bch_decode.argtypes = [C.c_uint64, C.POINTER(C.c_int)]
    L.or_m10_checksum.restype = C.c_uint16
    L.or_m10_checksum.argtypes = [C.POINTER(C.c_uint8), C.c_size_t]
    L.or_crc16_modbus.restype = C.c_uint16
    L.or_crc16_modbus.argtypes = [C.POINTER(C.c_uint8), C.c_size_t]
    return L


def test_bch_table_is_complete():
    """the 63 + 1953 remainders are distinct and non-zero (asserted at import); every codeword divides"""
    for v in (0, 1, 0x3FFFFFFFF, 0x2AAAAAAAA, 0x123456789):
        assert R.poly_mod((v << 12) | synth.bch_parity(v)) == 0


def test_oracle_bch_against_the_remainder_table(oracle):
    L = _lib()
    rng = np.random.default_rng(1)
    st = C.c_int()
    n = 0
    for v in [0, 0x3FFFFFFFF] + [int(x) for x in rng.integers(0, 1 << 34, size=6)]:
        cw = (v << 12) | synth.bch_parity(v)
        pats = S.ims_patterns()
        pats += [tuple(int(p) for p in rng.choice(46, size=w, replace=False)) for w in (3, 4, 5, 6) for _ in range(400)]
        for pat in pats:
            blk = cw
            for p in pat:
                blk ^= 1 << p
            got = L.or_bch_decode(blk, C.byref(st))
            want, wst = R.bch_decide(blk)
            assert (got, st.value) == (want, wst), (hex(cw), pat)
            if len(pat) <= 2:
                assert (want, wst) == (cw, len(pat)), (hex(cw), pat)
            n += 1
    print(f"FRAMER-REF bch: {n} words, oracle == remainder table")


def test_hamming_codebook_is_the_generators():
    assert sorted(R.HAMMING_CODEBOOK) == sorted(int(x) for x in synth.hamming84_encode(np.arange(16)))
    st = [R.HAMMING_TABLE[w][1] for w in range(256)]
    assert (st.count(0), st.count(1), st.count(-1)) == (16, 128, 112)


def test_oracle_checksums_against_the_reference(oracle):
    L = _lib()
    rng = np.random.default_rng(2)
    msgs = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in (1, 2, 12, 16, 43, 68, 99) for _ in range(8)]
    for n in (43, 68, 99):                                               # every single-bit message of the frame lengths
        for i in range(8 * n):
            m = np.zeros(n, dtype=np.uint8)
            m[i // 8] = 1 << (i % 8)
            msgs.append(m)
    for m in msgs:
        assert L.or_m10_checksum(oracle_lib.u8ptr(m), len(m)) == R.m10_checksum(m), m
        assert L.or_crc16_modbus(oracle_lib.u8ptr(m), len(m)) == R.crc16_reflected(m), m
        assert L.or_imet_crc(oracle_lib.u8ptr(m), len(m)) == R.binascii.crc_hqx(m.tobytes(), 0x1D0F), m
        assert int(synth.m10_checksum(m[None, :], n=len(m))[0]) == R.m10_checksum(m)
    print(f"FRAMER-REF checksums: {len(msgs)} messages x 3 checks")


# ------------------------------------------------------------------------------------------------ designed streams
@pytest.mark.parametrize("name", STREAMS)
def test_designed_stream(oracle, name):
    """the section-2 conditions (the demodulator returns the planted chips), reference == oracle byte for byte, the plan holds"""
    d, bits, recs = decoded(name)
    cover, nrec = {}, 0
    for c in range(len(bits)):
        off, pol = S.check_conditions(d, c, bits[c])
        ref = R.reference(d.stype, bits[c], c)
        assert len(ref) == len(recs[c]) and ref.tobytes() == recs[c].tobytes(), (name, c)
        S.check_plan(d, c, ref, off, pol, cover)
        nrec += len(ref)
    print(f"FRAMER-REF stream {name}: {len(bits)} channels, {nrec} records, {sum(len(p) for p in d.plan)} planned cases")


WIDE_DECIM = {S.IMS: (2, 4), S.M10: (1, 2), S.MRZ: (2, 4)}              # type -> (decimation under SONDE_FLAG_WIDE_AUTO: one step less, the default decimation)


@pytest.mark.parametrize("name", [n for n in STREAMS if n.split("-")[0] in ("ims", "m10", "m20", "mrz") or n[:6] in ("sync-2", "sync-3", "sync-6")])
def test_designed_stream_behind_the_wide_modem(oracle, name):
    """the conditions hold behind the other modem class too (the GPU test runs these streams under SONDE_FLAG_WIDE_AUTO)"""
    d = S.all_streams()[name]()
    L = oracle_lib.lib()
    L.or_modem_set_decim(d.stype, WIDE_DECIM[d.stype][0])          # (the setting is read while a channel runs: held until all are done)
    try:
        x = d.iq.numpy()
        for c in range(x.shape[0]):
            ch = oracle_lib.Channel(d.stype, c)
            ch.feed(x[c])
            bits = ch.bits()
            off, pol = S.check_conditions(d, c, bits)
            ref = R.reference(d.stype, bits, c)
            assert ref.tobytes() == ch.frames().tobytes(), (name, c)
            S.check_plan(d, c, ref, off, pol, {})
            del ch
    finally:
        L.or_modem_set_decim(d.stype, WIDE_DECIM[d.stype][1])


def test_designed_streams_cover_every_path(oracle):
    cover = {}
    pending = 0
    for name in STREAMS:
        d, bits, recs = decoded(name)
        for c in range(len(bits)):
            off, pol = S.align(d, c, bits[c])
            S.check_plan(d, c, recs[c], off, pol, cover)
            info = {}
            R.reference(d.stype, bits[c], c, info=info)
            pending += "pending" in info
            for why in info.get("drops", ()):
                cover[(d.stype, "drop", why)] = 1
    missing = [k for k in S.required_coverage(STREAMS) + S.required_drops() if k not in cover]
    assert not missing, (len(missing), missing[:10])
    assert pending > 0                   # a sync whose frame the end of the stream cuts: no record
    print(f"FRAMER-REF coverage: {len(cover)} keys, none of the {len(S.required_coverage(STREAMS))} required ones missing; "
          f"{pending} channels end inside a frame")


# ------------------------------------------------------------------------------------------------ RS41: designed streams
@pytest.mark.parametrize("name", RS41_STREAMS)
def test_rs41_designed_stream(oracle, name):
    """the conditions (the demodulator returns the planted bits of every planted frame and decoy), reference == oracle byte for byte,
    the plan holds: every planted header is a case, only each channel's first frame is nobody's"""
    d, bits, recs = decoded(name)
    cover, nrec = {}, 0
    for c in range(len(bits)):
        assert d.plan[c], (name, c, "a channel without cases")
        off, pol = S.check_conditions(d, c, bits[c])
        ref = R.reference(R.RS41, bits[c], c)
        assert len(ref) == len(recs[c]) and ref.tobytes() == recs[c].tobytes(), (name, c)
        S.check_plan(d, c, ref, off, pol, cover)
        assert name != "rs41-order" or len(ref) == 11, (name, c, len(ref))      # the first frame too: the cases are the 2nd .. 11th of the stream
        nrec += len(ref)
    print(f"FRAMER-REF stream {name}: {len(bits)} channels, {nrec} records, {sum(len(p) for p in d.plan)} planned cases")


def test_rs41_designed_streams_cover_every_path(oracle):
    cover, pending = {}, 0
    for name in RS41_STREAMS:
        d, bits, recs = decoded(name)
        for c in range(len(bits)):
            off, pol = S.align(d, c, bits[c])
            S.check_plan(d, c, recs[c], off, pol, cover)
            info = {}
            R.reference(R.RS41, bits[c], c, info=info)
            want = [e["pos"] + off for e in d.plan[c] if e.get("pending")]
            assert ([info["pending"]] if "pending" in info else []) == want, (name, c, info, want)
            pending += "pending" in info
    req = S.required_coverage_rs41(RS41_STREAMS)
    missing = [k for k in req if k not in cover]
    assert not missing, (len(missing), missing[:10])
    assert pending >= 2
    print(f"FRAMER-REF RS41 coverage: {len(cover)} keys, none of the {len(req)} required ones missing; {pending} channels end inside a frame")


@pytest.mark.parametrize("name", RS41_STREAMS)
def test_rs41_designed_stream_behind_the_wide_modem(oracle, name):
    """the conditions hold behind the 2:1 modem too (the GPU test runs these streams under SONDE_FLAG_WIDE)"""
    d = S.rs41_streams()[name]()
    L = oracle_lib.lib()
    L.or_modem_set_decim(R.RS41, 2)
    try:
        x = d.iq.numpy()
        for c in range(x.shape[0]):
            ch = oracle_lib.Channel(R.RS41, c)
            ch.feed(x[c])
            bits = ch.bits()
            off, pol = S.check_conditions(d, c, bits)
            ref = R.reference(R.RS41, bits, c)
            assert ref.tobytes() == ch.frames().tobytes(), (name, c)
            S.check_plan(d, c, ref, off, pol, {})
            del ch
    finally:
        L.or_modem_set_decim(R.RS41, 4)


def test_rs41_l13_word_is_what_it_claims():
    """the planted word of the `L13` case: Berlekamp-Massey ends with L = 13 and 13 roots inside the codeword (t = 13 would correct it)"""
    for n in (24 + 132, 255):
        e, pos = S.rs41_l13_parity_error(n, 13)
        word = list(e) + [0] * (n - 24)
        assert R.rs41_rs_decode(word)[0] == -1
        ne, out = R.rs41_rs_decode(word, t=13)
        assert ne == 13 and sorted(k for k in range(n) if out[k] != word[k]) == sorted(pos)


# ------------------------------------------------------------------------------------------------ noisy scenes
RS41_NOISY_EBN0 = (9.0, 12.0)


@pytest.mark.parametrize("ebn0,seed", [(5.0, 1), (7.5, 2), (10.0, 3), (12.5, 4)])
def test_noisy_mixed_scene(oracle, ebn0, seed):
    """the scenes of test_gpu_fuzz_parity.run_mixed (the non-RS41 types of it, plus M20 and the AFSK types)"""
    n, total = 2048 * 96, 0
    for t, kw in ((1, {}), (2, {}), (3, {}), (3, dict(m20=True)), (6, {}), (4, {}), (5, {})):
        afsk = t in (4, 5)
        sb = synth.make_batch(t, 4 if afsk else 10, 16384 * 12 if afsk else n, seed=100 * seed + t, ebn0_db=ebn0 + 2.0,
                              **(kw if afsk else dict(kw, invert=(t == 1 and seed % 2 == 0), cfo_max_hz=500.0)))
        x = sb.iq.numpy()
        for c in range(x.shape[0]):
            ch = oracle_lib.Channel(t, c)
            ch.feed(x[c])
            fr = ch.frames()
            assert R.reference(t, ch.bits(), c).tobytes() == fr.tobytes(), (t, kw, c)
            total += len(fr)
    assert total > 0
    # RS41 at levels of its own (five channels each), so that clean, corrected and rejected codewords all occur in every one of the four
    # scenes: a codeword of 156 bytes is clean only where almost none has 13 wrong bytes, so no single level shows all three
    kinds = [0, 0, 0]
    for k, level in enumerate(RS41_NOISY_EBN0):
        sb = synth.make_batch(0, 5, n, seed=100 * seed + k, ebn0_db=level, cfo_max_hz=500.0, invert=seed % 2 == 0, extended=seed == 3)
        x = sb.iq.numpy()
        for c in range(x.shape[0]):
            ch = oracle_lib.Channel(0, c)
            ch.feed(x[c])
            fr = ch.frames()
            assert R.reference(0, ch.bits(), c).tobytes() == fr.tobytes(), (0, level, c)
            kinds = [kinds[0] + int((fr["nerr"] == 0).sum()), kinds[1] + int((fr["nerr"] > 0).sum()), kinds[2] + int((fr["nerr"] < 0).sum())]
            total += len(fr)
    assert min(kinds) > 0, kinds
    print(f"FRAMER-REF noisy {ebn0} dB: {total} records equal; RS41 at {RS41_NOISY_EBN0} dB: codewords clean / corrected / rejected {kinds}")


def test_afsk_complemented_bit_streams(oracle):
    """both polarities of the packet framers fed bit streams directly (no tone demodulator in front)"""
    for t, mk in ((4, lambda: synth.imet_bitstreams(3, np.arange(3), 4000, xdata=True)[0]), (5, lambda: synth.c50_bitstreams(3, np.arange(3), 4000)[0])):
        for comp in (0, 1):
            for c, b in enumerate(mk()):
                r = R.reference(t, b ^ comp, c)
                assert len(r) > 10 and (r["flags"] == comp).all() and (r["nerr"][:, 0] == 0).all()


# ------------------------------------------------------------------------------------------------ mutations
MUT_CASES = [(m, t) for m, (kw, types) in R.MUTATIONS.items() for t in types]


@pytest.mark.parametrize("mutation,stype", MUT_CASES, ids=[f"{m.replace(' ', '-')}-t{t}" for m, t in MUT_CASES])
def test_mutation_is_rejected(oracle, mutation, stype):
    """the mutated reference must differ from the oracle on at least one designed stream of the type"""
    kw = R.MUTATIONS[mutation][0]
    for name in (RS41_STREAMS if stype == R.RS41 else STREAMS):
        d, bits, recs = decoded(name)
        if d.stype != stype:
            continue
        for c in range(len(bits)):
            if R.reference(stype, bits[c], c, **kw).tobytes() != recs[c].tobytes():
                print(f"FRAMER-REF mutation '{mutation}' (type {stype}): rejected by stream {name}, channel {c}")
                return
    pytest.fail(f"no designed stream of type {stype} sees the mutation '{mutation}'")
