"""Stage 3 (sync search, Manchester / biphase decode, de-interleaving, FEC and checks) of all seven sonde types in plain
Python, written from DESIGN.md SPEC 3.3, 3.3b-3.3e and 3.6 (RS41: and SURVEY.md Appendix B.2): it imports neither the oracle nor the
product and shares no arithmetic with them.  RS41 (type 0): its own header and mask constants, its own GF(2^8) tables, a textbook
Berlekamp-Massey / exhaustive root search / Forney decoder (rs41_rs_decode).  Hamming(8,4) is a nearest-codeword search over the 16 words of the null space; BCH(63,51) is the remainder of the block modulo
g(x) by long division, looked up in the table of the remainders of every error pattern of weight <= 2 over the full length 63 (no
GF(2^6) anywhere); the CRCs are bit-serial divisions (iMet: binascii.crc_hqx); the M10 checksum is SPEC 3.3b's byte recurrence.

reference(stype, bits, channel) takes one channel's whole chip / bit stream (one element per chip) and returns the frame records of
that channel.  It takes mutation keywords (MUTATIONS below), so that the tests can show that the designed streams reject the bugs
they exist for."""
from __future__ import annotations

import binascii
import itertools

import numpy as np

FRAME_MAX = 528
FRAME_DTYPE = np.dtype([("channel", "<u4"), ("type", "<u4"), ("len", "<i4"), ("nerr", "<i4", (2,)),
                        ("flags", "<u4"), ("bitpos", "<u8"), ("data", "u1", (FRAME_MAX,))])

RS41, DFM, IMS, M10, IMET, C50, MRZ = 0, 1, 2, 3, 4, 5, 6

# every mutation keyword of reference() with the value that switches it on, and the sonde types it applies to
MUTATIONS = {
    "thr+1": (dict(thr_norm=+1), (DFM, IMS, M10, MRZ)),
    "thr-1": (dict(thr_norm=-1), (DFM, IMS, M10, MRZ)),
    "inverted thr+1": (dict(thr_inv=+1), (DFM, M10, MRZ)),
    "inverted thr-1": (dict(thr_inv=-1), (DFM, M10, MRZ)),
    "inverted sync accepted": (dict(ims_inverted=True), (IMS,)),
    "latest position": (dict(latest=True), (DFM, IMS, M10, MRZ)),      # (DFM has no gap: its case is the sync planted inside a payload)
    "resume one chip early": (dict(resume=-1), (DFM, IMS, M10, MRZ)),
    "resume one chip late": (dict(resume=+1), (DFM, IMS, M10, MRZ)),
    "interleaver stride of block 0": (dict(dfm_stride=0), (DFM,)),
    "interleaver stride of block 1": (dict(dfm_stride=1), (DFM,)),
    "interleaver stride of block 2": (dict(dfm_stride=2), (DFM,)),
    "one Hamming decision": (dict(hamming_entry=0x5A), (DFM,)),
    "padding position accepted": (dict(bch_padding=True), (IMS,)),
    "positions modulo 46": (dict(bch_mod46=True), (IMS,)),
    "doubles counted as 1": (dict(bch_double_as_1=True), (IMS,)),
    "rejected block corrected anyway": (dict(bch_fix_rejected=True), (IMS,)),
    "M20 checksum over 99 bytes": (dict(m10_always_99=True), (M10,)),
    "checksum bytes swapped": (dict(m10_swap=True), (M10,)),
    "violations over 101 bytes": (dict(m10_viol_all=True), (M10,)),
    "CRC over 45 bytes": (dict(mrz_crc45=True), (MRZ,)),
    "CRC big-endian": (dict(mrz_big_endian=True), (MRZ,)),
    "stop bit not checked": (dict(imet_no_stop=True), (IMET,)),
    "XDATA length 4 + L": (dict(imet_xdata4=True), (IMET,)),
    "resume behind the stop bit": (dict(afsk_resume_behind=True), (IMET, C50)),
    "second sum not running": (dict(c50_plain_sum2=True), (C50,)),
    # RS41 (SPEC 3.3)
    "RS41 thr+1": (dict(thr_norm=+1), (RS41,)),
    "RS41 thr-1": (dict(thr_norm=-1), (RS41,)),
    "RS41 inverted thr+1": (dict(thr_inv=+1), (RS41,)),
    "RS41 inverted thr-1": (dict(thr_inv=-1), (RS41,)),
    "RS41 latest hit of 64 candidates": (dict(latest=True), (RS41,)),
    "RS41 resume one bit early": (dict(resume=-1), (RS41,)),
    "RS41 resume one bit late": (dict(resume=+1), (RS41,)),
    "RS41 resume behind the sync": (dict(resume_in_frame=True), (RS41,)),
    "RS41 tie goes to 518": (dict(tie_518=True), (RS41,)),
    "RS41 length from an exact 0xF0": (dict(len_exact=True), (RS41,)),
    "RS41 length byte not de-whitened": (dict(len_raw=True), (RS41,)),
    "RS41 length byte polarity kept": (dict(len_pol=True), (RS41,)),
    "RS41 mask aligned to the stream": (dict(mask_stream=True), (RS41,)),
    "RS41 codeword parities swapped": (dict(swap_parity=True), (RS41,)),
    "RS41 t = 11": (dict(t=11), (RS41,)),
    "RS41 t = 13": (dict(t=13), (RS41,)),
    "RS41 root in the padding accepted": (dict(pad_ok=True), (RS41,)),
    "RS41 rejected codeword partly rewritten": (dict(partial=True), (RS41,)),
    "RS41 bytes behind len not zeroed": (dict(tail_kept=True), (RS41,)),
    "RS41 nerr off by one": (dict(nerr_plus=1), (RS41,)),
}


def _msb_bits(v: int, n: int) -> np.ndarray:
    return np.array([(v >> (n - 1 - i)) & 1 for i in range(n)], dtype=np.uint8)


def manchester(bits) -> np.ndarray:
    b = np.asarray(bits, dtype=np.uint8)
    return np.stack([b, 1 - b], axis=-1).reshape(-1)


DFM_SYNC = manchester(_msb_bits(0x45CF, 16))
M10_SYNC = np.array([int(c) for c in "10011001100110010100110010011001"], dtype=np.uint8)
MRZ_SYNC = manchester(np.concatenate([_msb_bits(b, 8) for b in (0xAA, 0xBF, 0x35)]))
IMS_SYNC = _msb_bits(0x049DCE, 24)
DFM_CHIPS, M10_CHIPS, MRZ_CHIPS, IMS_CHIPS = 560, 32 + 16 * 101, 48 + 16 * 45, 2 * (24 + 12 * 46)
FIXED = {DFM: (DFM_SYNC, 3, DFM_CHIPS), M10: (M10_SYNC, 3, M10_CHIPS), MRZ: (MRZ_SYNC, 4, MRZ_CHIPS), IMS: (IMS_SYNC, 2, IMS_CHIPS)}


# ------------------------------------------------------------------------------------------------ sync search
def window_distances(stype: int, bits: np.ndarray) -> np.ndarray:
    """Hamming distance of every window to the type's sync pattern: hd[p] for the window that starts at chip p (iMS-100: of the 24
    decoded cells of the 48 chips from p on)"""
    bits = np.asarray(bits, dtype=np.uint8)
    sync = FIXED[stype][0]
    if stype == IMS:
        if len(bits) < 48:
            return np.zeros(0, dtype=np.int64)
        cell = (bits[:-1] == bits[1:]).astype(np.uint8)                  # cell[p] = 1 iff chips p and p + 1 are equal
        w = np.lib.stride_tricks.sliding_window_view(cell, 47)[:, ::2]  # cells p, p + 2, .. p + 46
    else:
        if len(bits) < len(sync):
            return np.zeros(0, dtype=np.int64)
        w = np.lib.stride_tricks.sliding_window_view(bits, len(sync))
    hd = np.zeros(w.shape[0], dtype=np.int64)
    for lo in range(0, w.shape[0], 1 << 16):
        hd[lo:lo + (1 << 16)] = (w[lo:lo + (1 << 16)] != sync[None, :]).sum(axis=1)
    return hd


def fixed_frames(stype: int, bits: np.ndarray, *, thr_norm=0, thr_inv=0, ims_inverted=False, latest=False, resume=0, info=None):
    """[(fstart, inverted)] of every complete frame: earliest matching window wins, a frame is emitted only when all its chips
    exist, the search resumes at fstart + frame chips.  info["pending"]: the start of a frame that the end of the stream cut."""
    sync, thr, flen = FIXED[stype]
    hd = window_distances(stype, bits)
    norm = hd <= thr + thr_norm
    inv = (hd >= len(sync) - (thr + thr_inv)) & ~norm if (stype != IMS or ims_inverted) else np.zeros_like(norm)
    hits = np.nonzero(norm | inv)[0]
    out, pos = [], 0
    while True:
        k = np.searchsorted(hits, pos)
        if k == len(hits):
            break
        p = int(hits[k])
        if latest:                                                       # (mutation) the last match inside the frame's span
            p = int(hits[np.searchsorted(hits, p + flen) - 1])
        if p + flen > len(bits):
            if info is not None:
                info["pending"] = p
            break
        out.append((p, bool(inv[p])))
        pos = p + flen + resume
    return out


# ------------------------------------------------------------------------------------------------ Hamming(8,4)
def _parity(v: int) -> int:
    return bin(v).count("1") & 1


HAMMING_CODEBOOK = [w for w in range(256) if not any(_parity(w & r) for r in (0x78, 0xB4, 0xD2, 0xE1))]
assert len(HAMMING_CODEBOOK) == 16


def hamming_decide(w: int):
    """(word out, status): distance 0 -> clean (0), 1 -> the codeword (1), 2 -> the word as received (-1)"""
    d = [bin(w ^ c).count("1") for c in HAMMING_CODEBOOK]
    m = min(d)
    if m == 0:
        return w, 0
    if m == 1:
        return HAMMING_CODEBOOK[d.index(1)], 1
    assert m == 2
    return w, -1


HAMMING_TABLE = [hamming_decide(w) for w in range(256)]


def dfm_decode(chips: np.ndarray, *, dfm_stride=None, hamming_entry=None):
    """chips: the 560 chips of a frame, polarity already removed -> (33 words, corrected words, uncorrectable words)"""
    first = chips[32::2]                                                 # the first chip of each of the 264 payload bits
    out, ncorr, nbad, off = [], 0, 0, 0
    for blk, n in enumerate((7, 13, 13)):
        stride = n - 1 if dfm_stride == blk else n
        for i in range(n):
            w = 0
            for j in range(8):
                w = (w << 1) | int(first[off + j * stride + i])
            v, st = HAMMING_TABLE[w]
            if hamming_entry is not None and w == hamming_entry:         # (mutation) one entry of the decision table
                v, st = w ^ 0x01, 1
            out.append(v)
            ncorr += st == 1
            nbad += st == -1
        off += 8 * n
    return out, ncorr, nbad


# ------------------------------------------------------------------------------------------------ BCH(63,51) shortened to (46,34)
BCH_G = 0x1539


def poly_mod(v: int, g: int = BCH_G) -> int:
    dg = g.bit_length() - 1
    while v.bit_length() - 1 >= dg:
        v ^= g << (v.bit_length() - 1 - dg)
    return v


def _bch_table():
    single = [poly_mod(1 << i) for i in range(63)]
    t = {}
    for i in range(63):
        t[single[i]] = (i,)
    for i, j in itertools.combinations(range(63), 2):
        t[single[i] ^ single[j]] = (i, j)
    assert len(t) == 63 + 1953 and 0 not in t                            # all distinct: the code's distance is 5
    return t


BCH_TABLE = _bch_table()


def bch_decide(blk: int, *, bch_padding=False, bch_mod46=False, bch_double_as_1=False, bch_fix_rejected=False):
    """blk: 46 bits, bit 45 first on air (bit i = coefficient of x^i).  (block out, status): status = corrected bits, -1 rejected"""
    r = poly_mod(blk)
    if r == 0:
        return blk, 0
    pos = BCH_TABLE.get(r)
    if pos is None:
        return blk, -1
    if bch_mod46:
        pos = tuple(p % 46 for p in pos)
    if all(p < 46 for p in pos):
        for p in pos:
            blk ^= 1 << p
        return blk, 1 if bch_double_as_1 else len(pos)
    if bch_padding or bch_fix_rejected:                                  # (mutations) the valid positions flipped all the same
        for p in pos:
            if p < 46:
                blk ^= 1 << p
        return blk, len(pos) if bch_padding else -1
    return blk, -1


def ims_decode(chips: np.ndarray, **mut):
    """chips: the 1152 chips of a frame -> (51 data bytes, corrected bits, rejected blocks)"""
    cells = (chips[48::2] == chips[49::2]).astype(np.uint8)            # 552 block bits
    dbits, ncorr, nbad = [], 0, 0
    for b in range(12):
        blk = 0
        for k in range(46):
            blk = (blk << 1) | int(cells[46 * b + k])
        blk, st = bch_decide(blk, **mut)
        ncorr += max(st, 0)
        nbad += st < 0
        dbits += [(blk >> (45 - k)) & 1 for k in range(34)]
    return np.packbits(np.array(dbits, dtype=np.uint8)), ncorr, nbad


# ------------------------------------------------------------------------------------------------ M10 / M20, MRZ-N1
def m10_checksum(data) -> int:
    """SPEC 3.3b: c <- ((c & 0xFF) << 8) | (b' ^ t ^ s) per byte b, c = 0 before the first"""
    c = 0
    for b in data:
        b = int(b)
        b1 = ((b >> 1) | (b << 7)) & 0xFF                                # the byte rotated right by one
        b1 ^= b1 >> 2
        t = c & 0x3F
        t |= (((c >> 0) ^ (c >> 2) ^ (c >> 4)) & 1) << 6
        t |= (((c >> 1) ^ (c >> 3) ^ (c >> 5)) & 1) << 7
        s = (c >> 7) & 0xFF
        s ^= s >> 2
        c = ((c & 0xFF) << 8) | (b1 ^ t ^ s)
    return c


def crc16_reflected(data, poly: int = 0xA001, init: int = 0xFFFF) -> int:
    """bit-serial division, least significant bit of every byte first"""
    crc = init
    for b in data:
        for k in range(8):
            fb = (crc ^ (int(b) >> k)) & 1
            crc >>= 1
            if fb:
                crc ^= poly
    return crc


def manchester_bytes(chips: np.ndarray, nbytes: int):
    """(bytes MSB first from the first chips, violations per byte)"""
    a, b = chips[0:16 * nbytes:2], chips[1:16 * nbytes:2]
    return np.packbits(a), (a == b).reshape(nbytes, 8).sum(axis=1)


def m10_decode(chips: np.ndarray, *, m10_always_99=False, m10_swap=False, m10_viol_all=False):
    data, viol = manchester_bytes(chips[32:], 101)
    total = 70 if data[0] == 0x45 else 101
    ncs = 101 if m10_always_99 else total
    cs = m10_checksum(data[:ncs - 2])
    hi, lo = int(data[ncs - 2]), int(data[ncs - 1])
    stored = (lo << 8 | hi) if m10_swap else (hi << 8 | lo)
    return data[:total], total, 0 if cs == stored else -1, int(viol[:101 if m10_viol_all else total].sum())


def mrz_decode(chips: np.ndarray, *, mrz_crc45=False, mrz_big_endian=False):
    data, viol = manchester_bytes(chips[48:], 45)
    crc = crc16_reflected(data[:45 if mrz_crc45 else 43])
    stored = (int(data[43]) << 8 | int(data[44])) if mrz_big_endian else (int(data[44]) << 8 | int(data[43]))
    return data, 0 if crc == stored else -1, int(viol.sum())


# ------------------------------------------------------------------------------------------------ the AFSK packet framers
IMET_SYNC = np.array([1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0], dtype=np.uint8)                   # stop / idle, the character 0x01, a start bit
C50_SYNC = np.array([1, 0] + [0] * 8 + [1, 0] + [1] * 8 + [1], dtype=np.uint8)             # stop / idle, the characters 00 and FF


def _char(bits: np.ndarray, at: int, check_stop: bool = True):
    """(value, framing ok) of the 8N1 character whose start bit is bits[at]"""
    v = 0
    for m in range(8):
        v |= int(bits[at + 1 + m]) << m
    return v, bits[at] == 0 and (bits[at + 9] == 1 or not check_stop)


def afsk_packets(stype: int, bits: np.ndarray, *, imet_no_stop=False, imet_xdata4=False, afsk_resume_behind=False,
                 c50_plain_sum2=False, info=None):
    """[(bitpos, inverted, packet bytes, nerr0)]; info["drops"]: why each dropped candidate was dropped"""
    bits = np.asarray(bits, dtype=np.uint8)
    sync = IMET_SYNC if stype == IMET else C50_SYNC
    n, ns = len(bits), len(sync)
    drops = []
    out = []
    if n >= ns:
        w = np.lib.stride_tricks.sliding_window_view(bits, ns)
        hd = (w != sync[None, :]).sum(axis=1)
        cands = np.nonzero((hd == 0) | (hd == ns))[0]
    else:
        cands, hd = np.zeros(0, dtype=np.int64), None
    pos = 0
    while True:
        k = np.searchsorted(cands, pos)
        if k == len(cands):
            break
        p = int(cands[k])
        inv = int(hd[p] == ns)
        c0 = p + 1                                                        # the first start bit
        if stype == IMET:
            if c0 + 30 > n:
                break
            v = bits[c0:c0 + 30] ^ inv
            ptype, ok1 = _char(v, 10, not imet_no_stop)
            lenb, ok2 = _char(v, 20, not imet_no_stop)
            length = {1: 14, 2: 18, 3: (4 if imet_xdata4 else 5) + lenb, 4: 20}.get(ptype, 0)
            if not (ok1 and ok2):
                drops.append("framing")
                pos = p + 1
                continue
            if length == 0 or length > 64:
                drops.append("type" if length == 0 else "length")
                pos = p + 1
                continue
        else:
            length = 9
        if c0 + 10 * length > n:
            break
        v = bits[c0:c0 + 10 * length] ^ inv
        chars = [_char(v, 10 * j, not (imet_no_stop and stype == IMET)) for j in range(length)]
        if not all(ok for _, ok in chars):
            drops.append("framing")
            pos = p + 1
            continue
        pkt = bytes(c for c, _ in chars)
        if stype == IMET:
            good = binascii.crc_hqx(pkt[:-2], 0x1D0F) == (pkt[-2] << 8 | pkt[-1])
        else:
            c1 = c2 = 0
            for x in pkt[2:7]:
                c1 = (c1 + x) & 0xFF
                c2 = (c2 + (x if c50_plain_sum2 else c1)) & 0xFF
            good = c1 == pkt[7] and c2 == pkt[8]
        out.append((c0, inv, pkt, 0 if good else -1))
        pos = c0 + 10 * length - (0 if afsk_resume_behind else 1)       # the last stop bit may open the next sync
    if info is not None:
        info["drops"] = drops
    return out



# ------------------------------------------------------------------------------------------------ RS41 (SPEC 3.3)
RS41_HEADER = bytes.fromhex("10B6CA11229612F8")                         # on air, every byte least significant bit first
RS41_MASK = bytes.fromhex("96833E51B1490898320559 0EF944C626 2160C2EA795D6DA15469470CDCE85CF1 F776827F0799A22C937C3063F5102E61"
                          "D0BCB4B606AAF423786E3BAEBF7B4CC1".replace(" ", ""))
assert len(RS41_MASK) == 64 and bytes(a ^ b for a, b in zip(RS41_HEADER, RS41_MASK)) == bytes.fromhex("8635F44093DF1A60")   # B.2's check
RS41_HEADER_BITS = np.array([(RS41_HEADER[i >> 3] >> (i & 7)) & 1 for i in range(64)], dtype=np.uint8)

GF_EXP, GF_LOG = [0] * 510, [0] * 256
_v = 1
for _i in range(255):
    GF_EXP[_i] = GF_EXP[_i + 255] = _v
    GF_LOG[_v] = _i
    _v = (_v << 1) ^ (0x11D if _v & 0x80 else 0)


def gf_mul(a: int, b: int) -> int:
    return GF_EXP[GF_LOG[a] + GF_LOG[b]] if a and b else 0


def gf_inv(a: int) -> int:
    return GF_EXP[255 - GF_LOG[a]]


def gf_poly_at(p, x: int) -> int:
    """p[0] + p[1] x + p[2] x^2 + ..."""
    r = 0
    for c in reversed(p):
        r = gf_mul(r, x) ^ c
    return r


def rs41_rs_decode(word, *, t=12, pad_ok=False, partial=False):
    """RS(255,231) shortened to len(word), roots alpha^0..alpha^23, position k = the coefficient of x^k: (corrected bytes or -1, word).
    SPEC 3.3: failure iff L > 12, deg Lambda != L, root count != L, a root in the padding, or a zero Forney denominator."""
    w = [int(v) for v in word]
    n = len(w)
    S = [gf_poly_at(w, GF_EXP[j]) for j in range(24)]
    if not any(S):
        return 0, w
    lam, B, L, m, b = [1], [1], 0, 1, 1                                  # Berlekamp-Massey, the textbook recurrence
    for r in range(24):
        d = S[r]
        for i in range(1, min(L, len(lam) - 1) + 1):
            d ^= gf_mul(lam[i], S[r - i])
        if d == 0:
            m += 1
            continue
        f = gf_mul(d, gf_inv(b))
        new = lam + [0] * max(0, len(B) + m - len(lam))
        for i, c in enumerate(B):
            new[i + m] ^= gf_mul(f, c)
        if 2 * L <= r:
            L, B, b, m = r + 1 - L, lam, d, 1
        else:
            m += 1
        lam = new
    while len(lam) > 1 and lam[-1] == 0:
        lam.pop()
    if L > t or len(lam) - 1 != L:
        return -1, w
    roots = [k for k in range(255) if gf_poly_at(lam, GF_EXP[(255 - k) % 255]) == 0]
    if len(roots) != L:
        return -1, w
    omega = [0] * 24
    for i in range(24):
        for k in range(min(i, L) + 1):
            omega[i] ^= gf_mul(lam[k], S[i - k])
    dlam = [lam[k] if k & 1 else 0 for k in range(1, L + 1)]           # the formal derivative: odd terms survive
    vals = []
    for k in roots:
        xi = GF_EXP[(255 - k) % 255]
        den = gf_poly_at(dlam, xi)
        if den == 0:
            return -1, w
        vals.append(gf_mul(GF_EXP[k], gf_mul(gf_poly_at(omega, xi), gf_inv(den))))
    out = list(w)
    for k, v in zip(roots, vals):
        if k < n:
            out[k] ^= v
    if any(k >= n for k in roots) and not pad_ok:
        return -1, (out if partial else w)                               # (mutation `partial`: the valid positions rewritten all the same)
    return L, out


def _lsb_bytes(bits: np.ndarray) -> np.ndarray:
    return np.packbits(bits[:len(bits) // 8 * 8].reshape(-1, 8), axis=1, bitorder="little")[:, 0]


def rs41_frames(bits: np.ndarray, *, thr_norm=0, thr_inv=0, latest=False, resume=0, resume_in_frame=False, tie_518=False,
                len_exact=False, len_raw=False, len_pol=False, info=None):
    """[(fstart, inverted, frame bytes)] of every complete frame.  The earliest window within 6 bits of the header (58 or more: inverted)
    wins; byte 56, polarity undone and de-whitened, decides the length (nearer to 0xF0 than to 0x0F: 518, else, a tie included,
    320); a frame is emitted when all its bits exist; the search resumes at its last bit + 1.  info["pending"]: the start of a frame
    that the end of the stream cut (found, but no record)."""
    n = len(bits)
    if n < 64:
        return []
    hd = (np.lib.stride_tricks.sliding_window_view(bits, 64) != RS41_HEADER_BITS[None, :]).sum(axis=1)
    norm = hd <= 6 + thr_norm
    inv = (hd >= 58 - thr_inv) & ~norm
    hits = np.nonzero(norm | inv)[0]
    out, pos = [], 0
    while True:
        k = np.searchsorted(hits, pos)
        if k == len(hits):
            break
        p = int(hits[k])
        if latest:                                                       # (mutation) the last match among the 64 candidates from p on
            p = int(hits[np.searchsorted(hits, p + 64) - 1])
        x = 0xFF if inv[p] else 0
        if p + 8 * 57 > n:
            if info is not None:
                info["pending"] = p
            break
        tb = int(_lsb_bytes(bits[p + 448:p + 456])[0]) ^ (0 if len_pol else x) ^ (0 if len_raw else RS41_MASK[56])
        d518, d320 = bin(tb ^ 0xF0).count("1"), bin(tb ^ 0x0F).count("1")
        ext = tb == 0xF0 if len_exact else (d518 <= d320 if tie_518 else d518 < d320)
        flen = 518 if ext else 320
        if p + 8 * flen > n:
            if info is not None:
                info["pending"] = p
            break
        out.append((p, bool(inv[p]), flen))
        pos = p + 64 if resume_in_frame else p + 8 * flen + resume
    return out


def rs41_record(bits: np.ndarray, p: int, inv: bool, flen: int, *, mask_stream=False, swap_parity=False, tail_kept=False, nerr_plus=0, **rs):
    """(528 data bytes, nerr[2]): the frame de-whitened with the mask aligned to its start (the 8 header bytes too: as received),
    then each codeword c: parity frame[8 + 24 c .. 32 + 24 c) at positions 0..23, frame[56 + 2 i + c] at 24 + i"""
    have = min(FRAME_MAX if tail_kept else flen, (len(bits) - p) // 8)
    raw = _lsb_bytes(bits[p:p + 8 * have]) ^ np.uint8(0xFF if inv else 0)
    m0 = (p // 8) if mask_stream else 0
    d = [int(raw[i]) ^ RS41_MASK[(i + m0) & 63] for i in range(have)] + [0] * (FRAME_MAX - have)
    nerr = []
    for c in (0, 1):
        pc = 1 - c if swap_parity else c
        word = d[8 + 24 * pc:32 + 24 * pc] + d[56 + c:flen:2]
        ne, word = rs41_rs_decode(word, **rs)
        d[8 + 24 * pc:32 + 24 * pc] = word[:24]
        d[56 + c:flen:2] = word[24:]
        nerr.append(ne + nerr_plus if ne > 0 else ne)
    return d, nerr

# ------------------------------------------------------------------------------------------------ records
_FRAMER_KW = ("thr_norm", "thr_inv", "ims_inverted", "latest", "resume")
_RS41_FRAMER_KW = ("thr_norm", "thr_inv", "latest", "resume", "resume_in_frame", "tie_518", "len_exact", "len_raw", "len_pol")


def reference(stype: int, bits, channel: int, *, info=None, **mut) -> np.ndarray:
    """the frame records of one channel's whole chip / bit stream; `mut`: the keywords of MUTATIONS; info: a dict that receives
    "pending" (RS41 and the fixed-length types) or "drops" (AFSK types)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    recs = []

    def rec(length, nerr0, nerr1, flags, bitpos, data):
        r = np.zeros((), dtype=FRAME_DTYPE)
        r["channel"], r["type"], r["len"], r["flags"], r["bitpos"] = channel, stype, length, flags, bitpos
        r["nerr"] = (nerr0, nerr1)
        r["data"][:length] = np.frombuffer(bytes(data), dtype=np.uint8)[:length]
        recs.append(r)

    if stype == RS41:
        fkw = {k: v for k, v in mut.items() if k in _RS41_FRAMER_KW}
        dkw = {k: v for k, v in mut.items() if k not in _RS41_FRAMER_KW}
        for p, inv, flen in rs41_frames(bits, info=info, **fkw):
            data, nerr = rs41_record(bits, p, inv, flen, **dkw)
            rec(flen, nerr[0], nerr[1], int(inv), p, data[:flen])
            if dkw.get("tail_kept"):
                recs[-1]["data"][:] = np.array(data, dtype=np.uint8)
    elif stype in (IMET, C50):
        for c0, inv, pkt, ne in afsk_packets(stype, bits, info=info, **mut):
            rec(len(pkt), ne, 0, inv, c0, pkt)
    else:
        fkw = {k: v for k, v in mut.items() if k in _FRAMER_KW}
        dkw = {k: v for k, v in mut.items() if k not in _FRAMER_KW}
        flen = FIXED[stype][2]
        for p, inv in fixed_frames(stype, bits, info=info, **fkw):
            chips = bits[p:p + flen] ^ np.uint8(inv)
            if stype == DFM:
                words, nc, nb = dfm_decode(chips, **dkw)
                rec(33, nc, nb, int(inv), p, words)
            elif stype == IMS:
                data, nc, nb = ims_decode(chips, **dkw)
                rec(51, nc, nb, 0, p, data)
            elif stype == M10:
                data, total, ne, viol = m10_decode(chips, **dkw)
                rec(total, ne, viol, int(inv), p, data)
            elif stype == MRZ:
                data, ne, viol = mrz_decode(chips, **dkw)
                rec(45, ne, viol, int(inv), p, data)
            else:
                raise ValueError(stype)
    return np.array(recs, dtype=FRAME_DTYPE) if recs else np.zeros(0, dtype=FRAME_DTYPE)
