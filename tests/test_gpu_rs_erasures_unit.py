"""-m gpu: the errors-and-erasures RS(255,231) corrector alone (sonde_batch_test_rs255_erasures: rsee_decode_one of sd_rsee.h on
caller-supplied codeword pairs and erasure flags) against the twin's textbook decoder (tests/rescue_reference.py): erasure counts
0, 1, 12, 23, 24, 25 with unknown errors on both sides of 2 v + e = 24, erased bytes that happen to be right, erasures in the
parity bytes and at the last position.  Status and bytes must be the twin's exactly; within capacity the result is the encoded
word; without erasures the corrector agrees with the errors-only one (sonde_batch_test_rs255)."""
import ctypes as C

import numpy as np
import pytest

import rescue_reference as rr
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu
E_COUNTS = [0, 1, 12, 23, 24, 25]


def _words(n, rng, per_cell=12):
    """[(received, erased, encoded, e, v)]"""
    out = []
    for e in E_COUNTS:
        cap = max(0, (24 - e) // 2)
        for v in sorted({0, max(cap - 1, 0), cap, cap + 1, cap + 3}):
            for trial in range(per_cell):
                cw = rr.rs_encode(rng.integers(0, 256, size=n - 24))
                style = trial % 3
                if style == 0:                         # anywhere
                    pos = rng.choice(n, size=e + v, replace=False)
                elif style == 1:                       # erasures from the parity bytes and the last position first
                    head = np.concatenate([[n - 1], rng.permutation(24)])[:e]
                    rest = rng.permutation(np.setdiff1d(np.arange(n), head))
                    pos = np.concatenate([head, rest])[:e + v].astype(np.int64)
                else:                                  # a burst
                    start = int(rng.integers(0, n - (e + v) + 1))
                    pos = np.arange(start, start + e + v)
                    pos = np.concatenate([pos[v // 2: v // 2 + e], pos[:v // 2], pos[v // 2 + e:]])       # the erasures inside it
                er = np.zeros(256, dtype=np.uint8)
                er[pos[:e]] = 1
                r = np.zeros(256, dtype=np.uint8)
                r[:n] = cw
                for k in pos:
                    r[k] ^= int(rng.integers(1, 256))
                for k in pos[:e][: trial % 4]:         # erased bytes that happen to be right
                    r[k] = cw[k]
                out.append((r, er, cw, e, v))
    return out


@pytest.mark.parametrize("n", [24 + 132, 255])
def test_erasure_corrector_against_the_twin(n):
    rng = np.random.default_rng(1000 + n)
    words = _words(n, rng)
    words += [(np.concatenate([rng.integers(0, 256, size=n), np.zeros(256 - n)]).astype(np.uint8), (rng.random(256) < 0.05).astype(np.uint8), None, -1, -1)
              for _ in range(20)]                      # pure noise
    if len(words) % 2:
        words.append(words[0])
    order = rng.permutation(len(words))
    words = [words[i] for i in order]
    pairs = np.stack([w[0] for w in words]).reshape(-1, 2, 256)
    erased = np.stack([w[1] for w in words]).reshape(-1, 2, 256)
    erased[:, :, n:] = 1                               # flags beyond the codeword are ignored
    b = SondeBatch(1, 2048)
    got, status = b.test_rs255_erasures(pairs, erased, n)
    status = status.reshape(-1)
    got = got.reshape(-1, 256)
    seen = {}
    for i, (r, er, cw, e, v) in enumerate(words):
        st, w = rr.rs_decode_ee(r[:n], er[:n])
        assert status[i] == st, (i, e, v, status[i], st)
        assert np.array_equal(got[i, :n], np.array(w, dtype=np.uint8)), (i, e, v, st)
        assert not got[i, n:].any()
        if cw is not None and e <= 24 and 2 * v + e <= 24:
            assert st >= 0 and list(got[i, :n]) == cw, (i, e, v, st)
            assert st == int(np.count_nonzero(r[:n] != np.array(cw, dtype=np.uint8)))
        if e == 25:
            assert st == -1
        seen[(e, st >= 0)] = seen.get((e, st >= 0), 0) + 1
    for e in E_COUNTS:
        assert seen.get((e, True), 0) >= (2 if e < 25 else 0) and seen.get((e, False), 0) >= (2 if e != 24 else 0), seen
    # e = 0: the errors-only corrector's verdicts and bytes
    plain = pairs.copy()
    st0 = np.zeros((len(plain), 2), dtype=np.int32)
    rc = b.L.sonde_batch_test_rs255(b.h, plain.ctypes.data_as(C.c_void_p), len(plain), n, st0.ctypes.data_as(C.c_void_p))
    assert rc == 0, _lib.last_error()
    g0, s0 = b.test_rs255_erasures(pairs, np.zeros_like(erased), n)
    assert np.array_equal(s0, st0) and np.array_equal(g0, plain)
    assert (st0 == -1).sum() > 20 and (st0 > 0).sum() > 20
    b.close()
