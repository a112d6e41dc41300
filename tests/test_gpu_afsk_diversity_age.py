"""-m gpu: the iMet and C50 groups of sonde_batch_set_diversity (DESIGN SPEC 3.3o) at high stream age (SPEC 3.13), as
tests/test_gpu_check_diversity_age.py does it for M10 groups: the scene of afsk_diversity_scenes fed over and over, granule by granule
-- the shift moves a stream by whole ring turns, so it lands up to a ring's length below the boundary, and the stream goes on for more
than a ring's length behind the shift so that it crosses --, every member's origin moved past 2^32 symbols by sonde_batch_test_shift_age once a pair, the triple and the quad have each combined a
packet (so that carried records exist and must move); the records equal the unaged run's with bitpos shifted, byte for byte, and so do
the counters and offsets."""
import numpy as np
import pytest
import torch

import afsk_diversity_scenes as ds
import age_scenes as A
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDARY = 1 << 32


@pytest.mark.parametrize("kind,mode", [("imet", "offsets"), ("imet", "learn_mark"), ("c50", "offsets")])
def test_afsk_groups_across_2_to_the_32(kind, mode):
    sc = ds.scene(kind)
    C, step = sc.C, ds.GRANULE
    types = np.full(C, sc.type, dtype=np.uint8)
    # the ring's length, from a batch of its own: one turn says it.  The scene is fed two times (by then a pair, the triple and the
    # quad have combined) and then for more than a ring's length
    probe = SondeBatch(C, step, types=types, flags=_lib.FLAG_AFSK_DIVERSITY)
    probe.submit(torch.from_numpy(sc.iq[:, :step]).to(DEV))
    ring = int(probe.test_shift_age(np.arange(C), [0] * C, [1] * C)[0])
    probe.close()
    reps = 2 + -(-ring // (sc.nbits - 16))
    iq = torch.from_numpy(sc.iq).to(DEV).repeat(1, reps, 1).contiguous()
    n = reps * sc.n
    cuts = n // step
    kw = dict(offsets=sc.offsets) if mode == "offsets" else dict(offsets=None, learn=True, mark_duplicates=True)

    def run(shift_after=None):
        b = SondeBatch(C, step, types=types, flags=_lib.FLAG_AFSK_DIVERSITY)
        b.set_diversity(sc.groups, window_bits=0, **kw)
        parts, added = [], 0
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            parts.append((b.frames(), [added] * C))
            if k == shift_after:
                turns = A.turns_below(BOUNDARY, max(b.nbits(c) for c in range(C)), ring)
                got = b.test_shift_age(np.arange(C), [0] * C, [turns] * C)
                assert all(int(g) == turns * ring for g in got)
                added = turns * ring
        return b, parts, added

    a, pa, _ = run()
    comb = [{int(c) for c in f["channel"][f["flags"] & _lib.FRAME_COMBINED != 0]} for f, _ in pa]
    sizes = {len(g): {c for h in sc.groups if len(h) == len(g) for c in h} for g in sc.groups}
    # the first submit by which a pair, the triple and the quad have each combined a packet
    k0 = next(k for k in range(cuts) if all(any(c in members for s in comb[:k + 1] for c in s) for members in sizes.values()))
    assert k0 < 2 * sc.n // step
    assert sum(len(s) for s in comb[k0 + 1:]) >= 10, "too few packets are combined behind the shift"
    b, pb, added = run(shift_after=k0)
    for k, ((fa, _), (fb, add)) in enumerate(zip(pa, pb)):
        why = A.frames_diff(fa, fb, add)
        assert not why, (k, why[:3])
    if mode == "learn_mark":
        assert sum(int((f["flags"] & _lib.FRAME_DUPLICATE != 0).sum()) for f, _ in pa[k0 + 1:]) > 0
    for g in range(len(sc.groups)):
        assert b.diversity_info(g) == a.diversity_info(g), g
        assert b.diversity_offsets(g) == a.diversity_offsets(g), g
    for c in range(C):
        assert b.nbits(c) == a.nbits(c) + added > BOUNDARY, c
    a.close()
    b.close()
