"""-m gpu: the M10 groups of sonde_batch_set_diversity (DESIGN SPEC 3.3l) at high stream age (SPEC 3.13), as tests/test_gpu_stream_age.py
does it for RS41 groups: the scene of check_diversity_scenes fed twice over in 20 submits, every member's origin moved past 2^32 and
past 2^37 chips by sonde_batch_test_shift_age once a pair, the triple and the quad have each combined a frame (so that carried records
exist and must move); the records equal the unaged run's with bitpos shifted, byte for byte, and so do the counters and offsets."""
import numpy as np
import pytest
import torch

import age_scenes as A
import check_diversity_scenes as cs
import demod_reference as D
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("boundary", [1 << 32, 1 << 37], ids=["2^32", "2^37"])
@pytest.mark.parametrize("mode", ["offsets", "learn_mark"])
def test_m10_groups_across_the_boundary(mode, boundary):
    sc = cs.scene("m10")
    iq = torch.from_numpy(sc.iq).to(DEV)
    iq = torch.cat([iq, iq], dim=1).contiguous()
    C, n, cuts = sc.C, 2 * sc.n, 20
    step = n // cuts
    types = np.full(C, sc.type, dtype=np.uint8)
    ring = A.ring_bits_of([D.modem(sc.type)], step)
    kw = dict(offsets=sc.offsets) if mode == "offsets" else dict(offsets=None, learn=True, mark_duplicates=True)

    def run(shift_after=None):
        b = SondeBatch(C, step, types=types)
        b.set_diversity(sc.groups, window_bits=sc.window, **kw)
        parts, added = [], 0
        for k in range(cuts):
            b.submit(iq[:, k * step:(k + 1) * step])
            parts.append((b.frames(), [added] * C))
            if k == shift_after:
                turns = A.turns_below(boundary, max(b.nbits(c) for c in range(C)), ring)
                got = b.test_shift_age(np.arange(C), [0] * C, [turns] * C)
                assert all(int(g) == turns * ring for g in got)
                added = turns * ring
        return b, parts, added

    a, pa, _ = run()
    comb = [{int(c) for c in f["channel"][f["flags"] & _lib.FRAME_COMBINED != 0]} for f, _ in pa]
    sizes = {len(g): {c for h in sc.groups if len(h) == len(g) for c in h} for g in sc.groups}
    # the first submit by which a pair, the triple and the quad have each combined a frame
    k0 = next(k for k in range(cuts) if all(any(c in members for s in comb[:k + 1] for c in s) for members in sizes.values()))
    assert sum(len(s) for s in comb[k0 + 1:]) >= 10, "too few frames are combined behind the shift"
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
        assert b.nbits(c) == a.nbits(c) + added > boundary, c
    a.close()
    b.close()
