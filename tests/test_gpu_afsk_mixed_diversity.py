"""-m gpu: iMet and C50 groups (SONDE_FLAG_AFSK_DIVERSITY, DESIGN SPEC 3.3o) next to RS41, M10 and DFM groups in one table, after
tests/test_gpu_all_kinds_diversity.py: one pair each and an ungrouped iMet and C50 channel.  With all groups set the records of every
submit are those of the same batch without groups passed through each kind's twin in turn on its own group; only records of grouped
AFSK channels differ from the run without the AFSK groups, and the other kinds' records are byte for byte what they are with their
own groups alone.  The rows are the first pair of each kind's damaged scene, cut or repeated to 12 granules of the AFSK chain."""
import functools

import numpy as np
import pytest
import torch

import afsk_diversity_reference as ad
import afsk_diversity_scenes as afs
import check_diversity_reference as ckr
import check_diversity_scenes as cks
import dfm_diversity_reference as dfr
import dfm_diversity_scenes as dfs
import diversity_reference as dr
import diversity_scenes as ds
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 12 * afs.GRANULE
OTHERS = [[0, 1], [2, 3], [4, 5]]                              # RS41, M10, DFM
GROUPS = OTHERS + [[6, 7], [8, 9]]                             # iMet, C50; channels 10 (iMet) and 11 (C50) are in no group


@functools.lru_cache(maxsize=None)
def batch_rows():
    def fit(rows):
        return np.concatenate([rows] * -(-N // rows.shape[1]), axis=1)[:, :N]

    src = [(dr.RS41, ds.scene().iq[:2]), (cks.M10, cks.scene("m10").iq[:2]), (dfs.DFM, dfs.scene().iq[:2]),
           (afs.IMET4, afs.scene("imet").iq[:2]), (afs.C50, afs.scene("c50").iq[:2]), (afs.IMET4, afs.scene("imet").iq[9:10]),
           (afs.C50, afs.scene("c50").iq[9:10])]
    types = np.array([t for t, rows in src for _ in rows], dtype=np.uint8)
    return types, np.ascontiguousarray(np.concatenate([fit(rows) for _, rows in src]))


def _sort(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


def _only(g, groups):
    return [members if k == g else [] for k, members in enumerate(groups)]


def twins(records, states, afsk):
    w = records
    w, _, states["rs41"] = dr.diversity(w, _only(0, GROUPS), None, 960, states["rs41"])
    w, _, states["m10"] = ckr.diversity(w, _only(1, GROUPS), None, 960, states["m10"])
    w, _, states["dfm"] = dfr.diversity(w, _only(2, GROUPS), None, 960, states["dfm"])
    if afsk:
        w, _, states["afsk"] = ad.diversity(w, [[], [], []] + GROUPS[3:], None, 0, states["afsk"])
    return w


@pytest.mark.parametrize("cuts", [1, 3], ids=["1_submit", "3_submits"])
def test_afsk_groups_next_to_the_other_kinds(cuts):
    types, rows = batch_rows()
    iq = torch.from_numpy(rows).to(DEV)
    step = N // cuts
    mk = lambda: SondeBatch(len(types), step, types=types, flags=_lib.FLAG_AFSK_DIVERSITY)      # noqa: E731
    b0, b1, b = mk(), mk(), mk()
    b1.set_diversity(OTHERS)
    b.set_diversity(GROUPS)
    st1, st = dict.fromkeys(["rs41", "m10", "dfm", "afsk"]), dict.fromkeys(["rs41", "m10", "dfm", "afsk"])
    changed = set()
    for k in range(cuts):
        for x in (b0, b1, b):
            x.submit(iq[:, k * step:(k + 1) * step])
        off, others, on = _sort(b0.frames()), _sort(b1.frames()), _sort(b.frames())
        want1, want = twins(off, st1, False), twins(off, st, True)
        assert len(on) == len(others) == len(off)
        assert others.tobytes() == want1.tobytes()
        for a, e, o in zip(on, want, others):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))
            if a.tobytes() != o.tobytes():                     # only records of grouped AFSK channels differ from the run without the AFSK groups
                changed.add(int(a["channel"]))
        afsk = np.isin(on["type"], (afs.IMET4, afs.C50))
        assert on[~afsk].tobytes() == others[~afsk].tobytes() and others[afsk].tobytes() == off[afsk].tobytes()
    assert changed and changed <= {6, 7, 8, 9} and {c // 2 for c in changed} == {3, 4}
    for g, kind in enumerate(["rs41", "m10", "dfm", "afsk", "afsk"]):
        assert st[kind]["combined"][g] >= 1, (g, st[kind]["combined"])
        assert b.diversity_info(g) == {"tried": st[kind]["tried"][g], "combined": st[kind]["combined"][g]}, g
    for x in (b0, b1, b):
        x.close()
