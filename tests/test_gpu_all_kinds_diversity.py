"""-m gpu: sonde_batch_set_diversity with a group of EVERY kind in one table (DESIGN SPEC 3.3j, 3.3l, 3.3m, 3.3n): one pair each of RS41,
M10, MRZ-N1, DFM and iMS-100 (SONDE_FLAG_IMS_DIVERSITY) and one ungrouped channel.  Every combining kernel is launched over the
whole table and takes the groups of its kinds, so with groups set the records of every submit are those of the same batch without
groups passed through each kind's twin in turn on its own group, whole records byte for byte, and diversity_info reports the twins'
counters; every kind combines at least one frame, so no pass can be left out unnoticed.  The rows are the first pair of each kind's
damaged scene, cut or repeated to 100 tiles."""
import functools

import numpy as np
import pytest
import torch

import check_diversity_reference as ckr
import check_diversity_scenes as cks
import dfm_diversity_reference as dfr
import dfm_diversity_scenes as dfs
import diversity_reference as dr
import diversity_scenes as ds
import ims_diversity_reference as imr
import ims_diversity_scenes as ims
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, TILES = ds.TILE, 100
KINDS = ["rs41", "m10", "mrz", "dfm", "ims"]
GROUPS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]              # group g is of kind KINDS[g]; channel 10 is in no group


@functools.lru_cache(maxsize=None)
def batch_rows():
    """(types [11], iq [11, n, 2] float32 numpy): channels 2 g, 2 g + 1 = the first pair of kind g's scene (both receivers of stream 0,
    offsets zero), channel 10 = the DFM scene's ungrouped receiver"""
    n = TILE * TILES

    def fit(rows):
        return np.concatenate([rows] * -(-n // rows.shape[1]), axis=1)[:, :n]

    src = [(dr.RS41, ds.scene().iq[:2]), (cks.M10, cks.scene("m10").iq[:2]), (cks.MRZN1, cks.scene("mrz").iq[:2]),
           (dfs.DFM, dfs.scene().iq[:2]), (ims.IMS, ims.scene().iq[:2]), (dfs.DFM, dfs.scene().iq[7:8])]
    types = np.array([t for t, rows in src for _ in rows], dtype=np.uint8)
    return types, np.ascontiguousarray(np.concatenate([fit(rows) for _, rows in src]))


def _sort(fr):
    return fr[np.lexsort((fr["bitpos"], fr["channel"]))]


def twins(records, chips, states):
    """one submit's records through each kind's twin in turn, each on its own group of the one table; states: per kind, None at first"""
    def only(g):
        return [members if k == g else [] for k, members in enumerate(GROUPS)]

    w = records
    w, _, states["rs41"] = dr.diversity(w, only(0), None, 960, states["rs41"])
    w, _, states["m10"] = ckr.diversity(w, only(1), None, 960, states["m10"])
    w, _, states["mrz"] = ckr.diversity(w, only(2), None, 960, states["mrz"])
    w, _, states["dfm"] = dfr.diversity(w, only(3), None, 960, states["dfm"])
    w, _, states["ims"] = imr.diversity(w, only(4), chips, None, imr.WINDOW, states["ims"])
    return w


@pytest.mark.parametrize("cuts", [1, 2], ids=["1_submit", "2_submits"])
def test_a_table_of_all_five_kinds_gives_each_kinds_twin_on_its_own_group(cuts):
    types, rows = batch_rows()
    iq = torch.from_numpy(rows).to(DEV)
    step = iq.shape[1] // cuts
    b0 = SondeBatch(len(types), step, types=types, flags=_lib.FLAG_IMS_DIVERSITY)
    b = SondeBatch(len(types), step, types=types, flags=_lib.FLAG_IMS_DIVERSITY)
    b.set_diversity(GROUPS)
    states, changed, lonely_failed = dict.fromkeys(KINDS), set(), 0
    for k in range(cuts):
        for x in (b0, b):
            x.submit(iq[:, k * step:(k + 1) * step])
        off, on = _sort(b0.frames()), _sort(b.frames())
        want = twins(off, ims.ring_chips(b0), states)
        assert len(on) == len(want) == len(off), (k, len(on), len(want))
        for a, e, o in zip(on, want, off):
            assert a.tobytes() == e.tobytes(), (k, int(e["channel"]), int(e["bitpos"]), a["nerr"], e["nerr"], hex(int(a["flags"])), hex(int(e["flags"])))
            if a.tobytes() != o.tobytes():
                changed.add(int(a["channel"]))
        lonely_failed += int(((off["channel"] == 10) & (off["nerr"][:, 1] > 0)).sum())
    for g, kind in enumerate(KINDS):
        st = states[kind]
        assert st["combined"][g] >= 1, (kind, st["tried"], st["combined"])
        assert b.diversity_info(g) == {"tried": st["tried"][g], "combined": st["combined"][g]}, kind
    assert {c // 2 for c in changed} == set(range(5)) and 10 not in changed
    assert lonely_failed >= 4                                   # the ungrouped channel's failed frames stay (compared above)
    b0.close()
    b.close()
