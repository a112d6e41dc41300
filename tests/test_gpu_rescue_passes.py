"""-m gpu: the five rescue passes side by side in one batch (DESIGN "what a rescue pass plugs into"): sonde_batch_restart_channels
clears the state of every pass at once.  The 12-channel mixed batch of test_gpu_afsk_rescue.py with all five flags, in two submits;
channels 0..5 (one of each kind) are restarted: each reports counters zero (RS41: no layout) afterwards, channels 6..11 report what
they did before, and every info method still refuses a channel of another kind."""
import numpy as np
import pytest
import torch

import afsk_rescue_scenes as sc
import dfm_rescue_scenes as ds
import ims_rescue_scenes as ims
import manchester_rescue_scenes as ms
import rescue_scenes as rs
from sdrpp_radiosonde_amd import _lib
from sdrpp_radiosonde_amd.batch import SondeBatch, SondeError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# sonde type -> the info method of the pass that follows it
INFO = {0: "rescue_info", 1: "dfm_rescue_info", 2: "ims_rescue_info", 3: "manchester_rescue_info", 4: "afsk_rescue_info", 5: "afsk_rescue_info"}


def _all_info(b, types):
    """every channel's counters from its own pass; the other four methods must refuse the channel"""
    out = []
    for c, t in enumerate(types):
        for method in sorted(set(INFO.values())):
            if method == INFO[int(t)]:
                out.append(getattr(b, method)(c))
            else:
                with pytest.raises(SondeError):
                    getattr(b, method)(c)
    return out


def test_restart_clears_every_pass_of_the_listed_channels_only():
    n = sc.TILE * 96
    rs41, m10, dfm, im = (torch.from_numpy(x).to(DEV)[:, :n] for x in (rs.scene().iq, ms.scene("m10").iq, ds.scene().iq, ims.scene_of("designed").iq))
    imet, c50 = (torch.from_numpy(sc.scene_of(k).iq).to(DEV) for k in ("imet", "c50"))
    assert all(x.shape[1] == n for x in (rs41, m10, dfm, im, imet, c50))
    iq = torch.stack([rs41[0], imet[0], m10[0], dfm[0], c50[0], im[0], imet[2], rs41[7], c50[1], dfm[3], m10[3], im[3]]).contiguous()
    types = np.array([0, 4, 3, 1, 5, 2, 4, 0, 5, 1, 3, 2], dtype=np.uint8)
    restart = list(range(6))
    assert sorted(types[restart]) == [0, 1, 2, 3, 4, 5]
    b = SondeBatch(len(types), n // 2, types=types, flags=_lib.rescue_flags(True, True, True, True, True))
    for k in range(2):
        b.submit(iq[:, k * (n // 2):(k + 1) * (n // 2)])
    before = _all_info(b, types)
    assert all(before[c]["tried"] >= 1 for c in restart), before
    assert any(before[c]["layouts"][320] or before[c]["layouts"][518] for c in restart if types[c] == 0)
    b.restart_channels(restart)
    torch.cuda.synchronize()
    after = _all_info(b, types)
    for c in restart:
        want = {"tried": 0, "rescued": 0}
        if types[c] == 0:
            want["layouts"] = {320: [], 518: []}
        assert after[c] == want, c
    assert after[6:] == before[6:]
    b.close()
