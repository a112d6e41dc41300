"""The live receiver's matching rule, written a second time in plain Python (DESIGN SPEC 3.12), and the scripts' helpers.  The rule:
each candidate goes to the nearest VFO no further than match_hz away (a tie: the lower VFO index); a VFO keeps only the nearest of
the candidates that went to it (a tie: the lower candidate index).  Integers only: exactly reproducible."""
from __future__ import annotations

MATCH_HZ = 10000


def match_ref(vfos, cands, match_hz=0):
    reach = match_hz or MATCH_HZ
    to = []
    for c in cands:
        d = [abs(int(c) - int(v)) for v in vfos]
        ok = [k for k in range(len(vfos)) if d[k] <= reach]
        to.append(min(ok, key=lambda k: (d[k], k)) if ok else -1)
    cand_of_vfo = []
    for k, v in enumerate(vfos):
        mine = [i for i in range(len(cands)) if to[i] == k]
        cand_of_vfo.append(min(mine, key=lambda i: (abs(int(cands[i]) - int(v)), i)) if mine else -1)
    vfo_of_cand = [to[i] if to[i] >= 0 and cand_of_vfo[to[i]] == i else -1 for i in range(len(cands))]
    return cand_of_vfo, vfo_of_cand
