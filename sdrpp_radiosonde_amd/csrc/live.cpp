// live.cpp -- the matching rule of the live receiver (DESIGN SPEC 3.12): pure host, integers only, exactly reproducible.
#include <stdint.h>
#include <stdlib.h>
#include "sd_host.h"
#include "../../include/sonde_abi.h"

// Each candidate goes to the nearest VFO no further than match_hz away (a tie: the lower VFO index); a VFO keeps only the nearest of
// the candidates that went to it (a tie: the lower candidate index); the others stay unmatched.
extern "C" int sonde_live_match(const int32_t *vfo_offsets, uint32_t n_vfos, const int32_t *cand_offsets, uint32_t n_cand, uint32_t match_hz,
	int32_t *cand_of_vfo, int32_t *vfo_of_cand)
{
	if ((n_vfos && (!vfo_offsets || !cand_of_vfo)) || (n_cand && (!cand_offsets || !vfo_of_cand))) return sd_fail_msg("sonde_live_match: null argument");
	const int64_t reach = match_hz ? match_hz : 10000;
	for (uint32_t v = 0; v < n_vfos; v++) cand_of_vfo[v] = -1;
	for (uint32_t c = 0; c < n_cand; c++) {
		vfo_of_cand[c] = -1;
		int64_t best = reach + 1;
		int32_t to = -1;
		for (uint32_t v = 0; v < n_vfos; v++) {
			const int64_t d = llabs((int64_t)cand_offsets[c] - (int64_t)vfo_offsets[v]);
			if (d < best) { best = d; to = (int32_t)v; }
		}
		if (to < 0) continue;
		const int32_t held = cand_of_vfo[to];
		if (held >= 0 && llabs((int64_t)cand_offsets[held] - (int64_t)vfo_offsets[to]) <= best) continue;
		if (held >= 0) vfo_of_cand[held] = -1;
		cand_of_vfo[to] = (int32_t)c;
		vfo_of_cand[c] = to;
	}
	return 0;
}
