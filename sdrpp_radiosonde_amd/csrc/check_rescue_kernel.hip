// check_rescue_kernel.hip -- SONDE_FLAG_MANCHESTER_RESCUE (DESIGN SPEC 3.3f): the second pass over the M10 / M20 and MRZ-N1 frame
// records of a submit.  These frames carry a 16-bit check and no FEC, but every data bit is a Manchester chip pair (a, !a): a pair
// with two equal chips marks a bit that may be wrong.  A frame whose check fails with 1..8 such pairs is a linear system over GF(2)
// -- 16 equations (the syndrome), one unknown per marked bit, the column of a bit being the change of the syndrome when it flips --
// and is rescued iff exactly one subset of the marked bits explains the syndrome.
//   the walk over the records is sd_rescue_walk.h's; for a candidate lane i reads 32 chips of the frame from the channel's bit ring
//   (16 pairs), the marked bits are gathered into lanes 0..7, and the <= 255 subsets are tried across the wave, four per lane.  No LDS.
// Runs behind whatever wrote the records, on the same stream, and rewrites them in place.  The records of a channel are
// independent of each other (only the two counters are shared), so the result does not depend on the cut into submits.
// Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_check_cols.h"
#include "sd_rescue_walk.h"

struct MqPass {
	const uint16_t *m10tab /* [99][8] */, *mrztab /* [43][8] */;
	static constexpr uint32_t header = SD_H_TYPE | SD_H_LEN | SD_H_NERR0 | SD_H_NERR1 | SD_H_BITPOS;

	__device__ __forceinline__ bool candidate(const SdRecHeader &h) const
	{
		const bool known = (h.type == SONDE_M10 && (h.len == 101 || h.len == 70)) || (h.type == SONDE_MRZN1 && h.len == 45);
		// nerr[1] is |V| (sd_fixed.h counts the same pairs): 0 or more than 8 of them never reach the solver
		return known && h.nerr0 == -1 && h.nerr1 >= 1 && h.nerr1 <= MQ_MAX_HINTS;
	}

	__device__ __forceinline__ int repair(SondeFrame *fr, const SdRecHeader &h, const SdRescueCtx &ctx) const
	{
		const int lane = ctx.lane, len = h.len, nbits = 8 * len;
		const bool mrz = h.type == SONDE_MRZN1;
		const uint32_t lead = mrz ? 48u : 32u;                    // chips in front of the first data chip
		// 2. the frame's chips must still be in the ring (always so for a record of this submit: DESIGN 3.3f)
		if (!sd_ring_holds(ctx.ring, h.bitpos, lead + 2ull * (uint64_t)nbits)) return SD_RESCUE_SKIPPED;

		// 1. V: lane i looks at the 16 pairs of frame bits 16 i .. 16 i + 15
		uint32_t vm = 0;
		if (16 * lane < nbits) {
			const uint32_t x = sd_ring_chips32(ctx.ring, h.bitpos + lead + 32ull * (uint64_t)lane);
			const uint32_t v = sd_even_bits32(~(x ^ (x >> 1)));    // bit q: the two chips of pair q are equal
			const int left = nbits - 16 * lane;
			vm = left >= 16 ? v : (v & ((1u << left) - 1u));
		}
		int nv = __popc(vm);
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off, 64);
		if (nv == 0 || nv > MQ_MAX_HINTS) return SD_RESCUE_SKIPPED;
		if (!mrz && (__builtin_amdgcn_readfirstlane((int)vm) & 0xFF)) return SD_RESCUE_SKIPPED;      // M10 / M20: the length byte decides the layout
		const int myk = mq_gather<16>(vm, lane);                  // the marked bits, ascending, into lanes 0 .. nv - 1

		// 3. syndrome of the frame as recorded (bytes lane and lane + 64) and the column of this lane's marked bit
		const uint16_t *tab = mrz ? mrztab : m10tab;
		const int n_cov = len - 2;
		const bool hi_first = !mrz;
		uint32_t s = 0;
#pragma unroll
		for (int r = 0; r < 2; r++) {
			const int i = lane + 64 * r;
			if (i < len) s ^= mq_byte_syndrome(mq_row(tab, n_cov, hi_first, i), fr->data[i]);
		}
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) s ^= (uint32_t)__shfl_xor((int)s, off, 64);
		if (mrz) s ^= mq_mrz_crc_of_zeros();
		uint32_t col = 0;
		if (lane < nv) col = mq_col(mq_row(tab, n_cov, hi_first, myk >> 3), 7 - (myk & 7));

		// 4. the subsets m = 1 .. 2^nv - 1 of the marked bits (bit j of m: lane j's), four per lane
		uint32_t U = 0;
		if (mq_solve(col, nv, s, lane, U) != 1) return SD_RESCUE_TRIED;      // none, or several: the frame stays

		// 5. the record: every lane flips what falls into its two bytes
#pragma unroll
		for (int r = 0; r < 2; r++) {
			const int i = lane + 64 * r;
			const uint32_t fm = mq_flips<1>(U, myk, i);
			if (fm) fr->data[i] = (uint8_t)(fr->data[i] ^ fm);
		}
		if (lane == 0) {
			fr->nerr[0] = 0;
			fr->flags |= SONDE_FRAME_RESCUED | ((uint32_t)__popc(U) << 8);
		}
		return SD_RESCUE_DONE;
	}
};

__global__ __launch_bounds__(64 * SD_RESCUE_WAVES) void sd_manchester_rescue_kernel(SdRescueWalk a, const uint16_t *__restrict__ m10tab,
	const uint16_t *__restrict__ mrztab)
{
	MqPass pass = { m10tab, mrztab };
	sd_rescue_walk(a, pass);
}

void sd_launch_rescue_manchester(const SdRescueArgs &a) { sd_rescue_launch(sd_manchester_rescue_kernel, a, a.fec.m10tab, a.mrztab); }
