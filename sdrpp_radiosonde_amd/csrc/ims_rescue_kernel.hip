// ims_rescue_kernel.hip -- SONDE_FLAG_IMS_RESCUE (DESIGN SPEC 3.3h): the second pass over the iMS-100 / RS-11G frame records of a submit.
// Biphase-S carries the bit in whether the two chips of a cell are equal, and makes a transition at every cell boundary.  The framer
// never looks at the boundaries: a boundary WITHOUT a transition says that one of its two chips is wrong, so one of the two bits next
// to it is.  A block of BCH(46,34) the first pass rejected (three or more wrong bits) with 1..6 such boundaries is decoded by trying
// the 2^m ways of blaming the left or the right cell of each; the block decodes iff exactly one distinct flip pattern is a codeword.
// A frame is rescued iff every rejected block decodes.
//   the walk over the records is sd_rescue_walk.h's; for a candidate lanes 0..11 rebuild their block, its boundaries and the first
//   pass's verdict from the chips of the channel's bit ring (sd_ims_block.h, shared with ims_diversity_kernel.hip); then, rejected block by rejected block, the 64 lanes are the up to 64
//   hypotheses.  LDS: each wave's own copy of the 192-byte GF(2^6) table (its look-ups are the kernel's critical path: read from
//   global memory they added 25 us to the step of profiles/ims_rescue_notes.md).
// Runs behind whatever wrote the records, on the same stream, and rewrites them in place.  The records of a channel are
// independent of each other (only the two counters are shared), so the result does not depend on the cut into submits.
// Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_rescue_walk.h"
#include "sd_ims_block.h"

#define IQ_CAP 6               // SPEC 3.3h step 3: at most this many violated boundaries per block

// SPEC 3.3h step 3 for one block, by the whole wave: blk as received (bit b of the block = coefficient 45 - b), its syndromes, viol
// = the mask of its violated boundaries (bit k: boundary k of the block, 0..46); all wave-uniform.  Lane h is hypothesis h: bit j of
// h picks, for the j-th violated boundary v, the cell v (1) or v - 1 (0); a pick outside 0..45 flips nothing, a cell picked twice
// cancels (XOR).  Returns true and e = the one distinct flip pattern that makes both syndromes zero, or false.
__device__ __forceinline__ bool iq_decode_block(uint32_t s1, uint32_t s3, uint64_t viol, const uint8_t *__restrict__ g_exp, int lane, uint64_t &e)
{
	const int m = __popcll(viol);
	if (m == 0 || m > IQ_CAP) return false;
	uint64_t pat = 0, v = viol;
#pragma unroll
	for (int j = 0; j < IQ_CAP; j++) {
		if (!v) break;
		const int cell = __builtin_ctzll(v) - 1 + ((lane >> j) & 1);
		v &= v - 1ull;
		if (cell >= 0 && cell < IQ_BLK_BITS) {
			const int i = IQ_BLK_BITS - 1 - cell;
			pat ^= 1ull << i;
			s1 ^= g_exp[i]; s3 ^= g_exp[(3 * i) % 63];
		}
	}
	const bool fit = lane < (1 << m) && s1 == 0u && s3 == 0u;
	const unsigned long long fm = __ballot(fit);
	if (!fm) return false;
	e = sd_readlane64(pat, __builtin_ctzll(fm));
	return __ballot(fit && pat != e) == 0ull;                    // several distinct patterns fit: no decode
}

struct IqPass {
	const uint8_t *g_exp, *g_log;          // the wave's own copy of the table in LDS
	static constexpr uint32_t header = SD_H_TYPE | SD_H_LEN | SD_H_NERR1 | SD_H_BITPOS;

	__device__ __forceinline__ bool candidate(const SdRecHeader &h) const { return h.type == SONDE_IMS100 && h.len == 51 && h.nerr1 >= 1; }

	__device__ __forceinline__ int repair(SondeFrame *fr, const SdRecHeader &h, const SdRescueCtx &ctx) const
	{
		const int lane = ctx.lane;
		// the frame's chips must still be in the ring (always so for a record of this submit: DESIGN 3.3h)
		if (!sd_ring_holds(ctx.ring, h.bitpos, IQ_FRAME_CHIPS)) return SD_RESCUE_SKIPPED;

		// 1. lane L < 12: block L and its boundaries 46 L .. 46 L + 46 (sd_ims_block.h)
		uint64_t blk = 0, viol = 0;
		uint32_t s1 = 0, s3 = 0;
		bool failed = false;
		if (lane < IQ_BLOCKS) {
			iq_rebuild_block(ctx.ring, h.bitpos, lane, blk, viol);
			// 2. F: the blocks the first pass rejects
			iq_syndromes(blk, g_exp, s1, s3);
			failed = iq_first_pass_rejects(s1, s3, g_exp, g_log);
		}
		const unsigned long long fm = __ballot(failed);
		const int nf = __popcll(fm);
		if (nf != h.nerr1) return SD_RESCUE_SKIPPED;                // record and ring disagree

		// 3. each failed block on its own, the lanes as its hypotheses; 4. one block that does not decode: the whole frame stays
		uint64_t dec = blk;
		int flips = 0;
		for (unsigned long long m = fm; m; m &= m - 1ull) {
			const int L = __builtin_ctzll(m);
			uint64_t e = 0;
			if (!iq_decode_block((uint32_t)__builtin_amdgcn_readlane((int)s1, L), (uint32_t)__builtin_amdgcn_readlane((int)s3, L),
			                     sd_readlane64(viol, L), g_exp, lane, e)) return SD_RESCUE_TRIED;
			if (lane == L) dec ^= e;
			flips += __popcll(e);
		}

		// 5. the record
		iq_write_blocks(fr, fm, dec, lane);
		if (lane == 0) {
			fr->nerr[0] += flips;
			fr->nerr[1] = 0;
			fr->flags |= SONDE_FRAME_RESCUED | ((uint32_t)nf << 8);
		}
		return SD_RESCUE_DONE;
	}
};

__global__ __launch_bounds__(64 * SD_RESCUE_WAVES) void sd_ims_rescue_kernel(SdRescueWalk a, const uint8_t *__restrict__ g64)
{
	// the wave's own copy of the table (exp[128], log[64]); wave-private, so a fence and a wave barrier order it, as in sd_fixed.h
	__shared__ uint32_t s_g64[SD_RESCUE_WAVES][48];
	const int lane = threadIdx.x & 63;
	uint32_t *const tab = s_g64[threadIdx.x >> 6];
	if (lane < 48) tab[lane] = reinterpret_cast<const uint32_t *>(g64)[lane];
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	__builtin_amdgcn_wave_barrier();
	IqPass pass = { reinterpret_cast<const uint8_t *>(tab), reinterpret_cast<const uint8_t *>(tab) + 128 };
	sd_rescue_walk(a, pass);
}

void sd_launch_rescue_ims(const SdRescueArgs &a) { sd_rescue_launch(sd_ims_rescue_kernel, a, a.fec.g64); }

// ---- test introspection: step 3 alone on caller-supplied (block, violation mask) pairs (sonde_batch_test_ims_block); one wave per
// pair, IQ_UNIT_PAIRS pairs per wave
#define IQ_UNIT_PAIRS 16
__global__ __launch_bounds__(64 * SD_RESCUE_WAVES) void sd_ims_block_unit_kernel(const uint8_t *__restrict__ g64, uint64_t *__restrict__ blocks,
	const uint64_t *__restrict__ viols, uint32_t n, int32_t *__restrict__ status)
{
	const int lane = threadIdx.x & 63;
	const uint32_t first = IQ_UNIT_PAIRS * (SD_RESCUE_WAVES * blockIdx.x + (threadIdx.x >> 6));
	for (uint32_t k = 0; k < IQ_UNIT_PAIRS; k++) {
		const uint32_t i = first + k;
		if (i >= n) return;
		const uint64_t blk = sd_readlane64(blocks[i], 0) & IQ_BLK_MASK, viol = sd_readlane64(viols[i], 0) & ((1ull << (IQ_BLK_BITS + 1)) - 1ull);
		uint32_t s1, s3;
		iq_syndromes(blk, g64, s1, s3);
		uint64_t e = 0;
		const bool ok = iq_decode_block((uint32_t)__builtin_amdgcn_readfirstlane((int)s1), (uint32_t)__builtin_amdgcn_readfirstlane((int)s3), viol, g64, lane, e);
		if (lane == 0) {
			if (ok) blocks[i] = blk ^ e;
			status[i] = ok ? __popcll(e) : -1;
		}
	}
}
void sd_launch_ims_block_unit(const uint8_t *g64, uint64_t *blocks, const uint64_t *viols, uint32_t n, int32_t *status, hipStream_t stream)
{
	const uint32_t per_wg = SD_RESCUE_WAVES * IQ_UNIT_PAIRS;
	hipLaunchKernelGGL(sd_ims_block_unit_kernel, dim3((n + per_wg - 1) / per_wg), dim3(64 * SD_RESCUE_WAVES), 0, stream, g64, blocks, viols, n, status);
}
