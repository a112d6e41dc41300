// dfm_rescue_kernel.hip -- SONDE_FLAG_DFM_RESCUE (DESIGN SPEC 3.3g): the second pass over the DFM06/09/17 frame records of a submit.
// The framer takes every data bit from the first chip of its Manchester pair and decodes Hamming(8,4) with hard decisions: a word
// with two wrong bits is given up (nerr[1]), and the host drops the frame.  The second chip of a pair says which bits are doubtful:
// a pair with two equal chips is an ERASURE, and the extended Hamming code (distance 4) decodes any word with 2v + e <= 3, v unknown
// errors and e erasures.  A frame is rescued iff every word the first pass gave up on decodes that way.
//   the walk over the records is sd_rescue_walk.h's; for a candidate lane i < 33 owns codeword i, reads its byte of the record and
//   the 16 chips of its eight pairs from the channel's bit ring, and decodes it on its own.  No LDS.
// Runs behind whatever wrote the records, on the same stream, and rewrites them in place.  The records of a channel are
// independent of each other (only the two counters are shared), so the result does not depend on the cut into submits.
// Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_rescue_walk.h"

#define DQ_MAX_WORDS 8         // SPEC 3.3g step 3: at most this many failed words
#define DQ_FRAME_CHIPS 560

// the four parity checks of a word (rows 0x78 / 0xB4 / 0xD2 / 0xE1 = bits 3..0), as in sd_dfm_decode_frame
__device__ __forceinline__ uint32_t dq_syndrome(uint32_t w)
{
	return ((uint32_t)__popc(w & 0x78u) & 1u) << 3 | ((uint32_t)__popc(w & 0xB4u) & 1u) << 2 |
	       ((uint32_t)__popc(w & 0xD2u) & 1u) << 1 | ((uint32_t)__popc(w & 0xE1u) & 1u);
}

// SPEC 3.3g step 4 for one word: w as received, E the mask of its erased bits (0x80 >> j: bit j).  Returns the number of bits
// changed and w = the codeword, or -1 (w untouched): e = 0, e > 3, or no codeword within 2v + e <= 3.
// The code is linear: flipping the bits S changes the syndrome by syndrome(S).  So every way of being wrong inside E is one submask
// S of E (at most 8), and what is left of the syndrome must be nothing (v = 0) or, when e = 1 leaves room for v = 1, the column of
// one bit outside E.  Distance 4 makes the answer unique, so the first fit is the only one.
__device__ __forceinline__ int sd_hamming84_erasures(uint32_t &w, uint32_t E)
{
	const int e = __popc(E);
	if (e == 0 || e > 3) return -1;
	// syndrome -> the bit j whose column it is, one nibble each (9: none; the rows above put the weight-3 columns on bits 0..3)
	const unsigned long long col_of = 0x9329199409959678ull;
	for (uint32_t S = E;; S = (S - 1u) & E) {
		const uint32_t t = dq_syndrome(w ^ S);
		uint32_t flips = S;
		bool fit = t == 0u;
		if (!fit && e == 1) {
			const uint32_t j = (uint32_t)(col_of >> (4u * t)) & 15u;
			if (j < 8u && !((0x80u >> j) & E)) { flips |= 0x80u >> j; fit = true; }
		}
		if (fit) { w ^= flips; return __popc(flips); }
		if (S == 0u) return -1;
	}
}

struct DqPass {
	int il_off, il_n, il_i;        // where codeword `lane` lies in the frame (SPEC 3.3b's interleaving): its bit j is frame bit off + j N + i
	static constexpr uint32_t header = SD_H_TYPE | SD_H_LEN | SD_H_NERR1 | SD_H_BITPOS;

	__device__ __forceinline__ DqPass(int lane)
	{
		const int blk = lane < 7 ? 0 : (lane < 20 ? 1 : 2);
		il_off = blk == 0 ? 0 : (blk == 1 ? 56 : 160); il_n = blk == 0 ? 7 : 13;
		il_i = lane - (blk == 0 ? 0 : (blk == 1 ? 7 : 20));
	}

	__device__ __forceinline__ bool candidate(const SdRecHeader &h) const { return h.type == SONDE_DFM09 && h.len == 33 && h.nerr1 >= 1; }

	__device__ __forceinline__ int repair(SondeFrame *fr, const SdRecHeader &h, const SdRescueCtx &ctx) const
	{
		const int lane = ctx.lane;
		// 2. F: the words the first pass left as received
		uint32_t w = 0;
		bool failed = false;
		if (lane < 33) {
			w = fr->data[lane];
			failed = dq_syndrome(w) != 0u;
		}
		const int nf = __popcll(__ballot(failed));
		// 3. the cap, and the frame's chips must still be in the ring (always so for a record of this submit: DESIGN 3.3g)
		if (nf == 0 || nf > DQ_MAX_WORDS) return SD_RESCUE_SKIPPED;
		if (!sd_ring_holds(ctx.ring, h.bitpos, DQ_FRAME_CHIPS)) return SD_RESCUE_SKIPPED;

		// 4. E of this lane's word from its eight pairs, and the decode
		int st = 0;
		if (failed) {
			uint32_t E = 0;
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const uint32_t x = sd_ring_chips32(ctx.ring, h.bitpos + 32u + 2u * (uint32_t)(il_off + j * il_n + il_i));
				if (!((x ^ (x >> 1)) & 1u)) E |= 0x80u >> j;           // the pair's two chips are equal
			}
			st = sd_hamming84_erasures(w, E);
		}
		if (__ballot(st < 0)) return SD_RESCUE_TRIED;               // one word that does not decode: the whole frame stays

		// 5. the record
		if (failed) fr->data[lane] = (uint8_t)w;
		if (lane == 0) {
			fr->nerr[0] += nf;
			fr->nerr[1] = 0;
			fr->flags |= SONDE_FRAME_RESCUED | ((uint32_t)nf << 8);
		}
		return SD_RESCUE_DONE;
	}
};

__global__ __launch_bounds__(64 * SD_RESCUE_WAVES) void sd_dfm_rescue_kernel(SdRescueWalk a)
{
	DqPass pass(threadIdx.x & 63);
	sd_rescue_walk(a, pass);
}

void sd_launch_rescue_dfm(const SdRescueArgs &a) { sd_rescue_launch(sd_dfm_rescue_kernel, a); }

// ---- test introspection: step 4 alone on caller-supplied (word, erasure mask) pairs (sonde_batch_test_hamming84_erasures)
__global__ __launch_bounds__(256) void sd_hamming84_unit_kernel(uint8_t *__restrict__ words, const uint8_t *__restrict__ erased, uint32_t n,
	int32_t *__restrict__ status)
{
	const uint32_t i = 256 * blockIdx.x + threadIdx.x;
	if (i >= n) return;
	uint32_t w = words[i];
	const int st = sd_hamming84_erasures(w, erased[i]);
	words[i] = (uint8_t)w;
	status[i] = st;
}
void sd_launch_hamming84_unit(uint8_t *words, const uint8_t *erased, uint32_t n, int32_t *status, hipStream_t stream)
{
	hipLaunchKernelGGL(sd_hamming84_unit_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, words, erased, n, status);
}
