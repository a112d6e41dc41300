// sd_ims_block.h -- what the two passes over iMS-100 / RS-11G frame records share (ims_rescue_kernel.hip, DESIGN SPEC 3.3h;
// ims_diversity_kernel.hip, SPEC 3.3n): a BCH(46,34) block as received from the chips of a channel's bit ring (SPEC 3.3h step 1), its
// syndromes, what the first pass makes of it (step 2), and the 34 data bits of decoded blocks into a record (step 5).  An iMS-100
// record keeps data bits only, so both passes go back to the chips.  g_exp / g_log: the GF(2^6) table (exp[128], log[64]); the
// callers keep a copy per wave in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_ring.h"

#define IQ_FRAME_CHIPS 1152
#define IQ_BLOCKS 12
#define IQ_BLK_BITS 46
#define IQ_DATA_BITS 34
#define IQ_BLK_MASK ((1ull << IQ_BLK_BITS) - 1ull)

// SPEC 3.3h step 1: block L (0..11) of the frame whose sync begins at chip p, and its boundaries 46 L .. 46 L + 46, from the 94 chips
// p + 47 + 92 L ..; chip j and chip j + 1 are boundary j / 2 of the block for even j, cell (j - 1) / 2 for odd j.  blk: bit b of the
// block = coefficient 45 - b; viol: bit n = boundary n has no transition.  Chip p + 1152 is not used: block 11 has no boundary 46.
// The ring words read lie up to 34 chips behind the frame; their indices are masked, and those chips are not looked at.
__device__ __forceinline__ void iq_rebuild_block(const SdRing &ring, uint64_t p, int L, uint64_t &blk, uint64_t &viol)
{
	const uint64_t c0 = p + 47u + 92u * (uint32_t)L;
	const uint64_t x0 = sd_ring_chips64(ring, c0), x1 = sd_ring_chips64(ring, c0 + 64u);
	const uint64_t eq0 = ~(x0 ^ (x0 >> 1 | x1 << 63)), eq1 = ~(x1 ^ (x1 >> 1));       // bit j: chip j == chip j + 1
	viol = (sd_even_bits64(eq0) | sd_even_bits64(eq1) << 32) & ((2ull << IQ_BLK_BITS) - 1ull);  // bit n: boundary n, 0..46
	const uint64_t cells = sd_even_bits64(eq0 >> 1) | sd_even_bits64(eq1 >> 1) << 32;         // bit b: cell b
	blk = (__builtin_bitreverse64(cells) >> (64 - IQ_BLK_BITS)) & IQ_BLK_MASK;                  // bit b -> coefficient 45 - b
	if (L == IQ_BLOCKS - 1) viol &= IQ_BLK_MASK;
}

// S1 and S3 of a block polynomial over GF(2^6) / x^6 + x + 1 (g64 = exp[128], log[64]), as in sd_ims_decode_frame
__device__ __forceinline__ void iq_syndromes(uint64_t blk, const uint8_t *__restrict__ g_exp, uint32_t &s1, uint32_t &s3)
{
	s1 = 0; s3 = 0;
#pragma unroll
	for (int i = 0; i < IQ_BLK_BITS; i++) {                       // no branch: the look-ups do not wait for each other
		const uint32_t on = 0u - (uint32_t)((blk >> i) & 1ull);
		s1 ^= g_exp[i] & on; s3 ^= g_exp[(3 * i) % 63] & on;
	}
}

// SPEC 3.3h step 2: what does the first pass make of a block with these syndromes?  Its rule restated: nothing to do; a single error
// iff S3 = S1^3, at a position < 46; otherwise the two roots of x^2 + S1 x + (S3 + S1^3) / S1, both < 46; otherwise rejected.
// Returns true if it rejects the block; WANT_E: else e = the coefficients it turns (the block becomes the codeword blk ^ e).
template <bool WANT_E> __device__ __forceinline__ bool iq_first_pass(uint32_t s1, uint32_t s3, const uint8_t *__restrict__ g_exp,
	const uint8_t *__restrict__ g_log, uint64_t &e)
{
	if (WANT_E) e = 0;
	if (!s1 && !s3) return false;
	if (!s1) return true;
	const uint32_t l1 = g_log[s1], s1c = g_exp[(3u * l1) % 63u];
	if (s3 == s1c) {
		if (WANT_E) e = 1ull << l1;
		return l1 >= IQ_BLK_BITS;
	}
	const uint32_t prod = g_exp[g_log[s3 ^ s1c] + 63u - l1];
	int found = 0, inside = 0;
#pragma unroll 9
	for (uint32_t i = 0; i < 63u; i++) {
		const bool root = (g_exp[(2u * i) % 63u] ^ g_exp[l1 + i] ^ prod) == 0u;
		found += root; inside += root && i < IQ_BLK_BITS;
		if (WANT_E && root) e |= 1ull << i;
	}
	return !(found == 2 && inside == 2);
}
__device__ __forceinline__ bool iq_first_pass_rejects(uint32_t s1, uint32_t s3, const uint8_t *__restrict__ g_exp, const uint8_t *__restrict__ g_log)
{
	uint64_t e;
	return iq_first_pass<false>(s1, s3, g_exp, g_log, e);
}

// a 64-bit value of lane src (per lane)
__device__ __forceinline__ uint64_t iq_shfl64(uint64_t v, int src)
{
	return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src, 64) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64) << 32);
}

// SPEC 3.3h step 5: the data bits of the decoded blocks into the record.  fm: the blocks to write (wave-uniform), dec: lane L < 12
// holds block L.  Lane i < 51 owns byte i; data bit k is bit k % 34 of block k / 34, and a byte lies in at most two blocks.  All 64
// lanes call.
__device__ __forceinline__ void iq_write_blocks(SondeFrame *fr, unsigned long long fm, uint64_t dec, int lane)
{
	const int La = (8 * lane) / IQ_DATA_BITS, Lb = (8 * lane + 7) / IQ_DATA_BITS;       // lanes >= 51: a lane of its own, unused
	const uint64_t da = iq_shfl64(dec, La & 63), db = iq_shfl64(dec, Lb & 63);
	if (lane < 51) {
		const uint32_t old = fr->data[lane];
		uint32_t nb = old;
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const int k = 8 * lane + j, L = k / IQ_DATA_BITS, b = k % IQ_DATA_BITS;
			if ((fm >> L) & 1ull) {
				const uint32_t bit = (uint32_t)(((L == La ? da : db) >> (IQ_BLK_BITS - 1 - b)) & 1ull);
				nb = (nb & ~(0x80u >> j)) | (bit << (7 - j));
			}
		}
		if (nb != old) fr->data[lane] = (uint8_t)nb;
	}
}
