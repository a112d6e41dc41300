// sd_div_copies.h -- what the combining passes "by check" share (check_diversity_kernel.hip, SPEC 3.3l: M10 / M20 / MRZ-N1;
// afsk_diversity_kernel.hip, SPEC 3.3o: iMet and SRS-C50): the copies of a frame as one 32-bit word per lane, step 3 -- the working
// frame (bitwise majority, copy 0's bit where there is none) and the bits on which the copies differ -- and step 6, the accepted
// result into the record.  Wave-synchronous, all 64 lanes active, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_diversity_scan.h"

// word `lane` of a record's data, zero behind the frame's last word
__device__ __forceinline__ uint32_t cd_word(const SondeFrame *f, int len, int lane)
{
	return 4 * lane < len ? reinterpret_cast<const uint32_t *>(f->data)[lane] : 0u;
}
// the bytes of word `lane` that belong to a frame of len bytes
__device__ __forceinline__ uint32_t cd_mask(int len, int lane)
{
	const int rem = len - 4 * lane;
	return rem >= 4 ? 0xFFFFFFFFu : rem > 0 ? (1u << (8 * rem)) - 1u : 0u;
}

// Step 3 on K copies of a frame of len bytes; c[j]: this lane's word of copy j (c[j] for j >= K is not looked at).  w = this lane's
// word of the working frame (frame bytes only), vm = this lane's unknowns (frame bit k = 32 lane + q is bit 7 - q % 8 of byte q / 8
// of the word: bit q of vm), nv = |V| over the wave
__device__ __forceinline__ void cd_majority(int len, int K, const uint32_t (&c)[SD_DIV_MAX], int lane, uint32_t &w, uint32_t &vm, int &nv)
{
	const uint32_t bm = cd_mask(len, lane);
	const uint32_t x0 = c[0] & bm, x1 = c[1] & bm, x2 = (K > 2 ? c[2] : c[0]) & bm, x3 = (K > 3 ? c[3] : c[0]) & bm;
	const uint32_t diff = (x0 ^ x1) | (x0 ^ x2) | (x0 ^ x3);
	if (K == 2) w = x0;
	else if (K == 3) w = (x0 & x1) | (x0 & x2) | (x1 & x2);
	else {      // four copies: three alike decide, two against two leave copy 0's bit
		const uint32_t ones = (x0 & x1 & x2) | (x0 & x1 & x3) | (x0 & x2 & x3) | (x1 & x2 & x3);
		const uint32_t zeros = (~x0 & ~x1 & ~x2) | (~x0 & ~x1 & ~x3) | (~x0 & ~x2 & ~x3) | (~x1 & ~x2 & ~x3);
		w = ones | (x0 & ~zeros);
	}
	vm = __brev(__builtin_bswap32(diff));
	nv = __popc(vm);
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off, 64);
}

// Step 6: the accepted result into the record; data behind len stays (c0: this lane's word of the record as it stands)
__device__ __forceinline__ void cd_write_record(SondeFrame *fr, int len, int K, int nv, uint32_t w, uint32_t c0, int lane)
{
	const uint32_t bm = cd_mask(len, lane);
	if (bm) reinterpret_cast<uint32_t *>(fr->data)[lane] = (w & bm) | (c0 & ~bm);
	if (lane == 0) {
		fr->nerr[0] = 0;
		fr->flags = dv_load_fresh(&fr->flags) | SONDE_FRAME_RESCUED | SONDE_FRAME_COMBINED | ((uint32_t)K << 8) | ((uint32_t)min(nv, 15) << 12);
	}
}
