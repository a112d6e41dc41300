// afsk_rescue_kernel.hip -- SONDE_FLAG_AFSK_RESCUE (DESIGN SPEC 3.3i): the second pass over the iMet-1/4 and SRS-C50 packet records of a
// submit.  These packets carry a 16-bit check and nothing else: no FEC, no second chip per bit.  A packet whose check fails is
// searched for ONE wrong bit, or TWO NEIGHBOURING wrong bits of one character (15 patterns per candidate byte), and is rescued iff
// exactly one pattern makes the check pass.
//   iMet: CRC16-CCITT is affine over GF(2).  The syndrome (computed CRC XOR stored CRC) is the XOR of the columns of the wrong bits,
//   the column of a bit being the change of the syndrome when it flips: x^(16 + 8 k + j) mod 0x11021 for bit j of the byte with k
//   covered bytes behind it, bit 8 + j / bit j of the syndrome itself for the two stored bytes.  Lane i owns byte i of the packet
//   (at most 64), XORs the columns of its set bits into the wave's syndrome and compares its 15 patterns with it.
//   C50: the two running byte sums are not linear over GF(2); lanes 2..8 recompute them over data XOR each of their 15 patterns.
//   The walk over the records is sd_rescue_walk.h's.  No LDS, no table in memory.
// Runs behind sd_imet_kernel / sd_c50_kernel, on the same stream, and rewrites the records in place.  It reads the records only (not
// the bit ring), and the records of a channel are independent of each other (only the two counters are shared), so the result
// does not depend on the cut into submits.  Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_rescue_walk.h"
#include "sd_ccitt_cols.h"      // AQ_IMET_MAXLEN, aq_pow, aq_imet_cols: the CRC-CCITT columns, shared with afsk_diversity_kernel.hip

#define AQ_C50_LEN 9

// pattern q = 0 .. 14 of SPEC 3.3i step 3: the single-bit masks 1 << q, then the adjacent-pair masks 3 << (q - 8)
__device__ __forceinline__ uint32_t aq_pattern(int q) { return q < 8 ? 1u << q : 3u << (q - 8); }

// SPEC 3.3i step 1: the records the pass works on -- a packet of a known shape whose check failed
__device__ __forceinline__ bool aq_imet(uint32_t type, int len) { return type == SONDE_IMET4 && len >= 5 && len <= AQ_IMET_MAXLEN; }
__device__ __forceinline__ bool aq_eligible(uint32_t type, int len, int nerr0)
{
	return (aq_imet(type, len) || (type == SONDE_C50 && len == AQ_C50_LEN)) && nerr0 == -1;
}

// Steps 1..5 of SPEC 3.3i for ONE record, by a whole wave (type, len, nerr0: the record's header, wave-uniform).
// Returns -1: not eligible; 0: no pattern fits; 1: rescued (the record is rewritten); 2: several patterns fit.
__device__ __forceinline__ int aq_repair(SondeFrame *__restrict__ fr, uint32_t type, int len, int nerr0, int lane)
{
	if (!aq_eligible(type, len, nerr0)) return -1;
	const bool imet = aq_imet(type, len);
	const uint32_t d = lane < len ? fr->data[lane] : 0u;
	int first = 2;
	uint32_t fit = 0;                       // bit q: pattern q of this lane's byte fits
	if (imet) {
		if ((uint32_t)__builtin_amdgcn_readlane((int)d, 1) == 3u) first = 3;     // XDATA: byte 2 decided len
		// the start value 0x1D0F is an XOR into the first two bytes; columns of the covered bytes from the table, of the stored
		// CRC (big-endian) the syndrome's own bits
		const int n_cov = len - 2;
		uint32_t c0 = 0;
		if (lane < n_cov) c0 = aq_pow.v[n_cov - 1 - lane];
		else if (lane < len) c0 = lane == n_cov ? 0x100u : 0x1u;
		uint32_t s = aq_imet_cols(c0, d ^ (lane == 0 ? 0x1Du : (lane == 1 ? 0x0Fu : 0u)));
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) s ^= (uint32_t)__shfl_xor((int)s, off, 64);
		if (lane >= first && lane < len) {
#pragma unroll
			for (int q = 0; q < 15; q++) if (aq_imet_cols(c0, aq_pattern(q)) == s) fit |= 1u << q;
		}
	} else {
		uint32_t b[AQ_C50_LEN];
#pragma unroll
		for (int i = 0; i < AQ_C50_LEN; i++) b[i] = (uint32_t)__builtin_amdgcn_readlane((int)d, i);
		if (lane >= first && lane < len) {
			for (int q = 0; q < 15; q++) {
				const uint32_t m = aq_pattern(q);
				uint32_t c1 = 0, c2 = 0;
#pragma unroll
				for (int i = 2; i < 7; i++) { c1 = (c1 + (b[i] ^ (i == lane ? m : 0u))) & 0xFFu; c2 = (c2 + c1) & 0xFFu; }
				if (c1 == (b[7] ^ (lane == 7 ? m : 0u)) && c2 == (b[8] ^ (lane == 8 ? m : 0u))) fit |= 1u << q;
			}
		}
	}
	int nfit = __popc(fit);
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) nfit += __shfl_xor(nfit, off, 64);
	if (nfit != 1) return nfit ? 2 : 0;     // none, or several: the record stays
	const unsigned long long who = __ballot(fit != 0u);
	const uint32_t m = aq_pattern(__builtin_ctz(fit | 0x8000u));
	if (fit) fr->data[lane] = (uint8_t)(d ^ m);
	const uint32_t w = (uint32_t)__popc((uint32_t)__builtin_amdgcn_readlane((int)m, __builtin_ctzll(who)));
	if (lane == 0) {
		fr->nerr[0] = 0;
		fr->flags |= SONDE_FRAME_RESCUED | (w << 8);
	}
	return 1;
}

struct AqPass {
	static constexpr uint32_t header = SD_H_TYPE | SD_H_LEN | SD_H_NERR0;          // no bitpos: the pass reads no ring
	__device__ __forceinline__ bool candidate(const SdRecHeader &h) const { return aq_eligible(h.type, h.len, h.nerr0); }
	__device__ __forceinline__ int repair(SondeFrame *fr, const SdRecHeader &h, const SdRescueCtx &ctx) const
	{
		const int r = aq_repair(fr, h.type, h.len, h.nerr0, ctx.lane);
		return r < 0 ? SD_RESCUE_SKIPPED : r == 1 ? SD_RESCUE_DONE : SD_RESCUE_TRIED;
	}
};

__global__ __launch_bounds__(64 * SD_RESCUE_WAVES) void sd_afsk_rescue_kernel(SdRescueWalk a)
{
	AqPass pass;
	sd_rescue_walk(a, pass);
}

void sd_launch_rescue_afsk(const SdRescueArgs &a) { sd_rescue_launch(sd_afsk_rescue_kernel, a); }

// ---- aq_repair alone over n caller-made records, one wave each (sonde_batch_test_afsk_repair): status 0 untouched, 1 rescued,
// 2 several patterns fit
__global__ __launch_bounds__(64 * SD_RESCUE_WAVES) void sd_afsk_repair_unit_kernel(SondeFrame *__restrict__ records, uint32_t n, int32_t *__restrict__ status)
{
	const int lane = threadIdx.x & 63;
	const uint32_t i = SD_RESCUE_WAVES * blockIdx.x + (threadIdx.x >> 6);
	if (i >= n) return;
	SondeFrame *fr = records + i;
	const uint32_t type = (uint32_t)__builtin_amdgcn_readfirstlane((int)fr->type);
	const int len = __builtin_amdgcn_readfirstlane(fr->len), nerr0 = __builtin_amdgcn_readfirstlane(fr->nerr[0]);
	const int r = aq_repair(fr, type, len, nerr0, lane);
	if (lane == 0) status[i] = r < 0 ? 0 : r;
}
void sd_launch_afsk_repair_unit(SondeFrame *records, uint32_t n, int32_t *status, hipStream_t stream)
{
	hipLaunchKernelGGL(sd_afsk_repair_unit_kernel, dim3((n + SD_RESCUE_WAVES - 1) / SD_RESCUE_WAVES), dim3(64 * SD_RESCUE_WAVES), 0, stream, records, n, status);
}
