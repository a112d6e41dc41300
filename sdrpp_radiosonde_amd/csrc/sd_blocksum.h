// sd_blocksum.h -- THE summation order of the carrier meter (DESIGN SPEC 3.11), which the antenna combiner's statistics share (SPEC
// 3.14): NQ sums of per-sample float32 products over a span of 256-sample blocks, by one 256-lane workgroup.  Wave w takes the span's
// blocks w, w + 4, ...; lane l the samples l, l + 64, l + 128, l + 192 of the block, the four products added in ascending order, then
// a fixed xor butterfly over the 64 lanes.  The block sums go through LDS, SD_BS_CHUNK blocks at a time; lane q < NQ adds those of
// quantity q to a double in ascending block order.  A sum therefore depends on the samples and on where its span starts alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SD_BS_WG     256                // lanes of the workgroup: four waves
#define SD_BS_BLK    256                // samples per block
#define SD_BS_CHUNK  32                 // blocks per trip through LDS (8 per wave)

// Blocks [b0, b1).  fetch(m): what sample m (counted from block 0's first) is made of; prod(v, p): its NQ products into p, each rounded
// once (one explicit fmaf).  They are two, so that a lane's four fetches are in flight before its first product.  acc: what lane
// q < NQ starts from; returns what it ends with (other lanes: acc).  Every lane of the workgroup calls it.
template <int NQ, class Fetch, class Prod>
__device__ __forceinline__ double sd_blocksum(uint32_t b0, uint32_t b1, double acc, float (&s_bs)[NQ][SD_BS_CHUNK], Fetch fetch, Prod prod)
{
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	for (uint32_t c0 = b0; c0 < b1; c0 += SD_BS_CHUNK) {
		const uint32_t cn = min((uint32_t)SD_BS_CHUNK, b1 - c0);
		for (uint32_t q = wave; q < cn; q += SD_BS_WG / 64) {
			const int64_t m0 = (int64_t)(c0 + q) * SD_BS_BLK + lane;
			decltype(fetch(m0)) v[4];
#pragma unroll
			for (int r = 0; r < 4; r++) v[r] = fetch(m0 + 64 * r);
			float s[NQ];
#pragma unroll
			for (int r = 0; r < 4; r++) {
				float p[NQ];
				prod(v[r], p);
#pragma unroll
				for (int k = 0; k < NQ; k++) s[k] = r ? s[k] + p[k] : p[k];
			}
#pragma unroll
			for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
				for (int k = 0; k < NQ; k++) s[k] += __shfl_xor(s[k], o, 64);
			if (lane == 0) {
#pragma unroll
				for (int k = 0; k < NQ; k++) s_bs[k][q] = s[k];
			}
		}
		__syncthreads();
		if (tid < (uint32_t)NQ)
			for (uint32_t q = 0; q < cn; q++) acc += (double)s_bs[tid][q];
		__syncthreads();
	}
	return acc;
}
