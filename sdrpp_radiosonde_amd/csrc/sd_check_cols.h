// sd_check_cols.h -- the 16-bit checks of M10 / M20 and MRZ-N1 as GF(2) column tables (DESIGN SPEC 3.3f step 3): the column of a frame
// bit is the change of the syndrome when the bit flips.  Shared by the two passes that solve for wrong bits from the syndrome:
// check_rescue_kernel.hip (SPEC 3.3f: the unknowns are the Manchester violations) and check_diversity_kernel.hip (SPEC 3.3l: the
// unknowns are the bits on which the receivers' copies differ).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MQ_MAX_HINTS 8         // SPEC 3.3f: at most this many marked bits (255 subsets)

// CRC16 (reflected 0xA001) of the 43 zero bytes from 0xFFFF: the constant part of MRZ-N1's affine check
static constexpr uint32_t mq_mrz_crc_of_zeros()
{
	uint32_t crc = 0xFFFFu;
	for (int i = 0; i < 43 * 8; i++) crc = (crc & 1u) ? ((crc >> 1) ^ 0xA001u) : (crc >> 1);
	return crc;
}

// the frame byte i of a record of n_cov covered bytes followed by the two stored check bytes: the eight columns of its bits (bit j
// of the byte = LSB index j) as four dwords of two 16-bit columns each, like a row of m10tab.  hi_first: the stored check is big-endian.
__device__ __forceinline__ uint4 mq_row(const uint16_t *__restrict__ tab, int n_cov, bool hi_first, int i)
{
	if (i < n_cov) return *reinterpret_cast<const uint4 *>(tab + 8 * (n_cov - 1 - i));
	// a bit of the stored check flips that bit of the syndrome
	const uint32_t sh = ((i == n_cov) == hi_first) ? 8u : 0u;
	return make_uint4(0x00020001u << sh, 0x00080004u << sh, 0x00200010u << sh, 0x00800040u << sh);
}
__device__ __forceinline__ uint32_t mq_col(const uint4 row, int j)
{
	const uint32_t w = (j >> 1) == 0 ? row.x : ((j >> 1) == 1 ? row.y : ((j >> 1) == 2 ? row.z : row.w));
	return (w >> (16 * (j & 1))) & 0xFFFFu;
}
// XOR of the columns of the bits set in byte b
__device__ __forceinline__ uint32_t mq_byte_syndrome(const uint4 row, uint32_t b)
{
	uint32_t s = 0;
#pragma unroll
	for (int j = 0; j < 8; j++) if ((b >> j) & 1u) s ^= mq_col(row, j);
	return s;
}

// The unknowns into lanes: vm = this lane's marked bits, bit q of it frame bit BPL * lane + q (frame bit k = bit 7 - k % 8 of byte
// k / 8).  The marked bits of the wave, ascending, go to lanes 0 .. nv - 1: returns this lane's frame bit (0 for lane >= nv).
template <int BPL> __device__ __forceinline__ int mq_gather(uint32_t vm, int lane)
{
	int myk = 0, n = 0;
	for (unsigned long long lm = __ballot(vm != 0u); lm; lm &= lm - 1ull) {
		const int l = __builtin_ctzll(lm);
		for (uint32_t bm = (uint32_t)__builtin_amdgcn_readlane((int)vm, l); bm; bm &= bm - 1u) {
			if (lane == n) myk = BPL * l + __builtin_ctz(bm);
			n++;
		}
	}
	return myk;
}
// The solution back into the frame: of the unknowns in U (bit j: lane j's, frame bit myk there) those that fall into the NB frame bytes
// from byte `first` on, as an XOR mask over these bytes (byte first + b at bits 8 b .. 8 b + 7)
template <int NB> __device__ __forceinline__ uint32_t mq_flips(uint32_t U, int myk, int first)
{
	uint32_t fm = 0;
#pragma unroll
	for (int j = 0; j < MQ_MAX_HINTS; j++) {
		const int kj = __builtin_amdgcn_readlane(myk, j), b = (kj >> 3) - first;
		if (((U >> j) & 1u) && b >= 0 && b < NB) fm ^= (0x80u >> (kj & 7)) << (8 * b);
	}
	return fm;
}

// SPEC 3.3f step 4: the subsets m = 1 .. 2^nv - 1 of nv <= MQ_MAX_HINTS unknowns (bit j of m: the unknown whose column lane j holds in
// col) tried across the wave, four per lane.  Returns how many of them XOR to s; U = one that does (the one, if the count is 1).
__device__ __forceinline__ int mq_solve(uint32_t col, int nv, uint32_t s, int lane, uint32_t &U)
{
	uint32_t c[MQ_MAX_HINTS];
#pragma unroll
	for (int j = 0; j < MQ_MAX_HINTS; j++) c[j] = (uint32_t)__builtin_amdgcn_readlane((int)col, j);
	int nhit = 0;
#pragma unroll
	for (int it = 0; it < 4; it++) {
		const uint32_t m = (uint32_t)(64 * it + lane);
		uint32_t x = 0;
#pragma unroll
		for (int j = 0; j < MQ_MAX_HINTS; j++) if ((m >> j) & 1u) x ^= c[j];
		const unsigned long long hm = __ballot(m != 0u && m < (1u << nv) && x == s);
		nhit += __popcll(hm);
		if (hm) U = (uint32_t)(64 * it + __builtin_ctzll(hm));
	}
	return nhit;
}
