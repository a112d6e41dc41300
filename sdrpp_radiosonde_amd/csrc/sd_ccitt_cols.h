// sd_ccitt_cols.h -- iMet's check, CRC16-CCITT (x^16 + x^12 + x^5 + 1) from 0x1D0F, as GF(2) columns: the column of a packet bit is the
// change of the syndrome (computed CRC XOR stored CRC) when the bit flips -- x^(16 + 8 k + j) mod 0x11021 for bit j (LSB index) of the
// byte with k covered bytes behind it, bit 8 + j / bit j of the syndrome itself for the two stored bytes (big-endian).  The start
// value is an XOR of 0x1D, 0x0F into the first two bytes.  Shared by the two passes that solve for wrong bits of an iMet packet from
// its syndrome: afsk_rescue_kernel.hip (SPEC 3.3i: one bit or an adjacent pair anywhere) and afsk_diversity_kernel.hip (SPEC 3.3o: the
// bits on which the receivers' copies differ).  No table in memory but the 62 powers below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AQ_IMET_MAXLEN 64      // sd_imet_kernel records nothing longer

// x^(16 + 8 k) mod (x^16 + x^12 + x^5 + 1), k = 0 .. 61: the column of bit 0 of the byte with k covered bytes behind it
struct AqPow { uint16_t v[AQ_IMET_MAXLEN - 2]; };
static constexpr uint32_t aq_mulx(uint32_t c) { return (c & 0x8000u) ? ((c << 1) ^ 0x1021u) & 0xFFFFu : (c << 1) & 0xFFFFu; }
static constexpr AqPow aq_make_pow()
{
	AqPow t{};
	uint32_t c = 0x1021u;                  // x^16
	for (int k = 0; k < AQ_IMET_MAXLEN - 2; k++) {
		t.v[k] = (uint16_t)c;
		for (int s = 0; s < 8; s++) c = aq_mulx(c);
	}
	return t;
}
__device__ const AqPow aq_pow = aq_make_pow();

// the column of bit 0 of byte i of a packet of len bytes (i < len <= AQ_IMET_MAXLEN; 0 behind the packet)
__device__ __forceinline__ uint32_t aq_imet_col0(int len, int i)
{
	const int n_cov = len - 2;
	if (i < n_cov) return aq_pow.v[n_cov - 1 - i];
	return i < len ? (i == n_cov ? 0x100u : 0x1u) : 0u;
}
// the change of the iMet syndrome when the bits `m` of a byte flip; c0 = the column of its bit 0
__device__ __forceinline__ uint32_t aq_imet_cols(uint32_t c0, uint32_t m)
{
	uint32_t s = 0, c = c0;
#pragma unroll
	for (int j = 0; j < 8; j++) {
		if ((m >> j) & 1u) s ^= c;
		c = aq_mulx(c);
	}
	return s;
}
// the start value as it enters the syndrome: an XOR into bytes 0 and 1
__device__ __forceinline__ uint32_t aq_imet_init(int i) { return i == 0 ? 0x1Du : i == 1 ? 0x0Fu : 0u; }
