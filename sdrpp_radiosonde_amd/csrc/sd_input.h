// sd_input.h -- the formats of the input rows (host and device).  The kinds are the public SONDE_INPUT_* of sonde_abi.h, the only
// numbering: complex64 (IQ, 8 bytes per sample), float FM-discriminator samples (REAL, 4), int16 I, Q pairs (IQ16, 4: what SDR hardware
// and WAV recordings hold, little endian) and int8 pairs (IQ8, 2).  The integer kinds are converted exactly in the load path (int ->
// float, no scaling: the discriminator does not depend on the amplitude; SPEC 3.0c), then every kernel runs the complex64 arithmetic.
// A kernel that takes rows is a template on the kind; sd_input_dispatch picks the instantiation.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/sonde_abi.h"

constexpr bool sd_input_known(int k) { return k == SONDE_INPUT_IQ || k == SONDE_INPUT_REAL || k == SONDE_INPUT_IQ16 || k == SONDE_INPUT_IQ8; }
constexpr bool sd_input_complex(int k) { return k == SONDE_INPUT_IQ || k == SONDE_INPUT_IQ16 || k == SONDE_INPUT_IQ8; }      // what a mixer or a transform takes
constexpr size_t sd_sample_bytes(int k) { return k == SONDE_INPUT_IQ ? 8 : (k == SONDE_INPUT_IQ8 ? 2 : 4); }

// calls f(std::integral_constant<int, K>()) for the runtime kind K (the entry points refuse unknown kinds when they are created)
template <typename F> inline void sd_input_dispatch(int kind, F &&f)
{
	switch (kind) {
	case SONDE_INPUT_IQ:   f(std::integral_constant<int, SONDE_INPUT_IQ>()); break;
	case SONDE_INPUT_REAL: f(std::integral_constant<int, SONDE_INPUT_REAL>()); break;
	case SONDE_INPUT_IQ16: f(std::integral_constant<int, SONDE_INPUT_IQ16>()); break;
	case SONDE_INPUT_IQ8:  f(std::integral_constant<int, SONDE_INPUT_IQ8>()); break;
	}
}

// ---- device converters
// one complex sample of 16- / 8-bit integers (I in the low bits) -> float2
static __device__ __forceinline__ float2 sd_cs16_f2(uint32_t q) { return make_float2((float)(int16_t)(q & 0xffffu), (float)((int32_t)q >> 16)); }
static __device__ __forceinline__ float2 sd_cs8_f2(uint16_t q) { return make_float2((float)(int8_t)(q & 0xffu), (float)(int8_t)(q >> 8)); }
// two complex samples (I0 Q0 I1 Q1, little endian) -> the float4 of the float path
static __device__ __forceinline__ float4 sd_cs16_f4(uint2 q)
{
	return make_float4((float)(int16_t)(q.x & 0xffffu), (float)((int32_t)q.x >> 16), (float)(int16_t)(q.y & 0xffffu), (float)((int32_t)q.y >> 16));
}
static __device__ __forceinline__ float4 sd_cs8_f4(uint32_t q)
{
	return make_float4((float)(int8_t)(q & 0xffu), (float)(int8_t)((q >> 8) & 0xffu), (float)(int8_t)((q >> 16) & 0xffu), (float)((int32_t)q >> 24));
}
// one complex sample as a row of IQ kind K holds it; sd_iq_f2 / sd_iq_f4: one / two of them as float2 / float4 (the float kinds: as they are)
template <int K> using sd_iq_t = typename std::conditional<K == SONDE_INPUT_IQ16, uint32_t, typename std::conditional<K == SONDE_INPUT_IQ8, uint16_t, float2>::type>::type;
static_assert(sizeof(sd_iq_t<SONDE_INPUT_IQ16>) == sd_sample_bytes(SONDE_INPUT_IQ16) && sizeof(sd_iq_t<SONDE_INPUT_IQ8>) == sd_sample_bytes(SONDE_INPUT_IQ8), "sample sizes");
template <int K> static __device__ __forceinline__ float2 sd_iq_f2(sd_iq_t<K> q)
{
	if constexpr (K == SONDE_INPUT_IQ16) return sd_cs16_f2(q); else if constexpr (K == SONDE_INPUT_IQ8) return sd_cs8_f2(q); else return q;
}
template <int K, typename T> static __device__ __forceinline__ float4 sd_iq_f4(T q)
{
	if constexpr (K == SONDE_INPUT_IQ16) return sd_cs16_f4(q); else if constexpr (K == SONDE_INPUT_IQ8) return sd_cs8_f4(q); else return q;
}
// SPEC 3.0d: the two half-sums of a group of four, (samples 0 + 1, samples 2 + 3), each exact in integers: (P0.re, P0.im, P1.re, P1.im)
typedef short sd_i16x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ float4 sd_cs16_halves(uint4 q)
{
	const sd_i16x2 lo = {1, 0}, hi = {0, 1};
	int a = 0, b = 0, c = 0, d = 0;
	a = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.x), lo, a, false); b = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.x), hi, b, false);
	a = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.y), lo, a, false); b = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.y), hi, b, false);
	c = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.z), lo, c, false); d = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.z), hi, d, false);
	c = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.w), lo, c, false); d = __builtin_amdgcn_sdot2(__builtin_bit_cast(sd_i16x2, q.w), hi, d, false);
	return make_float4((float)a, (float)b, (float)c, (float)d);
}
static __device__ __forceinline__ float4 sd_cs8_halves(uint2 q)
{
	int a = 0, b = 0, c = 0, d = 0;
	a = __builtin_amdgcn_sdot4((int)q.x, 0x00010001, a, false); b = __builtin_amdgcn_sdot4((int)q.x, 0x01000100, b, false);
	c = __builtin_amdgcn_sdot4((int)q.y, 0x00010001, c, false); d = __builtin_amdgcn_sdot4((int)q.y, 0x01000100, d, false);
	return make_float4((float)a, (float)b, (float)c, (float)d);
}
// the same for wave-uniform operands (scalar loads): plain integer adds, which the scalar unit has
static __device__ __forceinline__ float4 sd_cs16_halves_uniform(uint4 q)
{
	return make_float4((float)((int)(int16_t)(q.x & 0xffffu) + (int)(int16_t)(q.y & 0xffffu)), (float)(((int32_t)q.x >> 16) + ((int32_t)q.y >> 16)),
	                   (float)((int)(int16_t)(q.z & 0xffffu) + (int)(int16_t)(q.w & 0xffffu)), (float)(((int32_t)q.z >> 16) + ((int32_t)q.w >> 16)));
}
static __device__ __forceinline__ float4 sd_cs8_halves_uniform(uint2 q)
{
	return make_float4((float)((int)(int8_t)(q.x & 0xffu) + (int)(int8_t)((q.x >> 16) & 0xffu)), (float)((int)(int8_t)((q.x >> 8) & 0xffu) + ((int32_t)q.x >> 24)),
	                   (float)((int)(int8_t)(q.y & 0xffu) + (int)(int8_t)((q.y >> 16) & 0xffu)), (float)((int)(int8_t)((q.y >> 8) & 0xffu) + ((int32_t)q.y >> 24)));
}
