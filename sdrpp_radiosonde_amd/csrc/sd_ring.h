// sd_ring.h -- the small device helpers every pass over a submit's frame records shares (sd_rescue_walk.h, sd_diversity_scan.h, and
// sd_rs41.h for the first of them): a 64-bit value to all lanes, a channel's bit ring as the passes read it -- is a frame still in it,
// n chips from chip k -- and the packers that take every second bit of a word.  All integer work, no state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint64_t sd_uniform64(unsigned long long v)    // a value all lanes hold alike -> scalar registers
{
	return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
	       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
__device__ __forceinline__ uint64_t sd_readlane64(uint64_t v, int src)    // lane src's value -> scalar registers (src wave-uniform)
{
	return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src) << 32) |
	       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
}

// A channel's bit ring: chip k of the stream is bit k % 32 of word (k / 32) % n_words (a power of two); wpos = chips written so far
struct SdRing { const uint32_t *words; uint32_t n_words; uint64_t wpos; };

// are the n chips from chip p on all written, and none of them overwritten yet?
__device__ __forceinline__ bool sd_ring_holds(const SdRing &r, uint64_t p, uint64_t n)
{
	return !(r.wpos < p + n || r.wpos - p > 32ull * r.n_words);
}
// 32 / 64 chips of the ring from chip k on, the first in bit 0
__device__ __forceinline__ uint32_t sd_ring_chips32(const SdRing &r, uint64_t k)
{
	const uint32_t w = (uint32_t)(k >> 5), mask = r.n_words - 1u;
	return (uint32_t)((((uint64_t)r.words[(w + 1u) & mask] << 32) | r.words[w & mask]) >> ((uint32_t)k & 31u));
}
__device__ __forceinline__ uint64_t sd_ring_chips64(const SdRing &r, uint64_t k)
{
	return (uint64_t)sd_ring_chips32(r, k) | ((uint64_t)sd_ring_chips32(r, k + 32u) << 32);
}

// bits 0, 2, 4 .. of x, packed into the low half
__device__ __forceinline__ uint32_t sd_even_bits32(uint32_t x)
{
	x &= 0x55555555u;
	x = (x | x >> 1) & 0x33333333u;
	x = (x | x >> 2) & 0x0F0F0F0Fu;
	x = (x | x >> 4) & 0x00FF00FFu;
	return (x | x >> 8) & 0x0000FFFFu;
}
__device__ __forceinline__ uint64_t sd_even_bits64(uint64_t x)
{
	return (uint64_t)(sd_even_bits32((uint32_t)x) | sd_even_bits32((uint32_t)(x >> 32)) << 16);
}
