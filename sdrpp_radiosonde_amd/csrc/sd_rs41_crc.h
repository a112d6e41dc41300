// sd_rs41_crc.h -- the CRC of an RS41 block (type, len, body[len], crc16), one lane per block, on a frame held in LDS: shared by the
// second passes over RS41 records (rescue_kernel.hip, DESIGN SPEC 3.3c; diversity_kernel.hip, SPEC 3.3j).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// CRC16-CCITT (0x1021, init 0xFFFF) of p[0..n), a byte per step: the eight bit steps of parse.cpp's sonde_crc16_ccitt folded
__device__ __forceinline__ uint32_t rq_crc16(const uint8_t *p, int n)
{
	uint32_t crc = 0xFFFFu;
	auto step = [&](uint32_t v) {
		uint32_t t = (crc >> 8) ^ v;
		t ^= t >> 4;
		crc = ((crc << 8) ^ (t << 12) ^ (t << 5) ^ t) & 0xFFFFu;
	};
	int i = 0;
	for (; i + 8 <= n; i += 8) {           // eight LDS reads in flight, then the eight dependent steps (the chain is what a lane waits for)
		uint32_t v[8];
#pragma unroll
		for (int q = 0; q < 8; q++) v[q] = p[i + q];
#pragma unroll
		for (int q = 0; q < 8; q++) step(v[q]);
	}
	for (; i < n; i++) step(p[i]);
	return crc;
}
// block (off, len) of the frame: does the CRC behind its body match?
__device__ __forceinline__ bool rq_block_ok(const uint8_t *frame, int off, int len)
{
	const uint8_t *body = frame + off + 2;
	return rq_crc16(body, len) == ((uint32_t)body[len] | ((uint32_t)body[len + 1] << 8));
}
