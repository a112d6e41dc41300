// check_rescue_kernel.hip -- SONDE_FLAG_MANCHESTER_RESCUE (DESIGN SPEC 3.3f): the second pass over the M10 / M20 and MRZ-N1 frame
// records of a submit.  These frames carry a 16-bit check and no FEC, but every data bit is a Manchester chip pair (a, !a): a pair
// with two equal chips marks a bit that may be wrong.  A frame whose check fails with 1..8 such pairs is a linear system over GF(2)
// -- 16 equations (the syndrome), one unknown per marked bit, the column of a bit being the change of the syndrome when it flips --
// and is rescued iff exactly one subset of the marked bits explains the syndrome.
//   one 64-lane wave per channel, four waves per workgroup; lanes load the headers of 64 records at once and the wave works on
//   the candidates among them one by one: lane i reads 32 chips of the frame from the channel's bit ring (16 pairs), the marked
//   bits are gathered into lanes 0..7, and the <= 255 subsets are tried across the wave, four per lane.  No LDS.
// Runs behind whatever wrote the records, on the same stream, and rewrites them in place.  The records of a channel are
// independent of each other (only the two counters are shared), so the result does not depend on the cut into submits.
// Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_check_cols.h"
#include "launch.h"

#define MQ_WAVES 4

__global__ __launch_bounds__(64 * MQ_WAVES) void sd_manchester_rescue_kernel(
	const uint16_t *__restrict__ m10tab /* [99][8] */, const uint16_t *__restrict__ mrztab /* [43][8] */,
	const SdChanState *__restrict__ chan_states, const uint32_t *__restrict__ bitring, uint32_t ring_words,
	SondeFrame *__restrict__ frames, const uint32_t *__restrict__ counts, uint32_t max_frames,
	const uint32_t *__restrict__ chlist, uint32_t n_list, SdRescueCounters *__restrict__ states)
{
	const int lane = threadIdx.x & 63;
	const uint32_t li_ch = MQ_WAVES * blockIdx.x + (threadIdx.x >> 6);
	if (li_ch >= n_list) return;
	const uint32_t ch = chlist[li_ch];
	const uint32_t nfr = min(counts[ch], max_frames);
	if (nfr == 0) return;
	const uint64_t wpos = chan_states[ch].wpos;
	const uint32_t *ring = bitring + (size_t)ch * ring_words;
	const uint32_t mask = ring_words - 1;
	SondeFrame *const chfr = frames + (size_t)ch * max_frames;
	uint32_t tried = 0, rescued = 0;

	for (uint32_t base = 0; base < nfr; base += 64) {
		// the headers of records base .. base + 63, one per lane
		int h_len = 0;
		uint32_t h_type = 0, h_p_lo = 0, h_p_hi = 0;
		bool cand = false;
		if (base + (uint32_t)lane < nfr) {
			const SondeFrame *f = chfr + base + lane;
			h_type = f->type; h_len = f->len;
			h_p_lo = (uint32_t)f->bitpos; h_p_hi = (uint32_t)(f->bitpos >> 32);
			const bool known = (h_type == SONDE_M10 && (h_len == 101 || h_len == 70)) || (h_type == SONDE_MRZN1 && h_len == 45);
			// nerr[1] is |V| (sd_fixed.h counts the same pairs): 0 or more than 8 of them never reach the solver
			cand = known && f->nerr[0] == -1 && f->nerr[1] >= 1 && f->nerr[1] <= MQ_MAX_HINTS;
		}
		for (unsigned long long cm = __ballot(cand); cm; cm &= cm - 1ull) {
			const int q = __builtin_ctzll(cm);
			SondeFrame *fr = chfr + base + q;
			const int len = __builtin_amdgcn_readlane(h_len, q);
			const bool mrz = (uint32_t)__builtin_amdgcn_readlane((int)h_type, q) == SONDE_MRZN1;
			const uint64_t p = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)h_p_lo, q) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)h_p_hi, q) << 32);
			const int nbits = 8 * len;
			const uint64_t c0 = p + (mrz ? 48u : 32u);              // the first data chip
			// 2. the frame's chips must still be in the ring (always so for a record of this submit: DESIGN 3.3f)
			if (wpos < c0 + 2ull * (uint64_t)nbits || wpos - p > 32ull * ring_words) continue;

			// 1. V: lane i looks at the 16 pairs of frame bits 16 i .. 16 i + 15
			uint32_t vm = 0;
			if (16 * lane < nbits) {
				const uint64_t cp = c0 + 32ull * (uint64_t)lane;
				const uint32_t w = (uint32_t)(cp >> 5), sh = (uint32_t)cp & 31u;
				const uint32_t r0 = ring[w & mask], r1 = ring[(w + 1) & mask];
				const uint32_t x = (uint32_t)((((uint64_t)r1 << 32) | r0) >> sh);
				uint32_t v = ~(x ^ (x >> 1)) & 0x55555555u;         // even positions: the pair's two chips are equal
				v = (v | (v >> 1)) & 0x33333333u;
				v = (v | (v >> 2)) & 0x0F0F0F0Fu;
				v = (v | (v >> 4)) & 0x00FF00FFu;
				v = (v | (v >> 8)) & 0x0000FFFFu;                   // bit q: pair q
				const int left = nbits - 16 * lane;
				vm = left >= 16 ? v : (v & ((1u << left) - 1u));
			}
			int nv = __popc(vm);
#pragma unroll
			for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off, 64);
			if (nv == 0 || nv > MQ_MAX_HINTS) continue;
			if (!mrz && (__builtin_amdgcn_readfirstlane((int)vm) & 0xFF)) continue;     // M10 / M20: the length byte decides the layout

			// the marked bits, ascending, into lanes 0 .. nv - 1
			int myk = 0, n = 0;
			for (unsigned long long lm = __ballot(vm != 0u); lm; lm &= lm - 1ull) {
				const int l = __builtin_ctzll(lm);
				for (uint32_t bm = (uint32_t)__builtin_amdgcn_readlane((int)vm, l); bm; bm &= bm - 1u) {
					if (lane == n) myk = 16 * l + __builtin_ctz(bm);
					n++;
				}
			}

			// 3. syndrome of the frame as recorded (bytes lane and lane + 64) and the column of this lane's marked bit
			const uint16_t *tab = mrz ? mrztab : m10tab;
			const int n_cov = len - 2;
			const bool hi_first = !mrz;
			uint32_t s = 0;
#pragma unroll
			for (int r = 0; r < 2; r++) {
				const int i = lane + 64 * r;
				if (i < len) s ^= mq_byte_syndrome(mq_row(tab, n_cov, hi_first, i), fr->data[i]);
			}
#pragma unroll
			for (int off = 32; off > 0; off >>= 1) s ^= (uint32_t)__shfl_xor((int)s, off, 64);
			if (mrz) s ^= mq_mrz_crc_of_zeros();
			uint32_t col = 0;
			if (lane < nv) col = mq_col(mq_row(tab, n_cov, hi_first, myk >> 3), 7 - (myk & 7));
			tried++;

			// 4. the subsets m = 1 .. 2^nv - 1 of the marked bits (bit j of m: lane j's), four per lane
			uint32_t U = 0;
			if (mq_solve(col, nv, s, lane, U) != 1) continue;       // none, or several: the frame stays

			// 5. the record: every lane flips what falls into its two bytes
#pragma unroll
			for (int r = 0; r < 2; r++) {
				const int i = lane + 64 * r;
				uint32_t fm = 0;
#pragma unroll
				for (int j = 0; j < MQ_MAX_HINTS; j++) {
					const int kj = __builtin_amdgcn_readlane(myk, j);
					if (((U >> j) & 1u) && (kj >> 3) == i) fm ^= 0x80u >> (kj & 7);
				}
				if (fm) fr->data[i] = (uint8_t)(fr->data[i] ^ fm);
			}
			if (lane == 0) {
				fr->nerr[0] = 0;
				fr->flags |= SONDE_FRAME_RESCUED | ((uint32_t)__popc(U) << 8);
			}
			rescued++;
		}
	}
	if (tried && lane == 0) {
		states[ch].tried += tried;
		states[ch].rescued += rescued;
	}
}

void sd_launch_rescue_manchester(const SdRescueArgs &a)
{
	hipLaunchKernelGGL(sd_manchester_rescue_kernel, dim3((a.n_list + MQ_WAVES - 1) / MQ_WAVES), dim3(64 * MQ_WAVES), 0, a.stream,
		a.fec.m10tab, a.mrztab, a.chan_states, a.bitring, a.ring_words, a.frames, a.counts, a.max_frames, a.chlist, a.n_list, (SdRescueCounters *)a.states);
}
