// dfm_rescue_kernel.hip -- SONDE_FLAG_DFM_RESCUE (DESIGN SPEC 3.3g): the second pass over the DFM06/09/17 frame records of a submit.
// The framer takes every data bit from the first chip of its Manchester pair and decodes Hamming(8,4) with hard decisions: a word
// with two wrong bits is given up (nerr[1]), and the host drops the frame.  The second chip of a pair says which bits are doubtful:
// a pair with two equal chips is an ERASURE, and the extended Hamming code (distance 4) decodes any word with 2v + e <= 3, v unknown
// errors and e erasures.  A frame is rescued iff every word the first pass gave up on decodes that way.
//   one 64-lane wave per channel, four waves per workgroup; lanes load the headers of 64 records at once and the wave works on
//   the candidates among them one by one: lane i < 33 owns codeword i, reads its byte of the record and the 16 chips of its eight
//   pairs from the channel's bit ring, and decodes it on its own.  No LDS.
// Runs behind whatever wrote the records, on the same stream, and rewrites them in place.  The records of a channel are
// independent of each other (only the two counters are shared), so the result does not depend on the cut into submits.
// Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "launch.h"

#define DQ_WAVES 4
#define DQ_MAX_WORDS 8         // SPEC 3.3g step 3: at most this many failed words
#define DQ_FRAME_CHIPS 560

// the four parity checks of a word (rows 0x78 / 0xB4 / 0xD2 / 0xE1 = bits 3..0), as in sd_dfm_decode_frame
__device__ __forceinline__ uint32_t dq_syndrome(uint32_t w)
{
	return ((uint32_t)__popc(w & 0x78u) & 1u) << 3 | ((uint32_t)__popc(w & 0xB4u) & 1u) << 2 |
	       ((uint32_t)__popc(w & 0xD2u) & 1u) << 1 | ((uint32_t)__popc(w & 0xE1u) & 1u);
}

// SPEC 3.3g step 4 for one word: w as received, E the mask of its erased bits (0x80 >> j: bit j).  Returns the number of bits
// changed and w = the codeword, or -1 (w untouched): e = 0, e > 3, or no codeword within 2v + e <= 3.
// The code is linear: flipping the bits S changes the syndrome by syndrome(S).  So every way of being wrong inside E is one submask
// S of E (at most 8), and what is left of the syndrome must be nothing (v = 0) or, when e = 1 leaves room for v = 1, the column of
// one bit outside E.  Distance 4 makes the answer unique, so the first fit is the only one.
__device__ __forceinline__ int sd_hamming84_erasures(uint32_t &w, uint32_t E)
{
	const int e = __popc(E);
	if (e == 0 || e > 3) return -1;
	// syndrome -> the bit j whose column it is, one nibble each (9: none; the rows above put the weight-3 columns on bits 0..3)
	const unsigned long long col_of = 0x9329199409959678ull;
	for (uint32_t S = E;; S = (S - 1u) & E) {
		const uint32_t t = dq_syndrome(w ^ S);
		uint32_t flips = S;
		bool fit = t == 0u;
		if (!fit && e == 1) {
			const uint32_t j = (uint32_t)(col_of >> (4u * t)) & 15u;
			if (j < 8u && !((0x80u >> j) & E)) { flips |= 0x80u >> j; fit = true; }
		}
		if (fit) { w ^= flips; return __popc(flips); }
		if (S == 0u) return -1;
	}
}

__device__ __forceinline__ uint32_t dq_chip(const uint32_t *__restrict__ ring, uint32_t mask, uint64_t k)
{
	return (ring[(uint32_t)(k >> 5) & mask] >> ((uint32_t)k & 31u)) & 1u;
}

__global__ __launch_bounds__(64 * DQ_WAVES) void sd_dfm_rescue_kernel(
	const SdChanState *__restrict__ chan_states, const uint32_t *__restrict__ bitring, uint32_t ring_words,
	SondeFrame *__restrict__ frames, const uint32_t *__restrict__ counts, uint32_t max_frames,
	const uint32_t *__restrict__ chlist, uint32_t n_list, SdRescueCounters *__restrict__ states)
{
	const int lane = threadIdx.x & 63;
	const uint32_t li_ch = DQ_WAVES * blockIdx.x + (threadIdx.x >> 6);
	if (li_ch >= n_list) return;
	const uint32_t ch = chlist[li_ch];
	const uint32_t nfr = min(counts[ch], max_frames);
	if (nfr == 0) return;
	const uint64_t wpos = chan_states[ch].wpos;
	const uint32_t *ring = bitring + (size_t)ch * ring_words;
	const uint32_t mask = ring_words - 1;
	SondeFrame *const chfr = frames + (size_t)ch * max_frames;
	uint32_t tried = 0, rescued = 0;

	// where codeword `lane` lies in the frame (SPEC 3.3b's interleaving): its bit j is frame bit off + j N + i
	const int blk = lane < 7 ? 0 : (lane < 20 ? 1 : 2);
	const int il_off = blk == 0 ? 0 : (blk == 1 ? 56 : 160), il_n = blk == 0 ? 7 : 13;
	const int il_i = lane - (blk == 0 ? 0 : (blk == 1 ? 7 : 20));

	for (uint32_t base = 0; base < nfr; base += 64) {
		// the headers of records base .. base + 63, one per lane
		uint32_t h_p_lo = 0, h_p_hi = 0;
		bool cand = false;
		if (base + (uint32_t)lane < nfr) {
			const SondeFrame *f = chfr + base + lane;
			h_p_lo = (uint32_t)f->bitpos; h_p_hi = (uint32_t)(f->bitpos >> 32);
			cand = f->type == SONDE_DFM09 && f->len == 33 && f->nerr[1] >= 1;
		}
		for (unsigned long long cm = __ballot(cand); cm; cm &= cm - 1ull) {
			const int q = __builtin_ctzll(cm);
			SondeFrame *fr = chfr + base + q;
			const uint64_t p = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)h_p_lo, q) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)h_p_hi, q) << 32);

			// 2. F: the words the first pass left as received
			uint32_t w = 0;
			bool failed = false;
			if (lane < 33) {
				w = fr->data[lane];
				failed = dq_syndrome(w) != 0u;
			}
			const unsigned long long fm = __ballot(failed);
			const int nf = __popcll(fm);
			// 3. the cap, and the frame's chips must still be in the ring (always so for a record of this submit: DESIGN 3.3g)
			if (nf == 0 || nf > DQ_MAX_WORDS) continue;
			if (wpos < p + DQ_FRAME_CHIPS || wpos - p > 32ull * ring_words) continue;
			tried++;

			// 4. E of this lane's word from its eight pairs, and the decode
			int st = 0;
			if (failed) {
				uint32_t E = 0;
#pragma unroll
				for (int j = 0; j < 8; j++) {
					const uint64_t k = p + 32u + 2u * (uint32_t)(il_off + j * il_n + il_i);
					if (dq_chip(ring, mask, k) == dq_chip(ring, mask, k + 1)) E |= 0x80u >> j;
				}
				st = sd_hamming84_erasures(w, E);
			}
			if (__ballot(st < 0)) continue;                         // one word that does not decode: the whole frame stays

			// 5. the record
			if (failed) fr->data[lane] = (uint8_t)w;
			if (lane == 0) {
				fr->nerr[0] += nf;
				fr->nerr[1] = 0;
				fr->flags |= SONDE_FRAME_RESCUED | ((uint32_t)nf << 8);
			}
			rescued++;
		}
	}
	if (tried && lane == 0) {
		states[ch].tried += tried;
		states[ch].rescued += rescued;
	}
}

void sd_launch_rescue_dfm(const SdRescueArgs &a)
{
	hipLaunchKernelGGL(sd_dfm_rescue_kernel, dim3((a.n_list + DQ_WAVES - 1) / DQ_WAVES), dim3(64 * DQ_WAVES), 0, a.stream,
		a.chan_states, a.bitring, a.ring_words, a.frames, a.counts, a.max_frames, a.chlist, a.n_list, (SdRescueCounters *)a.states);
}

// ---- test introspection: step 4 alone on caller-supplied (word, erasure mask) pairs (sonde_batch_test_hamming84_erasures)
__global__ __launch_bounds__(256) void sd_hamming84_unit_kernel(uint8_t *__restrict__ words, const uint8_t *__restrict__ erased, uint32_t n,
	int32_t *__restrict__ status)
{
	const uint32_t i = 256 * blockIdx.x + threadIdx.x;
	if (i >= n) return;
	uint32_t w = words[i];
	const int st = sd_hamming84_erasures(w, erased[i]);
	words[i] = (uint8_t)w;
	status[i] = st;
}
void sd_launch_hamming84_unit(uint8_t *words, const uint8_t *erased, uint32_t n, int32_t *status, hipStream_t stream)
{
	hipLaunchKernelGGL(sd_hamming84_unit_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, words, erased, n, status);
}
