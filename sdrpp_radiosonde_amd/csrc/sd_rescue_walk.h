// sd_rescue_walk.h -- the walk over a submit's frame records that the rescue passes share (DESIGN "what a rescue pass plugs into"):
// one 64-lane wave per listed channel, SD_RESCUE_WAVES waves per workgroup; lanes load the headers of 64 records at once, the wave
// works on the candidates among them one by one, in ascending record order, and the channel's two counters are added to at the end.
// A pass is a struct with
//   static constexpr uint32_t header   the SD_H_* fields of a record it looks at; only those are loaded and handed on.  A pass
//                                      without SD_H_BITPOS reads no ring: the walk then fetches neither wpos nor the ring pointer
//   bool candidate(h) const            per lane, on that lane's header: may this record reach the decoder?
//   int repair(fr, h, ctx)             by the whole wave, h = the candidate's header (wave-uniform): SD_RESCUE_SKIPPED (the record
//                                      does not count as tried), SD_RESCUE_TRIED (it stays as recorded) or SD_RESCUE_DONE (rewritten)
// and the walk is inlined into the pass's kernel: no call, no pointer to a function.  The RS41 pass (rescue_kernel.hip) has a loop of
// its own: it learns from EVERY record in order and keeps its state in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_ring.h"
#include "launch.h"

#define SD_RESCUE_WAVES 4

enum { SD_H_TYPE = 1, SD_H_LEN = 2, SD_H_NERR0 = 4, SD_H_NERR1 = 8, SD_H_BITPOS = 16 };
enum { SD_RESCUE_SKIPPED = 0, SD_RESCUE_TRIED = 1, SD_RESCUE_DONE = 2 };
struct SdRecHeader { uint32_t type; int len, nerr0, nerr1; uint64_t bitpos; };        // fields outside the pass's `header` are zero
struct SdRescueCtx { int lane; uint32_t ch; SdRing ring; };

// what every pass kernel takes (SdRescueArgs, as the device sees it)
struct SdRescueWalk {
	const SdChanState *chan_states; const uint32_t *bitring; uint32_t ring_words;
	SondeFrame *frames; const uint32_t *counts; uint32_t max_frames;
	const uint32_t *chlist; uint32_t n_list; SdRescueCounters *counters;
};

template <class Pass> __device__ __forceinline__ void sd_rescue_walk(const SdRescueWalk &a, Pass &pass)
{
	constexpr uint32_t H = Pass::header;
	const int lane = threadIdx.x & 63;
	const uint32_t li_ch = SD_RESCUE_WAVES * blockIdx.x + (threadIdx.x >> 6);
	if (li_ch >= a.n_list) return;
	const uint32_t ch = a.chlist[li_ch];
	const uint32_t nfr = min(a.counts[ch], a.max_frames);
	if (nfr == 0) return;
	SdRescueCtx ctx = { lane, ch, { nullptr, 0u, 0ull } };
	if (H & SD_H_BITPOS) ctx.ring = SdRing{ a.bitring + (size_t)ch * a.ring_words, a.ring_words, a.chan_states[ch].wpos };
	SondeFrame *const chfr = a.frames + (size_t)ch * a.max_frames;
	uint32_t tried = 0, rescued = 0;

	for (uint32_t base = 0; base < nfr; base += 64) {
		// the headers of records base .. base + 63, one per lane
		SdRecHeader h = {};
		bool cand = false;
		if (base + (uint32_t)lane < nfr) {
			const SondeFrame *f = chfr + base + lane;
			if (H & SD_H_TYPE) h.type = f->type;
			if (H & SD_H_LEN) h.len = f->len;
			if (H & SD_H_NERR0) h.nerr0 = f->nerr[0];
			if (H & SD_H_NERR1) h.nerr1 = f->nerr[1];
			if (H & SD_H_BITPOS) h.bitpos = f->bitpos;
			cand = pass.candidate(h);
		}
		for (unsigned long long cm = __ballot(cand); cm; cm &= cm - 1ull) {
			const int q = __builtin_ctzll(cm);
			SdRecHeader u = {};
			if (H & SD_H_TYPE) u.type = (uint32_t)__builtin_amdgcn_readlane((int)h.type, q);
			if (H & SD_H_LEN) u.len = __builtin_amdgcn_readlane(h.len, q);
			if (H & SD_H_NERR0) u.nerr0 = __builtin_amdgcn_readlane(h.nerr0, q);
			if (H & SD_H_NERR1) u.nerr1 = __builtin_amdgcn_readlane(h.nerr1, q);
			if (H & SD_H_BITPOS) u.bitpos = sd_readlane64(h.bitpos, q);
			const int r = pass.repair(chfr + base + q, u, ctx);
			tried += r != SD_RESCUE_SKIPPED;
			rescued += r == SD_RESCUE_DONE;
		}
	}
	if (tried && lane == 0) {
		a.counters[ch].tried += tried;
		a.counters[ch].rescued += rescued;
	}
}

// the launch of a pass kernel (SdRescueWalk first, then what the pass adds) over the channels of its list
template <class... P, class... A> static inline void sd_rescue_launch(void (*kernel)(SdRescueWalk, P...), const SdRescueArgs &a, A... extra)
{
	const SdRescueWalk w = { a.chan_states, a.bitring, a.ring_words, a.frames, a.counts, a.max_frames, a.chlist, a.n_list, (SdRescueCounters *)a.states };
	hipLaunchKernelGGL(kernel, dim3((a.n_list + SD_RESCUE_WAVES - 1) / SD_RESCUE_WAVES), dim3(64 * SD_RESCUE_WAVES), 0, a.stream, w, extra...);
}
