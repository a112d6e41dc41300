// rescue_kernel.hip -- SONDE_FLAG_RS41_RESCUE (DESIGN SPEC 3.3c): the second pass over the RS41 frame records of a submit.  A frame
// the errors-only corrector gave up on (a codeword at nerr = -1) is a chain of CRC-guarded blocks; with the channel's LEARNED
// block layout written over the type / len bytes, the blocks whose CRC fails say where the damage is, and RS(255,231) fills up
// to 24 erased bytes per codeword (sd_rsee.h) where it corrects only 12 unknown ones.
//   one 64-lane wave per RS41 channel, four waves per workgroup (the GF tables are staged once per workgroup, as in
//   framer_kernel.hip); the wave walks its channel's records of this submit IN ORDER, so the layout it learns from the clean
//   frames and the decisions it takes do not depend on how the stream is cut into submits.
// Runs behind the kernel that wrote the records, on the same stream, and rewrites them in place.  Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_rsee.h"
#include "sd_rs41_crc.h"          // rq_crc16, rq_block_ok
#include "launch.h"

#define RQ_WAVES 4
struct RescueLds {                 // one per wave: 3.3 KB
	FramerLds f;
	RseeLds x;
	alignas(4) uint8_t orig[SONDE_FRAME_MAX];      // the frame as recorded
	SdRescueState st;                              // the channel's layouts and counters, carried from submit to submit
	SondeRs41Layout cand;                          // the chain of the clean frame in work
};

// the record's data words into LDS (and a second copy)
__device__ __forceinline__ void rq_load(const SondeFrame *__restrict__ fr, uint8_t *a, uint8_t *b, int flen, int lane)
{
	const uint32_t *src = reinterpret_cast<const uint32_t *>(fr->data);
	for (int i = lane; 4 * i < flen; i += 64) {
		const uint32_t w = src[i];
		reinterpret_cast<uint32_t *>(a)[i] = w;
		if (b) reinterpret_cast<uint32_t *>(b)[i] = w;
	}
}

__global__ __launch_bounds__(64 * RQ_WAVES) void sd_rs41_rescue_kernel(
	const uint8_t *__restrict__ gf_exp, const uint8_t *__restrict__ gf_log, const uint32_t *__restrict__ gf_swar /* [24][8] */,
	SondeFrame *__restrict__ frames, const uint32_t *__restrict__ counts, uint32_t max_frames,
	const uint32_t *__restrict__ chlist, uint32_t n_list, SdRescueState *__restrict__ states)
{
	__shared__ __attribute__((aligned(16))) FramerTabs tabs;
	__shared__ __attribute__((aligned(16))) RescueLds wl[RQ_WAVES];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	// the wave's channel, its state and the headers of its first 64 records: loads issued before the table staging, so that the
	// dependent round trips (channel list -> count -> records) overlap it
	const uint32_t li_ch = RQ_WAVES * blockIdx.x + (uint32_t)w;
	uint32_t ch = 0, nfr = 0;
	if (li_ch < n_list) {
		ch = chlist ? chlist[li_ch] : li_ch;
		nfr = min(counts[ch], max_frames);
	}
	RescueLds &s = wl[w];
	uint32_t *st32 = reinterpret_cast<uint32_t *>(&s.st);
	uint32_t *gst32 = reinterpret_cast<uint32_t *>(states + ch);
	constexpr int ST_WORDS = (int)(sizeof(SdRescueState) / 4), LAY_WORDS = (int)(sizeof(SondeRs41Layout) / 4);
	SondeFrame *const chfr = frames + (size_t)ch * max_frames;
	int h_len = 0, h_n0 = 0, h_n1 = 0;                         // header of record (k & ~63) + lane
	auto load_headers = [&](uint32_t base) {
		if (base + (uint32_t)lane < nfr) {
			const SondeFrame *f = chfr + base + lane;
			h_len = f->len; h_n0 = f->nerr[0]; h_n1 = f->nerr[1];
		}
	};
	if (nfr) {
		if (lane < ST_WORDS) st32[lane] = gst32[lane];
		load_headers(0);
	}
	GfSwar swar;
	{
		const uint32_t *sw = gf_swar + 8 * (lane % RS_R);
		swar.a_lo = sw[0]; swar.a_hi = sw[1]; swar.b_lo = sw[2]; swar.b_hi = sw[3]; swar.c = sw[4];
		for (int i = tid; i < GF_EXP2 / 16; i += 64 * RQ_WAVES) reinterpret_cast<uint4 *>(tabs.exp2)[i] = reinterpret_cast<const uint4 *>(gf_exp)[i];
		if (tid < 512 / 16) reinterpret_cast<uint4 *>(tabs.log2)[tid] = reinterpret_cast<const uint4 *>(gf_log)[tid];
	}
	__syncthreads();
	if (nfr == 0) return;
	bool dirty = false;

	for (uint32_t k = 0; k < nfr; k++) {
		if (k && (k & 63u) == 0u) load_headers(k);
		SondeFrame *fr = chfr + k;
		const int flen = __builtin_amdgcn_readlane(h_len, (int)(k & 63u));
		const int n0 = __builtin_amdgcn_readlane(h_n0, (int)(k & 63u)), n1 = __builtin_amdgcn_readlane(h_n1, (int)(k & 63u));
		if (flen != 320 && flen != 518) continue;
		const int li = flen == 518 ? 1 : 0;
		SondeRs41Layout &lay = s.st.lay[li];

		if (n0 >= 0 && n1 >= 0) {
			// ---- a frame the first pass found clean or corrected: does it teach the layout?
			// The usual case, 12 bytes read: the type / len bytes at the offsets of the layout the channel has already are the learned
			// ones.  The chain walked from 57 is then that layout again, entry by entry (each len leads to the next learned offset, the
			// last to the frame's end): whether its CRCs pass (learned again, the same) or not (nothing learned), the state stays.
			{
				const int nbs = __builtin_amdgcn_readfirstlane((int)lay.n_blocks);
				bool same = nbs != 0;
				if (lane < nbs) {
					const int o = lay.offset[lane & 15];
					same = fr->data[o] == lay.type[lane & 15] && fr->data[o + 1] == lay.len[lane & 15];
				}
				if (__ballot(!same) == 0ull) continue;
			}
			// else one lane walks the chain as received, then one lane per block checks its CRC
			rq_load(fr, s.f.frame, nullptr, flen, lane);
			WAVE_SYNC();
			if (lane == 0) {
				int off = 57, nb = 0;
				bool good = true;
				while (off < flen) {
					if (nb == 16 || off + 4 > flen) { good = false; break; }
					const int len = s.f.frame[off + 1];
					if (off + len + 4 > flen) { good = false; break; }
					s.cand.offset[nb] = (uint16_t)off;
					s.cand.type[nb] = s.f.frame[off];
					s.cand.len[nb] = (uint8_t)len;
					off += len + 4;
					nb++;
				}
				for (int q = nb; q < 16; q++) { s.cand.offset[q] = 0; s.cand.type[q] = 0; s.cand.len[q] = 0; }
				s.cand.n_blocks = good ? (uint32_t)nb : 0u;
			}
			WAVE_SYNC();
			const int nb = __builtin_amdgcn_readfirstlane((int)s.cand.n_blocks);
			if (nb == 0) continue;
			const bool okb = lane >= nb || rq_block_ok(s.f.frame, s.cand.offset[lane & 15], s.cand.len[lane & 15]);
			if (__ballot(!okb) != 0ull) continue;
			if (lane < LAY_WORDS) reinterpret_cast<uint32_t *>(&lay)[lane] = reinterpret_cast<const uint32_t *>(&s.cand)[lane];
			WAVE_SYNC();
			dirty = true;
			continue;
		}

		// ---- a frame with a failed codeword
		const int nb = __builtin_amdgcn_readfirstlane((int)lay.n_blocks);
		if (nb == 0) continue;                                  // no layout yet: stays as recorded
		const bool failed0 = n0 < 0, failed1 = n1 < 0;
		rq_load(fr, s.f.frame, s.orig, flen, lane);
		if (lane == 0) s.st.tried++;
		dirty = true;
		WAVE_SYNC();
		const int boff = lay.offset[lane & 15], blen = lay.len[lane & 15], btype = lay.type[lane & 15];
		// 1. the learned type / len bytes, at the positions that belong to a failed codeword (frame byte o >= 56: codeword (o - 56) & 1)
		if (lane < nb) {
			if (((boff - 56) & 1) ? failed1 : failed0) s.f.frame[boff] = (uint8_t)btype;
			if (((boff - 55) & 1) ? failed1 : failed0) s.f.frame[boff + 1] = (uint8_t)blen;
		}
		for (int i = lane; i < 128; i += 64) reinterpret_cast<uint32_t *>(s.x.er[0])[i] = 0u;
		WAVE_SYNC();
		// 2. the bad blocks; 3. their body and CRC bytes are the erasures (codeword position 24 + (o - 56) / 2, sd_rs41_deinterleave)
		const unsigned long long badm = __ballot(lane < nb && !rq_block_ok(s.f.frame, boff, blen));
		for (unsigned long long m = badm; m; m &= m - 1ull) {
			const int q = __builtin_ctzll(m);
			const int off = lay.offset[q], len = lay.len[q];
			for (int o = off + 2 + lane; o < off + len + 4; o += 64) s.x.er[(o - 56) & 1][RS_R + ((o - 56) >> 1)] = 1;
		}
		const int n = sd_rs41_deinterleave(s.f, flen, lane);
		WAVE_SYNC();
		(void)rsee_syndromes(tabs, s.f, n, lane, swar);
		// 4. decode the failed codewords (more than 24 erasures, or no codeword within 2 v + e <= 24: the frame stays)
		if (failed0 && rsee_decode_one(tabs, s.f, s.x, 0, n, lane, swar) < 0) continue;
		WAVE_SYNC();
		if (failed1 && rsee_decode_one(tabs, s.f, s.x, 1, n, lane, swar) < 0) continue;
		WAVE_SYNC();
		for (int c = 0; c < 2; c++) {
			if (!(c ? failed1 : failed0)) continue;
			for (int kk = lane; kk < n; kk += 64) {
				if (kk < RS_R) s.f.frame[8 + RS_R * c + kk] = s.f.cw[c][kk];
				else s.f.frame[56 + 2 * (kk - RS_R) + c] = s.f.cw[c][kk];
			}
		}
		WAVE_SYNC();
		// 5. accept: every block of the layout passes its CRC, every type / len byte is the learned one, both codewords' syndromes zero
		const bool okb = lane >= nb || (s.f.frame[boff] == (uint8_t)btype && s.f.frame[boff + 1] == (uint8_t)blen && rq_block_ok(s.f.frame, boff, blen));
		if (__ballot(!okb) != 0ull) continue;
		if (rsee_syndromes(tabs, s.f, n, lane, swar) != 0ull) continue;
		// 6. record
		int cnt0 = 0, cnt1 = 0;
		for (int o0 = 8; o0 < flen; o0 += 64) {
			const int o = o0 + lane;
			const bool diff = o < flen && s.f.frame[o] != s.orig[o];
			const int c = o < 56 ? (o - 8) / RS_R : ((o - 56) & 1);
			cnt0 += __popcll(__ballot(diff && c == 0));
			cnt1 += __popcll(__ballot(diff && c == 1));
		}
		for (int i = lane; 4 * i < flen; i += 64) {
			const int rem = flen - 4 * i;
			uint32_t wd = reinterpret_cast<const uint32_t *>(s.f.frame)[i];
			if (rem < 4) wd &= (1u << (8 * rem)) - 1u;
			reinterpret_cast<uint32_t *>(fr->data)[i] = wd;
		}
		if (lane == 0) {
			if (failed0) fr->nerr[0] = cnt0;
			if (failed1) fr->nerr[1] = cnt1;
			fr->flags |= SONDE_FRAME_RESCUED;
			s.st.rescued++;
		}
		WAVE_SYNC();
	}
	WAVE_SYNC();
	if (dirty && lane < ST_WORDS) gst32[lane] = st32[lane];
}

void sd_launch_rescue_rs41(const SdRescueArgs &a)
{
	hipLaunchKernelGGL(sd_rs41_rescue_kernel, dim3((a.n_list + RQ_WAVES - 1) / RQ_WAVES), dim3(64 * RQ_WAVES), 0, a.stream,
		a.fec.gfexp, a.fec.gflog, a.fec.gfswar, a.frames, a.counts, a.max_frames, a.chlist, a.n_list, (SdRescueState *)a.states);
}

// ---- test introspection: the errors-and-erasures corrector alone on caller-supplied codeword pairs (sonde_batch_test_rs255_erasures).
// One wave per pair; cw_io and erased hold [n_pairs][2][256] bytes (cw_io: positions >= n zero).
__global__ __launch_bounds__(64 * RQ_WAVES) void sd_rsee_unit_kernel(uint8_t *__restrict__ cw_io, const uint8_t *__restrict__ erased, uint32_t n_pairs, int n,
	int32_t *__restrict__ status, const uint8_t *__restrict__ gf_exp, const uint8_t *__restrict__ gf_log, const uint32_t *__restrict__ gf_swar)
{
	__shared__ __attribute__((aligned(16))) FramerTabs tabs;
	__shared__ __attribute__((aligned(16))) FramerLds wf[RQ_WAVES];
	__shared__ __attribute__((aligned(16))) RseeLds wx[RQ_WAVES];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	GfSwar swar;
	const uint32_t *sw = gf_swar + 8 * (lane % RS_R);
	swar.a_lo = sw[0]; swar.a_hi = sw[1]; swar.b_lo = sw[2]; swar.b_hi = sw[3]; swar.c = sw[4];
	for (int i = tid; i < GF_EXP2 / 16; i += 64 * RQ_WAVES) reinterpret_cast<uint4 *>(tabs.exp2)[i] = reinterpret_cast<const uint4 *>(gf_exp)[i];
	if (tid < 512 / 16) reinterpret_cast<uint4 *>(tabs.log2)[tid] = reinterpret_cast<const uint4 *>(gf_log)[tid];
	__syncthreads();
	const uint32_t k = RQ_WAVES * blockIdx.x + (uint32_t)w;
	if (k >= n_pairs) return;
	FramerLds &s = wf[w];
	RseeLds &x = wx[w];
	uint32_t *io = reinterpret_cast<uint32_t *>(cw_io + (size_t)k * 512);
	const uint32_t *ein = reinterpret_cast<const uint32_t *>(erased + (size_t)k * 512);
	for (int i = lane; i < 128; i += 64) {
		reinterpret_cast<uint32_t *>(s.cw[0])[i] = io[i];           // cw[0] and cw[1] are contiguous, and so are er[0] and er[1]
		reinterpret_cast<uint32_t *>(x.er[0])[i] = ein[i];
	}
	WAVE_SYNC();
	(void)rsee_syndromes(tabs, s, n, lane, swar);
	const int st0 = rsee_decode_one(tabs, s, x, 0, n, lane, swar);
	WAVE_SYNC();
	const int st1 = rsee_decode_one(tabs, s, x, 1, n, lane, swar);
	WAVE_SYNC();
	for (int i = lane; i < 128; i += 64) io[i] = reinterpret_cast<uint32_t *>(s.cw[0])[i];
	if (lane < 2) status[2 * k + lane] = lane ? st1 : st0;
}

void sd_launch_rsee_unit(uint8_t *cw_io, const uint8_t *erased, uint32_t n_pairs, int n, int32_t *status, const uint8_t *gf_exp, const uint8_t *gf_log,
	const uint32_t *gf_swar, hipStream_t stream)
{
	hipLaunchKernelGGL(sd_rsee_unit_kernel, dim3((n_pairs + RQ_WAVES - 1) / RQ_WAVES), dim3(64 * RQ_WAVES), 0, stream,
		cw_io, erased, n_pairs, n, status, gf_exp, gf_log, gf_swar);
}
