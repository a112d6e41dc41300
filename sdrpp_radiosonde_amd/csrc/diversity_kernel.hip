// diversity_kernel.hip -- sonde_batch_set_diversity (DESIGN SPEC 3.3j): the pass over the RS41 frame records of a submit that sees every
// receiver of one sonde.  A frame that failed alone in each copy (a codeword at nerr = -1) is put together from all of them: whole
// codewords a partner decoded, blocks whose CRC passes in any copy, bytes the copies agree on; what is left is erased, and RS(255,231)
// fills up to 24 erased bytes per codeword (sd_rsee.h).  The result is taken only if both codewords and every block CRC of its own
// chain pass.
//   one 64-lane wave per group, four waves per workgroup (the GF tables are staged once per workgroup, as in rescue_kernel.hip).  The
//   loop over a group -- the next failed record, its partners, the counters, the carried records -- is dv_walk of sd_diversity_scan.h,
//   shared with the other three combining kernels; this file is its pass DvPass: the copies in LDS, steps 3 to 8.  One lane per
//   candidate (length, copy) checks the block CRCs of the chain walk; the decoder is the wave-wide one of sd_rsee.h.
// Runs behind every other kernel of the submit, on the stream where the submit completes, and rewrites records in place.  What one
// lane wrote to a record and another reads later (a rewritten record's nerr, the carried copy) is ordered by a fence and read with
// agent-scope loads.  Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_rsee.h"
#include "sd_rs41_crc.h"
#include "sd_diversity_scan.h"
#include "launch.h"

constexpr int DV_DATA_WORDS = SONDE_FRAME_MAX / 4;

struct DivLds {                    // one per wave: 5.7 KB
	FramerLds f;                                       // f.frame: the working frame
	RseeLds x;
	alignas(4) uint8_t cp[SD_DIV_MAX][SONDE_FRAME_MAX];    // the copies as recorded: cp[0] is the record to rewrite
	alignas(4) uint8_t claim[SONDE_FRAME_MAX];         // step 4: the value a trusted block gives the byte
	alignas(4) uint8_t claimed[SONDE_FRAME_MAX];       // 1: the byte is claimed
	SondeRs41Layout cand;                              // step 7: the result's own chain
	int32_t nerr[SD_DIV_MAX][2];                       // the copies' nerr as recorded
};

__device__ __forceinline__ int dv_cw_of(int o) { return o < 56 ? (o - 8) / RS_R : ((o - 56) & 1); }
__device__ __forceinline__ int dv_pos_of(int o) { return o < 56 ? (o - 8) % RS_R : RS_R + ((o - 56) >> 1); }

__device__ __forceinline__ void dv_copy_frame(uint8_t *dst, const uint8_t *src, int lane)
{
	for (int i = lane; i < DV_DATA_WORDS; i += 64) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
}

// Steps 3 to 7 of SPEC 3.3j on the K copies in s.cp / s.nerr (copy 0 has a failed codeword).  Wave-synchronous, every branch
// wave-uniform.  Returns K (accepted: s.f.frame is the result, cnt0 / cnt1 the bytes of each codeword that differ from copy 0), -1 (a
// codeword with more than 24 erasures), -2 (no decode) or -3 (rejected by the accept step).
__device__ int dv_combine(const FramerTabs &tabs, DivLds &s, int K, int flen, int lane, const GfSwar &swar, int &cnt0, int &cnt1)
{
	const bool failed0 = DV_U(s.nerr[0][0]) < 0, failed1 = DV_U(s.nerr[0][1]) < 0;
	// ---- 3. whole codewords: the first partner that decoded codeword c and holds a codeword there
	int set0 = -1, set1 = -1;
	for (int j = 1; j < K; j++) {
		const bool want0 = failed0 && set0 < 0 && DV_U(s.nerr[j][0]) >= 0, want1 = failed1 && set1 < 0 && DV_U(s.nerr[j][1]) >= 0;
		if (!want0 && !want1) continue;
		dv_copy_frame(s.f.frame, s.cp[j], lane);
		WAVE_SYNC();
		const int n = sd_rs41_deinterleave(s.f, flen, lane);
		WAVE_SYNC();
		const unsigned long long nz = rsee_syndromes(tabs, s.f, n, lane, swar);      // lane = 24 c + j
		if (want0 && (nz & 0xFFFFFFull) == 0ull) set0 = j;
		if (want1 && ((nz >> RS_R) & 0xFFFFFFull) == 0ull) set1 = j;
	}
	const bool open0 = failed0 && set0 < 0, open1 = failed1 && set1 < 0;       // codewords steps 4 to 6 work on
	dv_copy_frame(s.f.frame, s.cp[0], lane);
	for (int i = lane; i < 128; i += 64) reinterpret_cast<uint32_t *>(s.x.er[0])[i] = 0u;
	for (int i = lane; i < DV_DATA_WORDS; i += 64) reinterpret_cast<uint32_t *>(s.claimed)[i] = 0u;
	WAVE_SYNC();
	for (int o = 8 + lane; o < flen; o += 64) {
		const int sj = dv_cw_of(o) ? (failed1 ? set1 : -1) : (failed0 ? set0 : -1);
		if (sj >= 0) s.f.frame[o] = s.cp[sj][o];
	}
	// ---- 4. trusted blocks: one walk over all copies; lane q = (candidate length q / K, copy q % K) checks that block's CRC
	if (open0 || open1) {
		int off = 57;
		for (int nb = 0; nb < 16 && off + 4 <= flen; nb++) {
			uint32_t lens = 0;              // the distinct candidate lengths, a byte each, in copy order
			int nl = 0;
			for (int j = 0; j < K; j++) {
				const int l = DV_U(s.cp[j][off + 1]);
				bool fresh = off + l + 4 <= flen;
				for (int q = 0; q < nl; q++) fresh = fresh && (int)((lens >> (8 * q)) & 0xFFu) != l;
				if (fresh) { lens |= (uint32_t)l << (8 * nl); nl++; }
			}
			if (nl == 0) break;
			const int li = lane / K, ci = lane - li * K;
			const bool ok = lane < nl * K && rq_block_ok(s.cp[ci], off, (int)((lens >> (8 * (li & 3))) & 0xFFu));
			const unsigned long long m = __ballot(ok);
			int len = (int)(lens & 0xFFu);
			if (m) {
				const int q = __builtin_ctzll(m), ql = q / K, qc = q - ql * K;
				len = (int)((lens >> (8 * ql)) & 0xFFu);
				for (int o = off + 1 + lane; o <= off + len + 3; o += 64) { s.claim[o] = s.cp[qc][o]; s.claimed[o] = 1; }
			}
			off += len + 4;
		}
	}
	WAVE_SYNC();
	// ---- 5. votes: claimed value, else the value more than K / 2 copies hold, else an erasure (the byte of copy 0 stays)
	for (int o = 8 + lane; o < flen; o += 64) {
		const int c = dv_cw_of(o);
		if (!(c ? open1 : open0)) continue;
		if (s.claimed[o]) { s.f.frame[o] = s.claim[o]; continue; }
		uint32_t v[SD_DIV_MAX];
#pragma unroll
		for (int j = 0; j < SD_DIV_MAX; j++) v[j] = j < K ? (uint32_t)s.cp[j][o] : 0x100u + (uint32_t)j;
		int val = -1;
#pragma unroll
		for (int j = 0; j < SD_DIV_MAX; j++) {
			int cnt = 0;
#pragma unroll
			for (int i = 0; i < SD_DIV_MAX; i++) cnt += v[i] == v[j];
			if (j < K && 2 * cnt > K) val = (int)v[j];
		}
		if (val >= 0) s.f.frame[o] = (uint8_t)val;
		else s.x.er[c][dv_pos_of(o)] = 1;
	}
	WAVE_SYNC();
	// ---- 6. decode the open codewords (2 v + e <= 24)
	const int n = RS_R + (flen - 56) / 2;
	int e0 = 0, e1 = 0;
	for (int it = 0; it < 4; it++) {
		const int i = lane + 64 * it;
		e0 += __popcll(__ballot(i < n && s.x.er[0][i] != 0));
		e1 += __popcll(__ballot(i < n && s.x.er[1][i] != 0));
	}
	if ((open0 && e0 > RS_R) || (open1 && e1 > RS_R)) return -1;
	(void)sd_rs41_deinterleave(s.f, flen, lane);
	WAVE_SYNC();
	(void)rsee_syndromes(tabs, s.f, n, lane, swar);
	if (open0 && rsee_decode_one(tabs, s.f, s.x, 0, n, lane, swar) < 0) return -2;
	WAVE_SYNC();
	if (open1 && rsee_decode_one(tabs, s.f, s.x, 1, n, lane, swar) < 0) return -2;
	WAVE_SYNC();
	for (int c = 0; c < 2; c++) {
		if (!(c ? open1 : open0)) continue;
		for (int kk = lane; kk < n; kk += 64) {
			if (kk < RS_R) s.f.frame[8 + RS_R * c + kk] = s.f.cw[c][kk];
			else s.f.frame[56 + 2 * (kk - RS_R) + c] = s.f.cw[c][kk];
		}
	}
	WAVE_SYNC();
	// ---- 7. accept: both codewords' syndromes zero, and the result's own chain lands on flen with every block CRC passing
	if (rsee_syndromes(tabs, s.f, n, lane, swar) != 0ull) return -3;
	if (lane == 0) {
		int off = 57, nb = 0;
		bool good = true;
		while (off < flen) {
			if (nb == 16 || off + 4 > flen) { good = false; break; }
			const int len = s.f.frame[off + 1];
			if (off + len + 4 > flen) { good = false; break; }
			s.cand.offset[nb] = (uint16_t)off;
			s.cand.len[nb] = (uint8_t)len;
			off += len + 4;
			nb++;
		}
		s.cand.n_blocks = good ? (uint32_t)nb : 0u;
	}
	WAVE_SYNC();
	const int nb = DV_U(s.cand.n_blocks);
	if (nb == 0) return -3;
	const bool okb = lane >= nb || rq_block_ok(s.f.frame, s.cand.offset[lane & 15], s.cand.len[lane & 15]);
	if (__ballot(!okb) != 0ull) return -3;
	// ---- 8. the bytes of each codeword that differ from copy 0 as recorded
	cnt0 = 0; cnt1 = 0;
	for (int o0 = 8; o0 < flen; o0 += 64) {
		const int o = o0 + lane;
		const bool diff = o < flen && s.f.frame[o] != s.cp[0][o];
		const int c = o < flen ? dv_cw_of(o) : 0;
		cnt0 += __popcll(__ballot(diff && c == 0));
		cnt1 += __popcll(__ballot(diff && c == 1));
	}
	return K;
}

// the accepted result into the record: data, nerr of the codewords that had failed, flags
__device__ __forceinline__ void dv_write_record(const DivLds &s, SondeFrame *fr, int K, int flen, int cnt0, int cnt1, int lane)
{
	for (int i = lane; 4 * i < flen; i += 64) {
		const int rem = flen - 4 * i;
		uint32_t wd = reinterpret_cast<const uint32_t *>(s.f.frame)[i];
		if (rem < 4) wd &= (1u << (8 * rem)) - 1u;
		reinterpret_cast<uint32_t *>(fr->data)[i] = wd;
	}
	if (lane == 0) {
		if (s.nerr[0][0] < 0) fr->nerr[0] = cnt0;
		if (s.nerr[0][1] < 0) fr->nerr[1] = cnt1;
		fr->flags |= SONDE_FRAME_RESCUED | SONDE_FRAME_COMBINED | ((uint32_t)K << 8);
	}
}

__device__ __forceinline__ void dv_stage_tabs(FramerTabs &tabs, GfSwar &swar, const uint8_t *gf_exp, const uint8_t *gf_log, const uint32_t *gf_swar, int tid)
{
	const uint32_t *sw = gf_swar + 8 * ((tid & 63) % RS_R);
	swar.a_lo = sw[0]; swar.a_hi = sw[1]; swar.b_lo = sw[2]; swar.b_hi = sw[3]; swar.c = sw[4];
	for (int i = tid; i < GF_EXP2 / 16; i += 64 * DV_WAVES) reinterpret_cast<uint4 *>(tabs.exp2)[i] = reinterpret_cast<const uint4 *>(gf_exp)[i];
	if (tid < 512 / 16) reinterpret_cast<uint4 *>(tabs.log2)[tid] = reinterpret_cast<const uint4 *>(gf_log)[tid];
	__syncthreads();
}

// The RS41 pass of the walk (sd_diversity_scan.h): the copies and their nerr live in the wave's LDS slots, which every visit reuses.
// OTHER_KINDS = false: every group of the table is RS41 and the kind word is not read; true: the table has groups of the other kinds,
// which are the other combining kernels'.  The host launches the one that fits the table.
template <bool OTHER_KINDS> struct DvPass {
	const FramerTabs &tabs; DivLds &s;
	static constexpr uint32_t nerr = 3;
	GfSwar swar;                   // by value: a reference would hide from the inliner that the decoder's argument is this kernel's own
	__device__ __forceinline__ bool takes(const SdDivGroup *G, uint32_t &kind) const
	{
		kind = SONDE_RS41;
		return !OTHER_KINDS || DV_U(G->kind) == SONDE_RS41;
	}
	__device__ __forceinline__ int flen(const SondeFrame *fr) const { return DV_U(fr->len); }
	__device__ __forceinline__ void copy(int K, const SondeFrame *f, int n0, int n1, int lane)
	{
		if (lane == 0) { s.nerr[K][0] = n0; s.nerr[K][1] = n1; }
		dv_copy_frame(s.cp[K], f->data, lane);
	}
	__device__ __forceinline__ void partner(int K, const SondeFrame *pf, uint32_t, int n0, int n1, int, int lane) { copy(K, pf, n0, n1, lane); }
	__device__ __forceinline__ int attempt(SondeFrame *fr, uint32_t, int K, int flen, int lane)
	{
		copy(0, fr, fr->nerr[0], fr->nerr[1], lane);
		WAVE_SYNC();
		int cnt0 = 0, cnt1 = 0;
		if (dv_combine(tabs, s, K, flen, lane, swar, cnt0, cnt1) <= 0) return DV_TRIED;
		dv_write_record(s, fr, K, flen, cnt0, cnt1, lane);
		return DV_COMBINED;
	}
	__device__ __forceinline__ void sync() const { WAVE_SYNC(); }
};

template <bool OTHER_KINDS> __global__ __launch_bounds__(64 * DV_WAVES) void sd_diversity_kernel(SdDivWalk a,
	const uint8_t *__restrict__ gf_exp, const uint8_t *__restrict__ gf_log, const uint32_t *__restrict__ gf_swar)
{
	__shared__ __attribute__((aligned(16))) FramerTabs tabs;
	__shared__ __attribute__((aligned(16))) DivLds wl[DV_WAVES];
	DvPass<OTHER_KINDS> pass = { tabs, wl[threadIdx.x >> 6], {} };
	dv_stage_tabs(tabs, pass.swar, gf_exp, gf_log, gf_swar, threadIdx.x);
	dv_walk(a, pass);
}

void sd_launch_diversity(const SdDivArgs &a)
{
	if (a.other_kinds) dv_launch(sd_diversity_kernel<true>, a, a.fec.gfexp, a.fec.gflog, a.fec.gfswar);
	else dv_launch(sd_diversity_kernel<false>, a, a.fec.gfexp, a.fec.gflog, a.fec.gfswar);
}

// ---- a restarted group (sonde_batch_restart_channels lists all its members): no carried records, counters zero, the align step's
// state (SPEC 3.3k) as set_diversity left it.  One workgroup per listed channel; slot_of[channel] = SD_DIV_MAX * group + member, or -1
// for a channel in no group.  The workgroups of a group's members write the same values to the group's words.
__global__ __launch_bounds__(64) void sd_diversity_clear_kernel(const uint32_t *__restrict__ list, const int32_t *__restrict__ slot_of,
	SondeFrame *__restrict__ carried, uint32_t *__restrict__ counters, const SdDivGroup *__restrict__ groups, SdDivState *__restrict__ states,
	uint32_t unlocked_start)
{
	const int32_t slot = slot_of[list[blockIdx.x]];
	if (slot < 0) return;
	uint32_t *p = reinterpret_cast<uint32_t *>(carried + slot);
	if ((int)threadIdx.x < DV_DATA_WORD0) p[threadIdx.x] = 0u;        // the header: len = 0 is "none"
	if (threadIdx.x < 2) counters[2 * (slot / SD_DIV_MAX) + threadIdx.x] = 0u;
	if (threadIdx.x == 2) {
		const SdDivGroup *G = groups + slot / SD_DIV_MAX;
		SdDivState *S = states + slot / SD_DIV_MAX;
		S->off[slot % SD_DIV_MAX] = G->off[slot % SD_DIV_MAX];
		S->locked = unlocked_start ? 0u : (1u << G->n) - 1u;
		S->learned = 0u;
		S->duplicates = 0u;
	}
}
void sd_launch_diversity_clear(uint32_t n, hipStream_t stream, const uint32_t *list, const int32_t *slot_of, SondeFrame *carried, uint32_t *counters,
	const SdDivGroup *groups, SdDivState *states, uint32_t unlocked_start)
{
	hipLaunchKernelGGL(sd_diversity_clear_kernel, dim3(n), dim3(64), 0, stream, list, slot_of, carried, counters, groups, states, unlocked_start);
}

// ---- test introspection: steps 3 to 7 alone on caller-made copies (sonde_batch_test_rs41_combine).  One wave per case; the host has
// checked n_copies (2..4) and the copies' len (320 or 518, the same in all copies of a case) and that copy 0 has a failed codeword.
__global__ __launch_bounds__(64 * DV_WAVES) void sd_diversity_unit_kernel(
	const uint8_t *__restrict__ gf_exp, const uint8_t *__restrict__ gf_log, const uint32_t *__restrict__ gf_swar,
	const SondeFrame *__restrict__ copies /* [n][SD_DIV_MAX] */, const uint32_t *__restrict__ n_copies, uint32_t n, SondeFrame *out,
	int32_t *__restrict__ status)
{
	__shared__ __attribute__((aligned(16))) FramerTabs tabs;
	__shared__ __attribute__((aligned(16))) DivLds wl[DV_WAVES];
	const int lane = threadIdx.x & 63;
	GfSwar swar;
	dv_stage_tabs(tabs, swar, gf_exp, gf_log, gf_swar, threadIdx.x);
	uint32_t k;
	if (!dv_unit_case(k, n, copies, SD_DIV_MAX, out, lane)) return;
	DivLds &s = wl[threadIdx.x >> 6];
	const SondeFrame *cps = copies + (size_t)SD_DIV_MAX * k;
	const int K = DV_U(n_copies[k]), flen = DV_U(cps[0].len);
	for (int j = 0; j < K; j++) {
		dv_copy_frame(s.cp[j], cps[j].data, lane);
		if (lane < 2) s.nerr[j][lane] = cps[j].nerr[lane];
	}
	WAVE_SYNC();
	int cnt0 = 0, cnt1 = 0;
	const int st = dv_combine(tabs, s, K, flen, lane, swar, cnt0, cnt1);
	if (st > 0) dv_write_record(s, out + k, K, flen, cnt0, cnt1, lane);
	if (lane == 0) status[k] = st;
}
void sd_launch_diversity_unit(const SdDivUnitArgs &a)
{
	hipLaunchKernelGGL(sd_diversity_unit_kernel, dim3((a.n + DV_WAVES - 1) / DV_WAVES), dim3(64 * DV_WAVES), 0, a.stream,
		a.fec.gfexp, a.fec.gflog, a.fec.gfswar, a.copies, a.n_copies, a.n, a.out, a.status);
}
