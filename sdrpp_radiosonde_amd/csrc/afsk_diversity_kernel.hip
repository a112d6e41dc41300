// afsk_diversity_kernel.hip -- sonde_batch_set_diversity for iMet and SRS-C50 groups (SONDE_FLAG_AFSK_DIVERSITY, DESIGN SPEC 3.3o): the
// pass over the packet records of a submit that sees every receiver of one sonde.  These packets carry a 16-bit check and nothing
// else: no FEC, no second chip per bit.  Two failed copies of one packet are almost certainly right where they agree, and exactly one
// of them is wrong where they differ: the working frame (copy 0, or the bitwise majority of three or four copies) is taken if its
// check passes, else iff exactly one non-empty subset of the at most 8 differing bits makes it pass.
//   iMet: CRC16-CCITT is affine over GF(2), so the subsets are solved for from the syndrome with the columns of sd_ccitt_cols.h
//   (shared with afsk_rescue_kernel.hip) and the solver of sd_check_cols.h (shared with the passes of SPEC 3.3f and 3.3l).
//   C50: the two running byte sums are not linear; both are recomputed for each of the <= 255 subsets, four per lane.
//   one 64-lane wave per group, four waves per workgroup.  The loop over a group is dv_walk of sd_diversity_scan.h; this file is its
//   pass AdPass.  Lane i holds the 32-bit word i of every copy (a packet has at most 16); majority, the differing bits and the record
//   store are sd_div_copies.h's, shared with check_diversity_kernel.hip.  No LDS.
// One launch per kind (the kinds have different default windows: batch_impl.h k_div_passes), each over the whole table, behind every
// other kernel of the submit, the AFSK rescue pass (SPEC 3.3i) included, and behind the align step; records are rewritten in place.
// What one lane wrote to a record and another reads later (a rewritten record's nerr, the carried copy) is ordered by a fence and
// read with agent-scope loads.  Vector stores only.  Bounds: min(counts, max_frames) records per member, 4 slots per group, every
// byte index < len <= 64 (word index < 16 of the 132-word data), every index into aq_pow < len - 2 <= 62.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_check_cols.h"
#include "sd_ccitt_cols.h"
#include "sd_diversity_scan.h"
#include "sd_div_copies.h"
#include "launch.h"

// C50's check on the packet whose words 0 .. 2 are w0, w1, w2: c1, c2 over data[2 .. 6] as in sd_c50_kernel, stored at bytes 7 and 8
__device__ __forceinline__ bool ad_c50_ok(uint32_t w0, uint32_t w1, uint32_t w2)
{
	const uint32_t b[5] = { (w0 >> 16) & 0xFFu, w0 >> 24, w1 & 0xFFu, (w1 >> 8) & 0xFFu, (w1 >> 16) & 0xFFu };
	uint32_t c1 = 0, c2 = 0;
#pragma unroll
	for (int i = 0; i < 5; i++) { c1 = (c1 + b[i]) & 0xFFu; c2 = (c2 + c1) & 0xFFu; }
	return c1 == (w1 >> 24) && c2 == (w2 & 0xFFu);
}

// Step 5 for C50: the subsets m = 1 .. 2^nv - 1 of the nv <= MQ_MAX_HINTS unknowns (bit j of m: frame bit myk of lane j) applied to the
// packet (w0, w1, w2: wave-uniform) and checked whole, four per lane.  Returns how many pass; U = one that does.
__device__ __forceinline__ int ad_c50_solve(int myk, int nv, uint32_t w0, uint32_t w1, uint32_t w2, int lane, uint32_t &U)
{
	uint32_t f0[MQ_MAX_HINTS], f1[MQ_MAX_HINTS], f2[MQ_MAX_HINTS];      // unknown j as an XOR mask over the three words
#pragma unroll
	for (int j = 0; j < MQ_MAX_HINTS; j++) {
		const int kj = __builtin_amdgcn_readlane(myk, j), q = kj & 31;
		const uint32_t bit = (0x80u >> (q & 7)) << (8 * (q >> 3));
		f0[j] = (kj >> 5) == 0 ? bit : 0u; f1[j] = (kj >> 5) == 1 ? bit : 0u; f2[j] = (kj >> 5) == 2 ? bit : 0u;
	}
	int nhit = 0;
#pragma unroll
	for (int it = 0; it < 4; it++) {
		const uint32_t m = (uint32_t)(64 * it + lane);
		uint32_t x0 = w0, x1 = w1, x2 = w2;
#pragma unroll
		for (int j = 0; j < MQ_MAX_HINTS; j++)
			if ((m >> j) & 1u) { x0 ^= f0[j]; x1 ^= f1[j]; x2 ^= f2[j]; }
		const unsigned long long hm = __ballot(m != 0u && m < (1u << nv) && ad_c50_ok(x0, x1, x2));
		nhit += __popcll(hm);
		if (hm) U = (uint32_t)(64 * it + __builtin_ctzll(hm));
	}
	return nhit;
}

// Steps 3 to 5 of SPEC 3.3o on K copies of a packet of len bytes; c[j]: this lane's word of copy j (copy 0 is the record to rewrite;
// c[j] for j >= K is not looked at).  Wave-synchronous, every branch wave-uniform, all 64 lanes active.  Returns K (accepted: w = this
// lane's word of the result, packet bytes only), -1 (not attempted), -2 (no subset fits) or -3 (several fit); nv = |V|.
__device__ int ad_combine(bool c50, int len, int K, const uint32_t (&c)[SD_DIV_MAX], int lane, uint32_t &w, int &nv)
{
	// ---- 3. working frame and unknowns
	uint32_t vm;
	cd_majority(len, K, c, lane, w, vm, nv);
	uint32_t U = 0;
	int nhit, myk;
	if (c50) {
		// ---- 4. majority alone
		const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)w, 0), w1 = (uint32_t)__builtin_amdgcn_readlane((int)w, 1),
			w2 = (uint32_t)__builtin_amdgcn_readlane((int)w, 2);
		if (ad_c50_ok(w0, w1, w2) && nv >= 1) return K;
		// ---- 5. solve
		if (nv == 0 || nv > MQ_MAX_HINTS) return -1;
		myk = mq_gather<32>(vm, lane);                         // V, ascending, into lanes 0 .. nv - 1
		nhit = ad_c50_solve(myk, nv, w0, w1, w2, lane, U);
	} else {
		// ---- 4. majority alone: the syndrome of w (this lane's four bytes; the start value is an XOR into bytes 0 and 1)
		uint32_t s = 0;
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int i = 4 * lane + b;
			if (i < len) s ^= aq_imet_cols(aq_imet_col0(len, i), ((w >> (8 * b)) & 0xFFu) ^ aq_imet_init(i));
		}
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) s ^= (uint32_t)__shfl_xor((int)s, off, 64);
		if (s == 0u && nv >= 1) return K;
		// ---- 5. solve
		if (nv == 0 || nv > MQ_MAX_HINTS) return -1;
		// the type byte and XDATA's length byte decide the layout
		const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)w, 0), vm0 = (uint32_t)__builtin_amdgcn_readlane((int)vm, 0);
		if (vm0 & (((w0 >> 8) & 0xFFu) == 3u ? 0xFFFFFFu : 0xFFFFu)) return -1;
		myk = mq_gather<32>(vm, lane);
		uint32_t col = 0;
		if (lane < nv) col = aq_imet_cols(aq_imet_col0(len, myk >> 3), 0x80u >> (myk & 7));
		nhit = mq_solve(col, nv, s, lane, U);
	}
	if (nhit != 1) return nhit ? -3 : -2;
	w ^= mq_flips<4>(U, myk, 4 * lane);
	return K;
}

// The pass of the walk (sd_diversity_scan.h): lane i holds word i of every copy in registers
struct AdPass {
	bool c50;                                      // the launch's kind: SONDE_C50, else SONDE_IMET4
	uint32_t c[SD_DIV_MAX];
	static constexpr uint32_t nerr = 1;
	__device__ __forceinline__ bool takes(const SdDivGroup *G, uint32_t &kind)
	{
		kind = c50 ? SONDE_C50 : SONDE_IMET4;      // one of two constants: the walk's predicates fold to these two kinds
		return (uint32_t)DV_U(G->kind) == kind;
	}
	__device__ __forceinline__ int flen(const SondeFrame *fr) const { return DV_U(fr->len); }
	__device__ __forceinline__ void partner(int K, const SondeFrame *pf, uint32_t, int, int, int flen, int lane)
	{
		dv_set_copy(c, K, cd_word(pf, flen, lane));
	}
	__device__ __forceinline__ int attempt(SondeFrame *fr, uint32_t, int K, int flen, int lane)
	{
		c[0] = cd_word(fr, flen, lane);
		uint32_t w;
		int nv;
		if (ad_combine(c50, flen, K, c, lane, w, nv) <= 0) return DV_TRIED;
		cd_write_record(fr, flen, K, nv, w, c[0], lane);
		return DV_COMBINED;
	}
	__device__ __forceinline__ void sync() const {}
};

__global__ __launch_bounds__(64 * DV_WAVES) void sd_afsk_diversity_kernel(SdDivWalk a, uint32_t c50)
{
	AdPass pass = { c50 != 0u, { 0u, 0u, 0u, 0u } };
	dv_walk(a, pass);
}

// a.kinds: the kinds of the row of k_div_passes that is launched -- SONDE_IMET4 or SONDE_C50
void sd_launch_afsk_diversity(const SdDivArgs &a) { dv_launch(sd_afsk_diversity_kernel, a, (a.kinds >> SONDE_C50) & 1u); }

// ---- test introspection: steps 3 to 6 alone on caller-made copies (sonde_batch_test_afsk_combine).  One wave per case; the host has
// checked n_copies (2..4), the copies' type (SONDE_IMET4 or SONDE_C50) and len (one of the type's, the same in all copies of a case)
// and that copy 0 has failed.
__global__ __launch_bounds__(64 * DV_WAVES) void sd_afsk_diversity_unit_kernel(const SondeFrame *__restrict__ copies /* [n][SD_DIV_MAX] */,
	const uint32_t *__restrict__ n_copies, uint32_t n, SondeFrame *out, int32_t *__restrict__ status)
{
	const int lane = threadIdx.x & 63;
	uint32_t k;
	if (!dv_unit_case(k, n, copies, SD_DIV_MAX, out, lane)) return;
	const SondeFrame *cps = copies + (size_t)SD_DIV_MAX * k;
	const int K = DV_U(n_copies[k]), len = DV_U(cps[0].len);
	const bool c50 = (uint32_t)DV_U(cps[0].type) == SONDE_C50;
	uint32_t c[SD_DIV_MAX];
#pragma unroll
	for (int j = 0; j < SD_DIV_MAX; j++) c[j] = j < K ? cd_word(cps + j, len, lane) : 0u;
	uint32_t w;
	int nv;
	const int st = ad_combine(c50, len, K, c, lane, w, nv);
	if (st > 0) cd_write_record(out + k, len, K, nv, w, c[0], lane);
	if (lane == 0) status[k] = st;
}

void sd_launch_afsk_diversity_unit(const SdDivUnitArgs &a)
{
	hipLaunchKernelGGL(sd_afsk_diversity_unit_kernel, dim3((a.n + DV_WAVES - 1) / DV_WAVES), dim3(64 * DV_WAVES), 0, a.stream,
		a.copies, a.n_copies, a.n, a.out, a.status);
}
