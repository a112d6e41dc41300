// check_diversity_kernel.hip -- sonde_batch_set_diversity for M10 / M20 and MRZ-N1 groups (DESIGN SPEC 3.3l): the pass over the frame
// records of a submit that sees every receiver of one sonde.  These frames carry a 16-bit check and no FEC.  Two failed copies of one
// frame are almost certainly right where they agree, and exactly one of them is wrong where they differ; both checks are linear over
// GF(2) (SPEC 3.3f), so the differing bits are the unknowns of a 16-equation system: the working frame (copy 0, or the bitwise majority
// of three or four copies) is taken if its check passes, else iff exactly one subset of the at most 8 differing bits explains its
// syndrome.
//   one 64-lane wave per group, four waves per workgroup.  The loop over a group -- the next failed record and its partners, this
//   submit's records plus the carried one, the counters, the carried records -- is dv_walk of sd_diversity_scan.h; this file is its
//   pass CdPass.  Lane i holds the 32-bit word i of every copy (a frame
//   has at most 26), so majority and the differing bits are a handful of bitwise operations, V is gathered by ballot into lanes 0..7,
//   and the <= 255 subsets are tried across the wave, four per lane (sd_check_cols.h, shared with check_rescue_kernel.hip).  No LDS.
// Runs behind every other kernel of the submit and behind the align step, on the stream where the submit completes, and rewrites
// records in place.  What one lane wrote to a record and another reads later (a rewritten record's nerr, the carried copy) is ordered
// by a fence and read with agent-scope loads.  Vector stores only.  Bounds: min(counts, max_frames) records per member, 4 slots per
// group, every byte index < len <= 101 (word index < 26 of the 132-word data).
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_check_cols.h"
#include "sd_diversity_scan.h"
#include "sd_div_copies.h"      // cd_word, cd_mask, cd_majority (step 3), cd_write_record (step 6): shared with afsk_diversity_kernel.hip
#include "launch.h"

// Steps 3 to 5 of SPEC 3.3l on K copies of a frame of len bytes; c[j]: this lane's word of copy j (copy 0 is the record to rewrite;
// c[j] for j >= K is not looked at).  Wave-synchronous, every branch wave-uniform, all 64 lanes active.  Returns K (accepted: w = this
// lane's word of the result, frame bytes only), -1 (not attempted), -2 (no subset fits) or -3 (several fit); nv = |V|.
__device__ int cd_combine(const uint16_t *__restrict__ m10tab, const uint16_t *__restrict__ mrztab, bool mrz, int len, int K,
	const uint32_t (&c)[SD_DIV_MAX], int lane, uint32_t &w, int &nv)
{
	// ---- 3. working frame and unknowns
	uint32_t vm;
	cd_majority(len, K, c, lane, w, vm, nv);

	// ---- 4. majority alone: the syndrome of w (this lane's four bytes)
	const uint16_t *tab = mrz ? mrztab : m10tab;
	const int n_cov = len - 2;
	const bool hi_first = !mrz;
	uint32_t s = 0;
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const int i = 4 * lane + b;
		if (i < len) s ^= mq_byte_syndrome(mq_row(tab, n_cov, hi_first, i), (w >> (8 * b)) & 0xFFu);
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) s ^= (uint32_t)__shfl_xor((int)s, off, 64);
	if (mrz) s ^= mq_mrz_crc_of_zeros();
	if (s == 0u && nv >= 1) return K;

	// ---- 5. solve
	if (nv == 0 || nv > MQ_MAX_HINTS) return -1;
	if (!mrz && (DV_U(vm) & 0xFF)) return -1;                  // M10 / M20: the length byte decides the layout
	const int myk = mq_gather<32>(vm, lane);                   // V, ascending, into lanes 0 .. nv - 1
	uint32_t col = 0;
	if (lane < nv) col = mq_col(mq_row(tab, n_cov, hi_first, myk >> 3), 7 - (myk & 7));
	uint32_t U = 0;
	const int nhit = mq_solve(col, nv, s, lane, U);
	if (nhit != 1) return nhit ? -3 : -2;
	w ^= mq_flips<4>(U, myk, 4 * lane);
	return K;
}

// The pass of the walk (sd_diversity_scan.h): lane i holds word i of every copy in registers
struct CdPass {
	const uint16_t *m10tab /* [99][8] */, *mrztab /* [43][8] */;
	bool mrz;
	uint32_t c[SD_DIV_MAX];
	static constexpr uint32_t nerr = 1;
	__device__ __forceinline__ bool takes(const SdDivGroup *G, uint32_t &kind)
	{
		const uint32_t k = (uint32_t)DV_U(G->kind);
		mrz = k == SONDE_MRZN1;
		kind = mrz ? SONDE_MRZN1 : SONDE_M10;      // one of two constants: the walk's predicates fold to these two kinds
		return k == SONDE_M10 || mrz;
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
		if (cd_combine(m10tab, mrztab, mrz, flen, K, c, lane, w, nv) <= 0) return DV_TRIED;
		cd_write_record(fr, flen, K, nv, w, c[0], lane);
		return DV_COMBINED;
	}
	__device__ __forceinline__ void sync() const {}
};

__global__ __launch_bounds__(64 * DV_WAVES) void sd_check_diversity_kernel(SdDivWalk a, const uint16_t *__restrict__ m10tab,
	const uint16_t *__restrict__ mrztab)
{
	CdPass pass = { m10tab, mrztab, false, { 0u, 0u, 0u, 0u } };
	dv_walk(a, pass);
}

void sd_launch_check_diversity(const SdDivArgs &a) { dv_launch(sd_check_diversity_kernel, a, a.fec.m10tab, a.mrztab); }

// ---- test introspection: steps 3 to 6 alone on caller-made copies (sonde_batch_test_check_combine).  One wave per case; the host has
// checked n_copies (2..4), the copies' type (SONDE_M10 or SONDE_MRZN1) and len (one of the type's, the same in all copies of a case)
// and that copy 0 has failed.
__global__ __launch_bounds__(64 * DV_WAVES) void sd_check_diversity_unit_kernel(
	const uint16_t *__restrict__ m10tab, const uint16_t *__restrict__ mrztab,
	const SondeFrame *__restrict__ copies /* [n][SD_DIV_MAX] */, const uint32_t *__restrict__ n_copies, uint32_t n, SondeFrame *out,
	int32_t *__restrict__ status)
{
	const int lane = threadIdx.x & 63;
	uint32_t k;
	if (!dv_unit_case(k, n, copies, SD_DIV_MAX, out, lane)) return;
	const SondeFrame *cps = copies + (size_t)SD_DIV_MAX * k;
	const int K = DV_U(n_copies[k]), len = DV_U(cps[0].len);
	const bool mrz = (uint32_t)DV_U(cps[0].type) == SONDE_MRZN1;
	uint32_t c[SD_DIV_MAX];
#pragma unroll
	for (int j = 0; j < SD_DIV_MAX; j++) c[j] = j < K ? cd_word(cps + j, len, lane) : 0u;
	uint32_t w;
	int nv;
	const int st = cd_combine(m10tab, mrztab, mrz, len, K, c, lane, w, nv);
	if (st > 0) cd_write_record(out + k, len, K, nv, w, c[0], lane);
	if (lane == 0) status[k] = st;
}

void sd_launch_check_diversity_unit(const SdDivUnitArgs &a)
{
	hipLaunchKernelGGL(sd_check_diversity_unit_kernel, dim3((a.n + DV_WAVES - 1) / DV_WAVES), dim3(64 * DV_WAVES), 0, a.stream,
		a.fec.m10tab, a.mrztab, a.copies, a.n_copies, a.n, a.out, a.status);
}
