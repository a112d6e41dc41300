// sd_diversity_scan.h -- what the five combining passes of sonde_batch_set_diversity share (DESIGN "what a combining pass plugs into";
// diversity_kernel.hip, SPEC 3.3j: RS41; check_diversity_kernel.hip, SPEC 3.3l: M10 / M20 / MRZ-N1; dfm_diversity_kernel.hip, SPEC 3.3m:
// DFM; ims_diversity_kernel.hip, SPEC 3.3n: iMS-100; afsk_diversity_kernel.hip, SPEC 3.3o: iMet and C50): the two predicates of a group's kind (SdDivGroup.kind = the members' sonde type)
// -- which record lengths are frames, and when a record has failed --, the members of a group, steps 1 and 2 of SPEC 3.3j -- the scan
// of the members' record headers for the next failed record in (t, member) order and for its partner in another member --, the
// carried records, and dv_walk, the loop that strings them together: one 64-lane wave per group, DV_WAVES waves per workgroup, every
// result wave-uniform.  A pass is a struct with
//   static constexpr uint32_t nerr      the nerr words its kinds' failed rule looks at (bit 0, bit 1): of a partner only those are
//                                       loaded; the other is handed on as 0
//   bool takes(G, kind)                 is the group one of its kinds?  Sets kind (the RS41 pass of a table of RS41 groups alone does
//                                       not read the kind word)
//   int flen(fr) const                  the length a partner of the failed record fr must have
//   void partner(K, pf, ch, n0, n1, flen, lane)
//                                       the failed partner pf (channel ch, nerr as read: n0, n1) becomes copy K = 1 .. 3
//   int attempt(fr, ch, K, flen, lane)  the rule on fr (channel ch) as copy 0 and the K - 1 partners: DV_SKIPPED (the record does not
//                                       count as tried), DV_TRIED (it stays as recorded) or DV_COMBINED (rewritten)
//   void sync()                         at the end of every visit and in front of the carried records: a pass whose copies live in LDS
//                                       orders their reuse here
// and the walk is inlined into the pass's kernel: no call, no pointer to a function.  Copies a pass holds in registers are selected by
// K == 1 ? .. : .., never indexed by K.
#pragma once
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_ring.h"
#include "launch.h"

#define DV_WAVES 4
#define DV_U(x) __builtin_amdgcn_readfirstlane((int)(x))
constexpr int DV_REC_WORDS = (int)(sizeof(SondeFrame) / 4);
constexpr int DV_DATA_WORD0 = (int)(offsetof(SondeFrame, data) / 4);

// a frame length of the kind: RS41 {320, 518}, M10 / M20 {101, 70}, MRZ-N1 {45}, DFM {33}, iMS-100 {51}, iMet 5 .. 64, C50 {9}
__device__ __forceinline__ bool dv_len_ok(uint32_t kind, int len)
{
	return kind == SONDE_M10 ? (len == 101 || len == 70) : kind == SONDE_MRZN1 ? len == 45 : kind == SONDE_DFM09 ? len == 33 :
	       kind == SONDE_IMS100 ? len == 51 : kind == SONDE_IMET4 ? (len >= 5 && len <= 64) : kind == SONDE_C50 ? len == 9 :
	       (len == 320 || len == 518);
}
// failed: RS41 a codeword at nerr < 0, M10 / M20 / MRZ-N1 and iMet / C50 the 16-bit check (nerr[0] < 0; nerr[1] counts Manchester violations there),
// DFM a Hamming word the first pass gave up on (nerr[1] > 0; nerr[0] counts corrected words there), iMS-100 a BCH block it rejected
// (nerr[1] > 0; nerr[0] counts corrected bits there).  A record with a frame length that has not failed is good: to the scan and as a
// partner (the align step, diversity_align_kernel.hip, states the same per kind as al_good)
__device__ __forceinline__ bool dv_failed(uint32_t kind, int nerr0, int nerr1)
{
	if (kind == SONDE_DFM09 || kind == SONDE_IMS100) return nerr1 > 0;
	return nerr0 < 0 || (kind == SONDE_RS41 && nerr1 < 0);
}
__device__ __forceinline__ bool dv_failed(uint32_t kind, const SondeFrame *f) { return dv_failed(kind, f->nerr[0], f->nerr[1]); }

// a word of a record another lane of this wave may have written earlier in this kernel
__device__ __forceinline__ uint32_t dv_load_fresh(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t dv_wave_min(uint32_t v)
{
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
	return v;
}

// The members of a group: channel, offset, records of this submit (wave-uniform; the member loops are unrolled over SD_DIV_MAX and the
// selectors below keep the arrays in registers).  The offsets and the lock bits are the align step's (SPEC 3.3k; an earlier launch, or
// as set_diversity left them): to steps 1 to 8 an unlocked member has no records (cnt), all[] is what the carried records are kept up
// to date from.
struct DvMembers {
	SondeFrame *frames;
	uint32_t max_frames, lockmask, total;
	int nm;
	uint32_t ch[SD_DIV_MAX], cnt[SD_DIV_MAX], all[SD_DIV_MAX], start[SD_DIV_MAX + 1];
	int64_t ofs[SD_DIV_MAX];
	__device__ __forceinline__ SondeFrame *rec_of(int m, uint32_t i) const
	{
		return frames + (size_t)ch_of(m) * max_frames + i;
	}
	__device__ __forceinline__ uint32_t ch_of(int m) const { return m == 0 ? ch[0] : m == 1 ? ch[1] : m == 2 ? ch[2] : ch[3]; }
	__device__ __forceinline__ int64_t ofs_of(int m) const { return m == 0 ? ofs[0] : m == 1 ? ofs[1] : m == 2 ? ofs[2] : ofs[3]; }
	__device__ __forceinline__ uint32_t cnt_of(int m) const { return m == 0 ? cnt[0] : m == 1 ? cnt[1] : m == 2 ? cnt[2] : cnt[3]; }
};

__device__ __forceinline__ void dv_members(DvMembers &M, SondeFrame *frames, const uint32_t *__restrict__ counts, uint32_t max_frames,
	const SdDivGroup *G, const SdDivState *S)
{
	M.frames = frames; M.max_frames = max_frames;
	M.nm = DV_U(G->n);
	M.lockmask = (uint32_t)DV_U(dv_load_fresh(&S->locked));
	M.start[0] = 0;
#pragma unroll
	for (int m = 0; m < SD_DIV_MAX; m++) {
		M.ch[m] = m < M.nm ? (uint32_t)DV_U(G->ch[m]) : 0u;
		M.all[m] = m < M.nm ? (uint32_t)DV_U(min(counts[M.ch[m]], max_frames)) : 0u;
		M.cnt[m] = (M.lockmask >> m) & 1u ? M.all[m] : 0u;
		M.ofs[m] = m < M.nm ? (int64_t)sd_uniform64(__hip_atomic_load(reinterpret_cast<const uint64_t *>(&S->off[m]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
		M.start[m + 1] = M.start[m] + M.cnt[m];
	}
	M.total = M.start[SD_DIV_MAX];
}

// Step 1: the failed record with the smallest (t, member) above the last one visited (last_t, last_m; both are moved on).  A record an
// earlier visit rewrote has been visited, so what the scan reads of the records still to visit is what the first pass recorded.
// Returns false when there is none; else t_r, and bk = member << 16 | record.
__device__ __forceinline__ bool dv_next_failed(const DvMembers &M, uint32_t kind, int lane, int64_t &last_t, int &last_m, int64_t &t_r, uint32_t &bk_out)
{
	int64_t bt = INT64_MAX;
	uint32_t bk = 0xFFFFFFFFu;                     // member << 16 | record
	for (uint32_t p = (uint32_t)lane; p < M.total; p += 64) {
		const int m = p >= M.start[3] ? 3 : p >= M.start[2] ? 2 : p >= M.start[1] ? 1 : 0;
		const uint32_t i = p - (m == 3 ? M.start[3] : m == 2 ? M.start[2] : m == 1 ? M.start[1] : 0u);
		const SondeFrame *f = M.rec_of(m, i);
		if (!dv_len_ok(kind, f->len) || !dv_failed(kind, f)) continue;
		const int64_t t = (int64_t)f->bitpos - M.ofs_of(m);
		if (t < last_t || (t == last_t && m <= last_m)) continue;
		const uint32_t k = ((uint32_t)m << 16) | i;
		if (t < bt || (t == bt && k < bk)) { bt = t; bk = k; }
	}
#pragma unroll
	for (int sh = 32; sh >= 1; sh >>= 1) {
		const int64_t ot = __shfl_xor((long long)bt, sh, 64);
		const uint32_t ok = (uint32_t)__shfl_xor((int)bk, sh, 64);
		if (ot < bt || (ot == bt && ok < bk)) { bt = ot; bk = ok; }
	}
	bk = (uint32_t)DV_U(bk);
	if (bk == 0xFFFFFFFFu) return false;
	t_r = (int64_t)sd_uniform64((uint64_t)bt);
	last_t = t_r; last_m = (int)(bk >> 16);
	bk_out = bk;
	return true;
}

// Step 2: the partner in member b of a record of length flen at t_r -- the nearest record of the same length within the window, this
// submit's or the carried one cf (key: 2 |dt| + (dt > 0), so that of two equally near ones the earlier wins; low half: record + 1,
// 0 = the carried record).  Null: none.
__device__ __forceinline__ const SondeFrame *dv_partner(const DvMembers &M, int b, int flen, int64_t t_r, uint32_t window, const SondeFrame *cf, int lane)
{
	uint32_t best = 0xFFFFFFFFu;
	for (uint32_t j = (uint32_t)lane; j <= M.cnt_of(b); j += 64) {       // j = cnt: the carried record
		const SondeFrame *f = j < M.cnt_of(b) ? M.rec_of(b, j) : cf;
		if (f->len != flen) continue;
		const int64_t dt = (int64_t)f->bitpos - M.ofs_of(b) - t_r;
		const uint64_t ad = (uint64_t)(dt < 0 ? -dt : dt);
		if (ad > (uint64_t)window) continue;
		best = min(best, (((uint32_t)ad * 2u + (dt > 0 ? 1u : 0u)) << 16) | (j < M.cnt_of(b) ? j + 1u : 0u));
	}
	best = (uint32_t)DV_U(dv_wave_min(best));
	if (best == 0xFFFFFFFFu) return nullptr;
	const uint32_t idx = best & 0xFFFFu;
	return idx ? M.rec_of(b, idx - 1u) : cf;
}

// The carried records: each member's newest record of this submit with a frame length, as the pass left it (carried_g: the group's
// SD_DIV_MAX slots).  The caller has fenced its own record stores.
__device__ __forceinline__ void dv_carry(const DvMembers &M, uint32_t kind, SondeFrame *carried_g, int lane)
{
#pragma unroll
	for (int m = 0; m < SD_DIV_MAX; m++) {
		if (m >= M.nm) continue;
		uint32_t newest = 0;                           // record + 1
		for (uint32_t j = (uint32_t)lane; j < M.all[m]; j += 64)
			if (dv_len_ok(kind, M.rec_of(m, j)->len)) newest = j + 1u;
		newest = ~(uint32_t)DV_U(dv_wave_min(~newest));
		if (!newest) continue;
		const uint32_t *from = reinterpret_cast<const uint32_t *>(M.rec_of(m, newest - 1u));
		uint32_t *to = reinterpret_cast<uint32_t *>(carried_g + m);
		for (int i = lane; i < DV_REC_WORDS; i += 64) to[i] = dv_load_fresh(from + i);
	}
}

// ---- the walk
// copy K = 1 .. 3 of a pass that holds its copies in registers: every element is stored to under a constant index (a store under the
// index K would put the array into scratch)
template <typename T> __device__ __forceinline__ void dv_set_copy(T (&x)[SD_DIV_MAX], int K, T v)
{
	x[1] = K == 1 ? v : x[1]; x[2] = K == 2 ? v : x[2]; x[3] = K == 3 ? v : x[3];
}
// copy j of such a pass, j wave-uniform or not: all four are read first, for the same reason
template <typename T> __device__ __forceinline__ T dv_copy_of(const T (&x)[SD_DIV_MAX], int j)
{
	const T x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
	return j == 0 ? x0 : j == 1 ? x1 : j == 2 ? x2 : x3;
}
enum { DV_SKIPPED = 0, DV_TRIED = 1, DV_COMBINED = 2 };
// what every combining kernel takes (SdDivArgs, as the device sees it); counters: [n_groups][2] (tried, combined)
struct SdDivWalk {
	SondeFrame *frames; const uint32_t *counts; uint32_t max_frames;
	const SdDivGroup *groups; const SdDivState *states; uint32_t n_groups, window;
	SondeFrame *carried; uint32_t *counters;
};

template <class Pass> __device__ __forceinline__ void dv_walk(const SdDivWalk &a, Pass &pass)
{
	const int lane = threadIdx.x & 63;
	const uint32_t g = DV_WAVES * blockIdx.x + (threadIdx.x >> 6);
	if (g >= a.n_groups) return;
	const SdDivGroup *G = a.groups + g;
	uint32_t kind;
	if (!pass.takes(G, kind)) return;                  // another kernel's group
	DvMembers M;
	dv_members(M, a.frames, a.counts, a.max_frames, G, a.states + g);
	SondeFrame *const carried_g = a.carried + (size_t)SD_DIV_MAX * g;

	// ---- steps 1 and 2: the failed records in ascending (t, member), each with its partners
	uint32_t tried = 0, combined = 0;
	int64_t last_t = INT64_MIN, t_r;
	int last_m = -1;
	uint32_t bk;
	while (dv_next_failed(M, kind, lane, last_t, last_m, t_r, bk)) {
		const int m_r = (int)(bk >> 16);
		SondeFrame *fr = M.rec_of(m_r, bk & 0xFFFFu);
		const int flen = pass.flen(fr);
		// partners: in every other locked member the nearest record of that length within the window, this submit's or the carried
		// one.  A good partner ends it: no member behind it is searched
		int K = 1;
		bool any_good = false;
#pragma unroll
		for (int b = 0; b < SD_DIV_MAX; b++) {
			if (b >= M.nm || b == m_r || any_good || !((M.lockmask >> b) & 1u)) continue;
			const SondeFrame *pf = dv_partner(M, b, flen, t_r, a.window, carried_g + b, lane);
			if (!pf) continue;
			const int pn0 = Pass::nerr & 1u ? DV_U(dv_load_fresh(reinterpret_cast<const uint32_t *>(&pf->nerr[0]))) : 0;
			const int pn1 = Pass::nerr & 2u ? DV_U(dv_load_fresh(reinterpret_cast<const uint32_t *>(&pf->nerr[1]))) : 0;
			if (!dv_failed(kind, pn0, pn1)) { any_good = true; continue; }
			// a partner that is not good has not been rewritten: its data are as recorded
			pass.partner(K, pf, M.ch_of(b), pn0, pn1, flen, lane);
			K++;
		}
		// no partner, or the group has a good copy already: the record stays as recorded
		const int r = K == 1 || any_good ? DV_SKIPPED : pass.attempt(fr, M.ch_of(m_r), K, flen, lane);
		tried += r != DV_SKIPPED;
		combined += r == DV_COMBINED;
		if (r == DV_COMBINED) __threadfence();         // the scan and later partners read the rewritten record
		pass.sync();
	}

	// ---- the carried records: each member's newest record of this submit with a frame length, as the pass left it
	__threadfence();
	pass.sync();
	dv_carry(M, kind, carried_g, lane);
	if (lane == 0 && (tried | combined)) { a.counters[2 * g] += tried; a.counters[2 * g + 1] += combined; }
}

// the launch of a combining kernel (SdDivWalk first, then what the pass adds) over the group table
template <class... P, class... A> static inline void dv_launch(void (*kernel)(SdDivWalk, P...), const SdDivArgs &a, A... extra)
{
	const SdDivWalk w = { a.frames, a.counts, a.max_frames, a.groups, a.states, a.n_groups, a.window, a.carried, a.counters };
	hipLaunchKernelGGL(kernel, dim3((a.n_groups + DV_WAVES - 1) / DV_WAVES), dim3(64 * DV_WAVES), 0, a.stream, w, extra...);
}

// ---- what the five unit kernels (test introspection: a pass's rule alone on caller-made cases, one wave per case) begin with: the
// case k of this wave (false: there is none), and out[k] = copy 0 of the case (copy0[stride * k]) in memory before the result is
// written over it (other lanes write the same words then)
__device__ __forceinline__ bool dv_unit_case(uint32_t &k, uint32_t n, const SondeFrame *copy0, uint32_t stride, SondeFrame *out, int lane)
{
	k = DV_WAVES * blockIdx.x + (threadIdx.x >> 6);
	if (k >= n) return false;
	const uint32_t *from = reinterpret_cast<const uint32_t *>(copy0 + (size_t)stride * k);
	for (int i = lane; i < DV_REC_WORDS; i += 64) reinterpret_cast<uint32_t *>(out + k)[i] = from[i];
	__threadfence();
	return true;
}
