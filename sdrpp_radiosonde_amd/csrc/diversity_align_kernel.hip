// diversity_align_kernel.hip -- sonde_batch_set_diversity_auto (DESIGN SPEC 3.3k): the align step in front of the combining pass of
// diversity_kernel.hip, check_diversity_kernel.hip, dfm_diversity_kernel.hip and ims_diversity_kernel.hip.  Two good RS41 records of different members whose bytes 8 .. len are identical
// are the same transmitted frame (the frame carries its number and the sonde's serial), and so are two good M10 / M20 or MRZ-N1 records
// whose bytes 0 .. len are (SPEC 3.3l: consecutive frames of one sonde differ), two good DFM records whose 33 bytes are (SPEC 3.3m) and two good iMS-100 records whose 51 bytes are (SPEC 3.3n); from such pairs the step learns where each member's bit count stands on the
// group's clock (SONDE_DIVERSITY_LEARN), and it marks all but one copy of a frame (SONDE_DIVERSITY_MARK_DUPLICATES).
//   one 64-lane wave per group, a launch of its own in front of sd_diversity_kernel on the stream where the submit completes.  The
//   lanes take one member's records (any number: the loops stride by 64) and each walks the other member's; a record's key is two
//   words that differ between any two frames (RS parity bytes; the check bytes), so the byte compare runs for true matches only.
// Writes: the group's SdDivState (lane 0) and the duplicate bit of records (each record by the one lane that owns it).  Nothing the
// step reads of a record (len, nerr, bitpos, data) is written here, and the carried records are only read.  Vector stores only.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "launch.h"

#define AL_U(x) __builtin_amdgcn_readfirstlane((int)(x))

// a member's candidates: recs[0 .. cnt) are its records of this submit, index cnt is its carried record
struct AlMember { SondeFrame *recs; const SondeFrame *carried; uint32_t cnt; };

// The two predicates of the step depend on the group's kind (SdDivGroup.kind; wave-uniform).  al_good says per kind what
// sd_diversity_scan.h says as dv_len_ok && !dv_failed: the step keeps its own statement, one branch on the kind, so that its code
// object stays what it was (profiles/diversity_walk_notes.md).  RS41 (SPEC 3.3k): good = len 320 or 518 and
// both nerr >= 0, the same frame = data[8 .. len) identical.  M10 / M20 and MRZ-N1 (SPEC 3.3l): good = a length of the type and
// nerr[0] >= 0 (nerr[1] counts Manchester violations there), the same frame = data[0 .. len) identical.  DFM (SPEC 3.3m): good = len 33
// and nerr[1] == 0 (no word the first pass gave up on; nerr[0] counts corrected words), the same frame = data[0 .. 33) identical.
// iMS-100 (SPEC 3.3n): good = len 51 and nerr[1] == 0 (no rejected block), the same frame = data[0 .. 51) identical.
// iMet (SPEC 3.3o): good = len 14, 18 or 20 (PTU, GPS, PTUX: they carry a packet counter or the time) and nerr[0] >= 0, the same
// frame = data[0 .. len) identical.  XDATA packets may repeat byte for byte: they are never good here, so they teach no offset and
// are not marked.  C50 packets carry no identity: set_diversity refuses the step for a table with a C50 group.
__device__ __forceinline__ const SondeFrame *al_cand(const AlMember &M, uint32_t i) { return i < M.cnt ? M.recs + i : M.carried; }
__device__ __forceinline__ bool al_good(uint32_t kind, const SondeFrame *f)
{
	if (kind == SONDE_M10) return (f->len == 101 || f->len == 70) && f->nerr[0] >= 0;
	if (kind == SONDE_MRZN1) return f->len == 45 && f->nerr[0] >= 0;
	if (kind == SONDE_DFM09) return f->len == 33 && f->nerr[1] == 0;
	if (kind == SONDE_IMS100) return f->len == 51 && f->nerr[1] == 0;
	if (kind == SONDE_IMET4) return (f->len == 14 || f->len == 18 || f->len == 20) && f->nerr[0] >= 0;
	return (f->len == 320 || f->len == 518) && f->nerr[0] >= 0 && f->nerr[1] >= 0;
}
// the quick reject: two words that differ between any two frames.  RS41: parity bytes of codeword 0 and of codeword 1; the others: the
// frame's last two words, which hold the 16-bit check -- for DFM the end of the second data block, for iMS-100 (len 51: words 11 and
// 12, three bytes of the latter) the data bits of block 11 and the end of block 10 -- (the bytes of the last word behind len are not
// looked at; the key only spares the byte compare, which decides)
__device__ __forceinline__ uint32_t al_key(uint32_t kind, const SondeFrame *f)
{
	const uint32_t *w = reinterpret_cast<const uint32_t *>(f->data);
	if (kind == SONDE_RS41) return w[2] ^ w[8];
	const int len = f->len, wl = (len - 1) >> 2;           // a good record: len is 33, 45, 51, 70 or 101, wl >= 8; iMet 14, 18 or 20, wl >= 3
	const uint32_t last = (len & 3) ? w[wl] & ((1u << (8 * (len & 3))) - 1u) : w[wl];
	return last ^ ((w[wl - 1] << 13) | (w[wl - 1] >> 19));
}
// two good records: the same length and data[8 .. len) (RS41), data[0 .. len) (the others) identical; whole words, and the bytes of a
// last part-filled word
__device__ __forceinline__ bool al_match(uint32_t kind, const SondeFrame *x, const SondeFrame *y)
{
	const int len = x->len;
	if (y->len != len || al_key(kind, x) != al_key(kind, y)) return false;
	const uint32_t *a = reinterpret_cast<const uint32_t *>(x->data), *b = reinterpret_cast<const uint32_t *>(y->data);
	uint32_t diff = 0;
	for (int i = kind == SONDE_RS41 ? 2 : 0; i < len / 4; i++) diff |= a[i] ^ b[i];
	if (len & 3) diff |= (a[len / 4] ^ b[len / 4]) & ((1u << (8 * (len & 3))) - 1u);
	return diff == 0;
}

__device__ __forceinline__ int64_t al_u64(int64_t v)
{
	return (int64_t)(((uint64_t)(uint32_t)AL_U((uint32_t)((uint64_t)v >> 32)) << 32) | (uint32_t)AL_U((uint32_t)(uint64_t)v));
}

// the learn rule for the pair (A, B): the match with the greatest bitpos in B (of several, the one with the greatest bitpos in A).
// Returns true if there is a match; then d = bitpos_B - bitpos_A.  Wave-uniform result.
__device__ __forceinline__ bool al_pair(uint32_t kind, const AlMember &A, const AlMember &B, int lane, int64_t &d)
{
	int64_t bb = -1, ba = -1;                          // bitpos < 2^63
	for (uint32_t j = (uint32_t)lane; j <= B.cnt; j += 64) {
		const SondeFrame *fb = al_cand(B, j);
		if (!al_good(kind, fb)) continue;
		const int64_t pb = (int64_t)fb->bitpos;
		if (pb < bb) continue;
		for (uint32_t i = 0; i <= A.cnt; i++) {
			const SondeFrame *fa = al_cand(A, i);
			if (!al_good(kind, fa) || !al_match(kind, fa, fb)) continue;
			const int64_t pa = (int64_t)fa->bitpos;
			if (pb > bb || pa > ba) { bb = pb; ba = pa; }
		}
	}
#pragma unroll
	for (int sh = 32; sh >= 1; sh >>= 1) {
		const int64_t ob = __shfl_xor((long long)bb, sh, 64), oa = __shfl_xor((long long)ba, sh, 64);
		if (ob > bb || (ob == bb && oa > ba)) { bb = ob; ba = oa; }
	}
	bb = al_u64(bb); ba = al_u64(ba);
	d = bb - ba;
	return bb >= 0;
}

// The align step of one group (SPEC 3.3k) of the given kind.  M[m], m < nm: the members; st: the group's state, read and written by
// this wave alone.  Inlined into each kernel: where the kernel knows the kind when it is compiled, the predicates fold to that kind's.
__device__ __forceinline__ void al_group(uint32_t kind, AlMember (&M)[SD_DIV_MAX], int nm, SdDivState *st, uint32_t mode, int lane)
{
	int64_t off[SD_DIV_MAX];
#pragma unroll
	for (int m = 0; m < SD_DIV_MAX; m++) off[m] = al_u64(st->off[m]);
	uint32_t locked = (uint32_t)AL_U(st->locked), learned = 0, dups = 0;
	if (mode & SONDE_DIVERSITY_LEARN) {
#pragma unroll
		for (int a = 0; a < SD_DIV_MAX - 1; a++) {
#pragma unroll
			for (int b = a + 1; b < SD_DIV_MAX; b++) {
				if (b >= nm) continue;
				int64_t d;
				if (!al_pair(kind, M[a], M[b], lane, d)) continue;
				const bool la = (locked >> a) & 1u, lb = (locked >> b) & 1u;
				if (lb && !la) { off[a] = off[b] - d; learned++; }
				else if (!la || !lb || off[b] - off[a] != d) { off[b] = off[a] + d; learned++; }
				locked |= (1u << a) | (1u << b);
			}
		}
	}
	if (mode & SONDE_DIVERSITY_MARK_DUPLICATES) {
#pragma unroll
		for (int b = 0; b < SD_DIV_MAX; b++) {
			if (b >= nm) continue;
			for (uint32_t j0 = 0; j0 < M[b].cnt; j0 += 64) {
				const uint32_t j = j0 + (uint32_t)lane;
				bool dup = false;
				if (j < M[b].cnt && al_good(kind, M[b].recs + j)) {
					const SondeFrame *fb = M[b].recs + j;
#pragma unroll
					for (int a = 0; a < SD_DIV_MAX; a++) {
						if (a >= nm || a == b || dup) continue;
						if (al_good(kind, M[a].carried) && al_match(kind, M[a].carried, fb)) dup = true;
						for (uint32_t i = 0; a < b && !dup && i < M[a].cnt; i++)
							dup = al_good(kind, M[a].recs + i) && al_match(kind, M[a].recs + i, fb);
					}
					if (dup) M[b].recs[j].flags |= SONDE_FRAME_DUPLICATE;
				}
				dups += (uint32_t)__popcll(__ballot(dup));
			}
		}
	}
	if (lane == 0) {
#pragma unroll
		for (int m = 0; m < SD_DIV_MAX; m++) st->off[m] = off[m];
		st->locked = locked;
		st->learned += learned;
		st->duplicates += dups;
	}
}

// OTHER_KINDS = false: every group of the table is RS41 -- the kind word is not read and the code is the RS41 step alone; true: the
// table has groups of SPEC 3.3l, and each group's kind is read from the table.  The host launches the one that fits the table.
template <bool OTHER_KINDS> __global__ __launch_bounds__(64) void sd_diversity_align_kernel(SondeFrame *frames, const uint32_t *__restrict__ counts,
	uint32_t max_frames, const SdDivGroup *__restrict__ groups, const SondeFrame *__restrict__ carried, SdDivState *states, uint32_t mode)
{
	const uint32_t g = blockIdx.x;
	const int lane = (int)threadIdx.x;
	const SdDivGroup *G = groups + g;
	const int nm = AL_U(G->n);
	AlMember M[SD_DIV_MAX];
#pragma unroll
	for (int m = 0; m < SD_DIV_MAX; m++) {
		const uint32_t ch = m < nm ? (uint32_t)AL_U(G->ch[m]) : 0u;
		M[m].recs = frames + (size_t)ch * max_frames;
		M[m].cnt = m < nm ? (uint32_t)AL_U(min(counts[ch], max_frames)) : 0u;
		M[m].carried = carried + (size_t)SD_DIV_MAX * g + m;
	}
	al_group(OTHER_KINDS ? (uint32_t)AL_U(G->kind) : (uint32_t)SONDE_RS41, M, nm, states + g, mode, lane);
}

void sd_launch_diversity_align(const SdDivArgs &a, uint32_t mode)
{
	const auto kernel = a.other_kinds ? sd_diversity_align_kernel<true> : sd_diversity_align_kernel<false>;
	hipLaunchKernelGGL(kernel, dim3(a.n_groups), dim3(64), 0, a.stream, a.frames, a.counts, a.max_frames, a.groups, a.carried, a.states, mode);
}

// ---- test introspection: the align step alone on caller-made records (sonde_batch_test_diversity_align: RS41;
// sonde_batch_test_diversity_align_kind: any kind a group can have; OTHER_KINDS as above, so that the RS41 kernel stays what it was).
// One wave per case; case k has SD_DIV_MAX members of max_rec record slots each (counts[4 k + m] <= max_rec in use), SD_DIV_MAX carried records, its state and
// its mode; the host has checked n_members (2..4), the counts and the modes.
template <bool OTHER_KINDS> __global__ __launch_bounds__(64) void sd_diversity_align_unit_kernel(SondeFrame *records, const uint32_t *__restrict__ counts, uint32_t max_rec,
	const uint32_t *__restrict__ n_members, const SondeFrame *__restrict__ carried, SdDivState *states, const uint32_t *__restrict__ modes, uint32_t kind)
{
	const uint32_t k = blockIdx.x;
	const int lane = (int)threadIdx.x;
	const int nm = AL_U(n_members[k]);
	AlMember M[SD_DIV_MAX];
#pragma unroll
	for (int m = 0; m < SD_DIV_MAX; m++) {
		M[m].recs = records + ((size_t)SD_DIV_MAX * k + m) * max_rec;
		M[m].cnt = m < nm ? (uint32_t)AL_U(min(counts[SD_DIV_MAX * k + m], max_rec)) : 0u;
		M[m].carried = carried + (size_t)SD_DIV_MAX * k + m;
	}
	al_group(OTHER_KINDS ? (uint32_t)AL_U(kind) : (uint32_t)SONDE_RS41, M, nm, states + k, (uint32_t)AL_U(modes[k]), lane);
}

void sd_launch_diversity_align_unit(uint32_t n, hipStream_t stream, SondeFrame *records, const uint32_t *counts, uint32_t max_rec,
	const uint32_t *n_members, const SondeFrame *carried, SdDivState *states, const uint32_t *modes, uint32_t kind)
{
	if (kind != SONDE_RS41) hipLaunchKernelGGL(sd_diversity_align_unit_kernel<true>, dim3(n), dim3(64), 0, stream, records, counts, max_rec, n_members, carried, states, modes, kind);
	else hipLaunchKernelGGL(sd_diversity_align_unit_kernel<false>, dim3(n), dim3(64), 0, stream, records, counts, max_rec, n_members, carried, states, modes, kind);
}
