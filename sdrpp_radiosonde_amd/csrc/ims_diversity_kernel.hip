// ims_diversity_kernel.hip -- sonde_batch_set_diversity for iMS-100 / RS-11G groups (SONDE_FLAG_IMS_DIVERSITY, DESIGN SPEC 3.3n): the pass
// over the frame records of a submit that sees every receiver of one sonde.  An iMS-100 frame is 12 blocks of BCH(46,34), t = 2, and
// no frame check; a record keeps a rejected block's 34 data bits as received, without its parity bits, and does not say which blocks
// were rejected.  So this is the combining pass that reads CHIPS: every copy's 12 received blocks come from its own channel's bit ring
// (sd_ims_block.h, shared with ims_rescue_kernel.hip), the carried record's too.  A block rejected in the record to rewrite is taken
// from the partners that accepted it, if every copy that rejected it lies within 5 bits of that codeword; a block rejected in every
// copy is the bitwise majority of the received blocks, the positions without a majority (at most 6) tried both ways.  A frame is
// rewritten only if every rejected block decodes, and only if the copies agree on their accepted blocks (the pairing guard).
//   one 64-lane wave per group, four waves per workgroup.  The loop over a group is dv_walk of sd_diversity_scan.h; this file is its
//   pass IdPass, whose attempt begins with step 3 and leaves a record uncounted where the chips do not serve.  Lane 12 j + L
//   (48 lanes) rebuilds block L of copy j and holds its syndromes, verdict and codeword; the block sets A, D, F are ballots; for a block
//   rejected everywhere the 64 lanes are the hypotheses, as in iq_decode_block.  LDS: each wave's own copy of the 192-byte GF(2^6) table.
// Runs behind every other kernel of the submit (SONDE_FLAG_IMS_RESCUE's pass included), behind the align step and the other combining
// kernels (they take disjoint groups), on the stream where the submit completes, and rewrites records in place.  What one lane wrote
// to a record and another reads later (a rewritten record's nerr, the carried copy) is ordered by a fence and read with agent-scope
// loads.  Vector stores only.  Bounds: min(counts, max_frames) records per member, 4 slots per group, 12 blocks per copy; every ring
// index is masked with ring_words - 1 (a power of two), every channel is one of the group table's.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_diversity_scan.h"
#include "sd_ims_block.h"
#include "launch.h"

constexpr int ID_LEN = 51;            // bytes of an iMS-100 record: 12 x 34 data bits
constexpr int ID_MIN_AGREED = 6;      // SPEC 3.3n step 4: blocks accepted in every copy, at least
constexpr int ID_MAX_DIFFER = 1;      // ... and of those, blocks whose codewords are not all equal, at most
constexpr int ID_MAX_DIST = 5;        // step 5a: a copy that rejected the block lies at most this far from the partners' codeword
constexpr int ID_CAP = 6;             // step 5b: positions without a majority, at most

// the 12-bit sets of a ballot over lanes 12 j + L, one per copy, folded into one: blocks for which the predicate holds in SOME copy
__device__ __forceinline__ uint32_t id_fold(unsigned long long m) { return (uint32_t)(m | m >> 12 | m >> 24 | m >> 36) & 0xFFFu; }

// Steps 4 to 6 of SPEC 3.3n.  Lane 12 j + L holds block L of copy j: blk as received, rej = the first pass rejects it, cw = else the
// codeword it made of it; valid: bit j = copy j takes part (bit 0 always; wave-uniform), K = their number.  Wave-synchronous, every
// branch around a ballot or a shuffle wave-uniform, all 64 lanes active.  Returns K (accepted: fm = the blocks of F, lane L < 12 holds
// in v the value of block L; add = the bits in which the values differ from copy 0's received blocks; nj = the blocks decoded by 5b),
// -1 (the pairing guard refuses), -2 (a block has no solution) or -3 (none has none, one has several).
__device__ int id_combine(uint32_t valid, uint64_t blk, bool rej, uint64_t cw, int lane, const uint8_t *g_exp, const uint8_t *g_log,
	unsigned long long &fm, uint64_t &v, int &add, int &nj)
{
	const int j_mine = lane / IQ_BLOCKS, L_mine = lane - IQ_BLOCKS * j_mine;
	const bool active = lane < IQ_BLOCKS * SD_DIV_MAX && ((valid >> j_mine) & 1u);
	const int K = __popc(valid);
	fm = 0ull; v = 0ull; add = 0; nj = 0;
	// ---- 4. pairing guard
	const unsigned long long rejm = __ballot(active && rej), accm = __ballot(active && !rej);
	const uint64_t cw0 = iq_shfl64(cw, L_mine);
	const uint32_t in_a = ~id_fold(rejm) & 0xFFFu;
	const uint32_t in_d = id_fold(__ballot(active && !rej && cw != cw0)) & in_a;
	if (__popc(in_a) < ID_MIN_AGREED || __popc(in_d) > ID_MAX_DIFFER) return -1;

	// ---- 5. the blocks copy 0 rejected, one by one; everything wave-uniform but the hypotheses of 5b
	fm = rejm & 0xFFFull;
	bool several = false;
	for (unsigned long long m = fm; m; m &= m - 1ull) {
		const int L = __builtin_ctzll(m);
		uint64_t x[SD_DIV_MAX], c[SD_DIV_MAX];                 // copy j's received block and codeword
		bool rj[SD_DIV_MAX], in[SD_DIV_MAX];
		bool held = false;
#pragma unroll
		for (int j = 0; j < SD_DIV_MAX; j++) {
			in[j] = (valid >> j) & 1u;
			x[j] = sd_readlane64(blk, IQ_BLOCKS * j + L);
			c[j] = sd_readlane64(cw, IQ_BLOCKS * j + L);
			rj[j] = !((accm >> (IQ_BLOCKS * j + L)) & 1ull);
			held = held || (in[j] && !rj[j]);
		}
		uint64_t val = 0;
		if (held) {
			// (a) the codeword most of the partners that accepted the block hold; a tie between different values: several
			int best = 0;
			bool tie = false;
#pragma unroll
			for (int j = 1; j < SD_DIV_MAX; j++) {
				if (!in[j] || rj[j]) continue;
				int n = 0;
#pragma unroll
				for (int k = 1; k < SD_DIV_MAX; k++) n += in[k] && !rj[k] && c[k] == c[j];
				if (n > best) { best = n; val = c[j]; tie = false; }
				else if (n == best && c[j] != val) tie = true;
			}
			if (tie) { several = true; continue; }
#pragma unroll
			for (int j = 0; j < SD_DIV_MAX; j++)
				if (in[j] && rj[j] && __popcll(x[j] ^ val) > ID_MAX_DIST) return -2;
		} else {
			// (b) rejected in every copy: the bitwise majority, the positions without one (V) as r has them
			uint64_t p[SD_DIV_MAX] = { x[0], 0ull, 0ull, 0ull };
			int n = 1;
#pragma unroll
			for (int j = 1; j < SD_DIV_MAX; j++) {
				if (!in[j]) continue;
				if (n == 1) p[1] = x[j]; else if (n == 2) p[2] = x[j]; else p[3] = x[j];
				n++;
			}
			uint64_t w, V;
			if (K == 2) { V = p[0] ^ p[1]; w = p[0]; }
			else if (K == 3) { V = 0ull; w = (p[0] & p[1]) | (p[0] & p[2]) | (p[1] & p[2]); }
			else {
				const uint64_t ab = p[0] & p[1], cd = p[2] & p[3], a_b = p[0] | p[1], c_d = p[2] | p[3];
				const uint64_t three = (ab & c_d) | (cd & a_b), two = ab | cd | (a_b & c_d);
				V = two & ~three; w = three | (V & p[0]);
			}
			uint32_t s1, s3;
			iq_syndromes(w, g_exp, s1, s3);
			const int nv = __popcll(V);
			if (nv == 0) {
				uint64_t e;
				if (iq_first_pass<true>(s1, s3, g_exp, g_log, e)) return -2;
				val = w ^ e;
			} else {
				if (nv > ID_CAP) return -2;
				// lane h: the subset of V whose i-th position is taken iff bit i of h is set
				uint64_t pat = 0, u = V;
#pragma unroll
				for (int i = 0; i < ID_CAP; i++) {
					if (!u) break;
					const int pos = __builtin_ctzll(u);
					u &= u - 1ull;
					if ((lane >> i) & 1) { pat ^= 1ull << pos; s1 ^= g_exp[pos]; s3 ^= g_exp[(3 * pos) % 63]; }
				}
				const unsigned long long fit = __ballot(lane < (1 << nv) && s1 == 0u && s3 == 0u);
				if (!fit) return -2;
				if (fit & (fit - 1ull)) { several = true; continue; }
				val = w ^ sd_readlane64(pat, __builtin_ctzll(fit));
			}
			nj++;
		}
		add += __popcll(val ^ x[0]);
		if (lane == L) v = val;
	}
	// ---- 6. all or nothing
	return several ? -3 : K;
}

// Step 7: the accepted result into the record
__device__ __forceinline__ void id_write_record(SondeFrame *fr, int K, unsigned long long fm, uint64_t v, int add, int nj, int lane)
{
	iq_write_blocks(fr, fm, v, lane);
	if (lane == 0) {
		fr->nerr[0] = (int)dv_load_fresh(reinterpret_cast<const uint32_t *>(&fr->nerr[0])) + add;
		fr->nerr[1] = 0;
		fr->flags = dv_load_fresh(&fr->flags) | SONDE_FRAME_RESCUED | SONDE_FRAME_COMBINED | ((uint32_t)K << 8) | ((uint32_t)min(nj, 15) << 12);
	}
}

// the wave's own copy of the GF(2^6) table (exp[128], log[64]); wave-private, so a fence and a wave barrier order it, as in sd_fixed.h
__device__ __forceinline__ void id_table(uint32_t *tab, const uint8_t *__restrict__ g64, int lane)
{
	if (lane < 48) tab[lane] = reinterpret_cast<const uint32_t *>(g64)[lane];
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// The pass of the walk (sd_diversity_scan.h).  A copy is where its chips are: channel, first chip, and the nerr[1] of its record
struct IdPass {
	const SdChanState *chan_states; const uint32_t *bitring; uint32_t ring_words;
	const uint8_t *g_exp, *g_log;
	uint32_t c_ch[SD_DIV_MAX];
	uint64_t c_pos[SD_DIV_MAX];
	int c_bad[SD_DIV_MAX];
	static constexpr uint32_t nerr = 2;
	__device__ __forceinline__ bool takes(const SdDivGroup *G, uint32_t &kind) const
	{
		kind = SONDE_IMS100;
		return (uint32_t)DV_U(G->kind) == SONDE_IMS100;
	}
	__device__ __forceinline__ int flen(const SondeFrame *) const { return ID_LEN; }
	__device__ __forceinline__ void partner(int K, const SondeFrame *pf, uint32_t ch, int, int bad, int, int)
	{
		dv_set_copy(c_ch, K, ch);
		dv_set_copy(c_pos, K, (uint64_t)sd_uniform64(pf->bitpos));
		dv_set_copy(c_bad, K, bad);
	}
	// the copies: r first, then the failed partners in member order
	__device__ __forceinline__ int attempt(SondeFrame *fr, uint32_t ch, int nc, int, int lane)
	{
		c_ch[0] = ch; c_pos[0] = sd_uniform64(fr->bitpos);
		c_bad[0] = DV_U(dv_load_fresh(reinterpret_cast<const uint32_t *>(&fr->nerr[1])));
		// ---- 3. lane 12 j + L: block L of copy j from the chips of its channel's ring, and the first pass's verdict on it
		const int j_mine = lane / IQ_BLOCKS, L_mine = lane - IQ_BLOCKS * j_mine;
		const uint32_t my_ch = dv_copy_of(c_ch, j_mine);
		const uint64_t my_pos = dv_copy_of(c_pos, j_mine);
		uint64_t blk = 0, cw = 0;
		bool rej = false, held = false;
		if (j_mine < nc) {
			const SdRing ring = { bitring + (size_t)my_ch * ring_words, ring_words, chan_states[my_ch].wpos };
			held = sd_ring_holds(ring, my_pos, IQ_FRAME_CHIPS);
			if (held) {
				uint64_t viol, e;
				uint32_t s1, s3;
				iq_rebuild_block(ring, my_pos, L_mine, blk, viol);
				iq_syndromes(blk, g_exp, s1, s3);
				rej = iq_first_pass<true>(s1, s3, g_exp, g_log, e);
				cw = rej ? blk : blk ^ e;
			}
		}
		const unsigned long long heldm = __ballot(held), rejm = __ballot(rej);
		uint32_t valid = 0;
#pragma unroll
		for (int j = 0; j < SD_DIV_MAX; j++)         // a copy takes part if its chips are held and they say what its record says
			if (j < nc && ((heldm >> (IQ_BLOCKS * j)) & 1ull) && __popcll((rejm >> (IQ_BLOCKS * j)) & 0xFFFull) == dv_copy_of(c_bad, j)) valid |= 1u << j;
		if (!(valid & 1u) || __popc(valid) < 2) return DV_SKIPPED;      // r itself, or fewer than two copies: stays as recorded, not counted
		unsigned long long fm;
		uint64_t v;
		int add, nj;
		const int st = id_combine(valid, blk, rej, cw, lane, g_exp, g_log, fm, v, add, nj);
		if (st <= 0) return DV_TRIED;
		id_write_record(fr, st, fm, v, add, nj, lane);
		return DV_COMBINED;
	}
	__device__ __forceinline__ void sync() const {}
};

__global__ __launch_bounds__(64 * DV_WAVES) void sd_ims_diversity_kernel(SdDivWalk a, const SdChanState *__restrict__ chan_states,
	const uint32_t *__restrict__ bitring, uint32_t ring_words, const uint8_t *__restrict__ g64)
{
	__shared__ uint32_t s_g64[DV_WAVES][48];
	uint32_t *const tab = s_g64[threadIdx.x >> 6];
	id_table(tab, g64, threadIdx.x & 63);
	const uint8_t *g_exp = reinterpret_cast<const uint8_t *>(tab);
	IdPass pass = { chan_states, bitring, ring_words, g_exp, g_exp + 128, { 0u, 0u, 0u, 0u }, { 0ull, 0ull, 0ull, 0ull }, { 0, 0, 0, 0 } };
	dv_walk(a, pass);
}

void sd_launch_ims_diversity(const SdDivArgs &a) { dv_launch(sd_ims_diversity_kernel, a, a.chan_states, a.bitring, a.ring_words, a.fec.g64); }

// ---- test introspection: steps 4 to 7 alone on caller-made cases (sonde_batch_test_ims_combine).  One wave per case: copy 0's record,
// n_copies and the copies' received blocks [SD_DIV_MAX][12] (bit b of a block = coefficient 45 - b).  The host has checked n_copies
// (2..4), the record's type and len and that it has failed.  status 0: the record's nerr[1] is not the number of blocks the first pass
// rejects among copy 0's (SPEC step 3: the record stays, nothing is tried).
__global__ __launch_bounds__(64 * DV_WAVES) void sd_ims_diversity_unit_kernel(
	const SondeFrame *__restrict__ records, const uint32_t *__restrict__ n_copies, const uint64_t *__restrict__ blocks, uint32_t n,
	SondeFrame *out, int32_t *__restrict__ status, const uint8_t *__restrict__ g64)
{
	__shared__ uint32_t s_g64[DV_WAVES][48];
	const int lane = threadIdx.x & 63;
	uint32_t k;
	if (!dv_unit_case(k, n, records, 1, out, lane)) return;
	uint32_t *const tab = s_g64[threadIdx.x >> 6];
	id_table(tab, g64, lane);
	const uint8_t *g_exp = reinterpret_cast<const uint8_t *>(tab), *g_log = g_exp + 128;
	const int K = DV_U(n_copies[k]);
	uint64_t blk = 0, cw = 0;
	bool rej = false;
	if (lane < IQ_BLOCKS * K) {
		uint64_t e;
		uint32_t s1, s3;
		blk = blocks[(size_t)IQ_BLOCKS * SD_DIV_MAX * k + lane] & IQ_BLK_MASK;
		iq_syndromes(blk, g_exp, s1, s3);
		rej = iq_first_pass<true>(s1, s3, g_exp, g_log, e);
		cw = rej ? blk : blk ^ e;
	}
	int st = 0;
	if (__popcll(__ballot(rej) & 0xFFFull) == DV_U(records[k].nerr[1])) {
		unsigned long long fm;
		uint64_t v;
		int add, nj;
		st = id_combine((1u << K) - 1u, blk, rej, cw, lane, g_exp, g_log, fm, v, add, nj);
		if (st > 0) id_write_record(out + k, st, fm, v, add, nj, lane);
	}
	if (lane == 0) status[k] = st;
}

void sd_launch_ims_diversity_unit(const SdDivUnitArgs &a)
{
	hipLaunchKernelGGL(sd_ims_diversity_unit_kernel, dim3((a.n + DV_WAVES - 1) / DV_WAVES), dim3(64 * DV_WAVES), 0, a.stream,
		a.copies, a.n_copies, a.blocks, a.n, a.out, a.status, a.fec.g64);
}
