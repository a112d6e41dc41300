// dfm_diversity_kernel.hip -- sonde_batch_set_diversity for DFM groups (DESIGN SPEC 3.3m): the pass over the frame records of a submit
// that sees every receiver of one sonde.  A DFM frame is 33 Hamming(8,4) words and no frame check; a record keeps a word the first pass
// gave up on as received and every other word as a codeword (SPEC 3.3g step 2), so the syndrome of a record's byte says whether the word
// failed in that copy, and the pass needs the records alone.  A word that failed in the record to rewrite is taken from the partners
// that hold it as a codeword, or -- where it failed in every copy -- is the one codeword two bits away from every copy's word; a frame
// is rewritten only if every failed word decodes, and only if the copies agree on their good words (the pairing guard: DFM has no
// check behind the code that would catch copies of two different frames).
//   one 64-lane wave per group, four waves per workgroup.  The loop over a group -- the next failed record and its partners, this
//   submit's records plus the carried one, the counters, the carried records -- is dv_walk of sd_diversity_scan.h; this file is its
//   pass DdPass.  Lane i < 33 holds byte i of every copy: the syndromes are
//   parities of masked bytes, the 16 codewords are made from their nibbles in registers, and step 4 is lane-local; the word sets A, D, F,
//   none and several are ballots.  No LDS, no tables in memory.
// Runs behind every other kernel of the submit, behind the align step and the other two combining kernels (they take disjoint groups),
// on the stream where the submit completes, and rewrites records in place.  What one lane wrote to a record and another reads later (a
// rewritten record's nerr, the carried copy) is ordered by a fence and read with agent-scope loads.  Vector stores only.  Bounds:
// min(counts, max_frames) records per member, 4 slots per group, every byte index < 33.
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "sd_diversity_scan.h"
#include "launch.h"

constexpr int DD_WORDS = 33;          // Hamming(8,4) words of a DFM frame = bytes of its record
constexpr int DD_MIN_AGREED = 17;     // SPEC 3.3m step 3: words that are codewords in every copy, at least
constexpr int DD_MAX_DIFFER = 2;      // ... and of those, words on which the copies differ, at most

// byte `lane` of a record's frame, zero behind the frame
__device__ __forceinline__ uint32_t dd_byte(const SondeFrame *f, int lane) { return lane < DD_WORDS ? (uint32_t)f->data[lane] : 0u; }
// a codeword: all four parity rows (0x78 / 0xB4 / 0xD2 / 0xE1) close
__device__ __forceinline__ bool dd_codeword(uint32_t b)
{
	return ((__popc(b & 0x78u) | __popc(b & 0xB4u) | __popc(b & 0xD2u) | __popc(b & 0xE1u)) & 1) == 0;
}
// the codeword of a data nibble: the nibble in the high half, each parity bit closing one row
__device__ __forceinline__ uint32_t dd_encode(uint32_t nib)
{
	const uint32_t w = nib << 4;
	return w | ((__popc(w & 0x70u) & 1u) << 3) | ((__popc(w & 0xB0u) & 1u) << 2) | ((__popc(w & 0xD0u) & 1u) << 1) | (__popc(w & 0xE0u) & 1u);
}

// Steps 3 to 5 of SPEC 3.3m on K copies; x[j]: this lane's byte of copy j (copy 0 is the record to rewrite; x[j] for j >= K is not
// looked at).  Wave-synchronous, every branch around a ballot wave-uniform, all 64 lanes active.  Returns K (accepted: in_f = this
// lane's word is rewritten, to v; nf = |F|, nj = the words decoded jointly), -1 (the pairing guard refuses), -2 (a word has no solution)
// or -3 (none has none, one has several).
__device__ int dd_combine(int K, const uint32_t (&x)[SD_DIV_MAX], int lane, bool &in_f, uint32_t &v, int &nf, int &nj)
{
	// ---- 3. pairing guard
	const bool in = lane < DD_WORDS;
	bool cw[SD_DIV_MAX], all_cw = in, all_eq = true;
#pragma unroll
	for (int j = 0; j < SD_DIV_MAX; j++) {
		cw[j] = j < K && dd_codeword(x[j]);
		if (j < K) { all_cw = all_cw && cw[j]; all_eq = all_eq && x[j] == x[0]; }
	}
	const int n_a = __popcll(__ballot(all_cw)), n_d = __popcll(__ballot(all_cw && !all_eq));
	in_f = false; v = 0u; nf = 0; nj = 0;
	if (n_a < DD_MIN_AGREED || n_d > DD_MAX_DIFFER) return -1;

	// ---- 4. the words copy 0 does not hold as codewords, each in its own lane, over the 16 codewords
	in_f = in && !cw[0];
	int np = 0;                                    // partners that hold the word as a codeword
#pragma unroll
	for (int j = 1; j < SD_DIV_MAX; j++) np += cw[j] ? 1 : 0;
	int best = 0, nbest = 0, njoint = 0;
	uint32_t vbest = 0u, vjoint = 0u;
	bool best_ok = false;
	for (uint32_t nib = 0; nib < 16u; nib++) {
		const uint32_t c = dd_encode(nib);
		int votes = 0;
		bool two = true;                           // every copy that failed here lies two bits from c
#pragma unroll
		for (int j = 0; j < SD_DIV_MAX; j++) {
			if (j >= K) continue;
			if (cw[j]) votes += (j >= 1 && x[j] == c) ? 1 : 0;
			else two = two && __popc(x[j] ^ c) == 2;
		}
		if (votes > best) { best = votes; nbest = 1; vbest = c; best_ok = two; }
		else if (votes == best && votes > 0) nbest++;
		if (two) { njoint++; vjoint = c; }
	}
	bool none, several;
	if (np) { several = nbest > 1; none = !several && !best_ok; v = vbest; }        // (a)
	else { none = njoint == 0; several = njoint > 1; v = vjoint; }                  // (b)

	// ---- 5. all or nothing
	const uint64_t f_none = __ballot(in_f && none), f_several = __ballot(in_f && several);
	nf = __popcll(__ballot(in_f));
	nj = __popcll(__ballot(in_f && !np));
	if (f_none) return -2;
	if (f_several) return -3;
	return K;
}

// Step 6: the accepted result into the record (in_f: this lane's word is one of F, v its value)
__device__ __forceinline__ void dd_write_record(SondeFrame *fr, int K, bool in_f, uint32_t v, int nf, int nj, int lane)
{
	if (in_f) fr->data[lane] = (uint8_t)v;
	if (lane == 0) {
		fr->nerr[0] = (int)dv_load_fresh(reinterpret_cast<const uint32_t *>(&fr->nerr[0])) + nf;
		fr->nerr[1] = 0;
		fr->flags = dv_load_fresh(&fr->flags) | SONDE_FRAME_RESCUED | SONDE_FRAME_COMBINED | ((uint32_t)K << 8) | ((uint32_t)min(nj, 15) << 12);
	}
}

// The pass of the walk (sd_diversity_scan.h): lane i < 33 holds byte i of every copy in registers
struct DdPass {
	uint32_t x[SD_DIV_MAX];
	static constexpr uint32_t nerr = 2;
	__device__ __forceinline__ bool takes(const SdDivGroup *G, uint32_t &kind) const
	{
		kind = SONDE_DFM09;
		return (uint32_t)DV_U(G->kind) == SONDE_DFM09;
	}
	__device__ __forceinline__ int flen(const SondeFrame *) const { return DD_WORDS; }
	__device__ __forceinline__ void partner(int K, const SondeFrame *pf, uint32_t, int, int, int, int lane)
	{
		dv_set_copy(x, K, dd_byte(pf, lane));
	}
	__device__ __forceinline__ int attempt(SondeFrame *fr, uint32_t, int K, int, int lane)
	{
		x[0] = dd_byte(fr, lane);
		bool in_f;
		uint32_t v;
		int nf, nj;
		if (dd_combine(K, x, lane, in_f, v, nf, nj) <= 0) return DV_TRIED;
		dd_write_record(fr, K, in_f, v, nf, nj, lane);
		return DV_COMBINED;
	}
	__device__ __forceinline__ void sync() const {}
};

__global__ __launch_bounds__(64 * DV_WAVES) void sd_dfm_diversity_kernel(SdDivWalk a)
{
	DdPass pass = { { 0u, 0u, 0u, 0u } };
	dv_walk(a, pass);
}

void sd_launch_dfm_diversity(const SdDivArgs &a) { dv_launch(sd_dfm_diversity_kernel, a); }

// ---- test introspection: steps 3 to 6 alone on caller-made copies (sonde_batch_test_dfm_combine).  One wave per case; the host has
// checked n_copies (2..4), the copies' type (SONDE_DFM09) and len (33) and that copy 0 has failed.
__global__ __launch_bounds__(64 * DV_WAVES) void sd_dfm_diversity_unit_kernel(
	const SondeFrame *__restrict__ copies /* [n][SD_DIV_MAX] */, const uint32_t *__restrict__ n_copies, uint32_t n, SondeFrame *out,
	int32_t *__restrict__ status)
{
	const int lane = threadIdx.x & 63;
	uint32_t k;
	if (!dv_unit_case(k, n, copies, SD_DIV_MAX, out, lane)) return;
	const SondeFrame *cps = copies + (size_t)SD_DIV_MAX * k;
	const int K = DV_U(n_copies[k]);
	uint32_t x[SD_DIV_MAX];
#pragma unroll
	for (int j = 0; j < SD_DIV_MAX; j++) x[j] = j < K ? dd_byte(cps + j, lane) : 0u;
	bool in_f;
	uint32_t v;
	int nf, nj;
	const int st = dd_combine(K, x, lane, in_f, v, nf, nj);
	if (st > 0) dd_write_record(out + k, K, in_f, v, nf, nj, lane);
	if (lane == 0) status[k] = st;
}

void sd_launch_dfm_diversity_unit(const SdDivUnitArgs &a)
{
	hipLaunchKernelGGL(sd_dfm_diversity_unit_kernel, dim3((a.n + DV_WAVES - 1) / DV_WAVES), dim3(64 * DV_WAVES), 0, a.stream,
		a.copies, a.n_copies, a.n, a.out, a.status);
}
