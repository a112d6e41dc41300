// sd_rsee.h -- RS(255,231) errors-AND-erasures decoding of one codeword by one 64-lane wave (DESIGN SPEC 3.3c): the second pass
// behind sd_rsdec.h's errors-only corrector, for RS41 frames whose damaged blocks are known from their CRCs (rescue_kernel.hip).
//   bounded distance: 2 v + e <= 24 (v unknown errors outside the e erased positions), roots alpha^0..alpha^23, coefficient k of
//   the word at position k -- the code of sd_rsdec.h.  Stages, one coefficient / position / erratum per lane, products in the
//   log domain through FramerTabs (sd_rsdec.h), WAVE_SYNC() between stages:
//     erasure list -> Gamma(x) = prod (1 + X_k x) -> T = Gamma S mod x^24 -> Berlekamp-Massey over T_e..T_23 -> Chien over the
//     non-erased positions -> Psi = Lambda Gamma, Omega = Psi S mod x^24 -> Forney over erasures and errors together ->
//     the corrected word's syndromes must be zero (what guards a decode at e = 24, where the code has no redundancy left).
// A bounded-distance decision is unique: a word decodes iff a codeword exists that differs from it in erased positions and in v
// others with 2 v + e <= 24, and then the result is that codeword.  All integer / byte work.
#pragma once
#include "sd_rsdec.h"

struct RseeLds {                   // one per wave, beside its FramerLds
	alignas(4) uint8_t er[2][256];     // 1: position erased
	uint16_t lgam[RS_R + 2];           // logarithms of Gamma_0..Gamma_25
	uint16_t llam[RS_T + 2];           // ... of Lambda_0..Lambda_12
	uint16_t lT[RS_R];                 // ... of the modified syndromes
	uint16_t lpsi[RS_R + 2];           // ... of Psi_0..Psi_25
	uint16_t lom[RS_R];                // ... of Omega_0..Omega_23
	int      pos[RS_R + RS_T + 4];     // errata positions: the erasures, then the errors
};

// syndromes of both codewords (s.cw[c][0..n), zero-padded to 256) into s.logS: lane = 24 c + j.  Returns the ballot of non-zero ones.
__device__ __forceinline__ unsigned long long rsee_syndromes(const FramerTabs &tb, FramerLds &s, int n, int lane, const GfSwar &swar)
{
	uint32_t syn = 0;
	if (lane < 2 * RS_R) {
		const int c = lane / RS_R, j = lane % RS_R;
		syn = syndrome_swar(tb, s.cw[c], (n + 3) >> 2, j, swar);
		s.logS[c][j] = tb.log2[syn];
	}
	const unsigned long long nz = __ballot(syn != 0);
	WAVE_SYNC();
	return nz;
}

__device__ __forceinline__ uint32_t rsee_wave_xor(uint32_t v)
{
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m, 64);
	return v;
}

// Codeword c of the pair: s.cw[c][0..n) with s.logS[c] its syndromes and x.er[c] its erasure flags (positions >= n are not looked
// at).  Wave-synchronous, 64 lanes, every branch wave-uniform.  Returns -1 (no codeword within the bound, or more than 24
// erasures: the word is left as it was) or the number of bytes it changed (0: the word was a codeword already).
__device__ int rsee_decode_one(const FramerTabs &tb, FramerLds &s, RseeLds &x, int c, int n, int lane, const GfSwar &swar)
{
	uint8_t *cw = s.cw[c];
	const uint8_t *er = x.er[c];
	const uint16_t *lS = s.logS[c];
	// ---- erasure list, in ascending position
	int e = 0;
	for (int it = 0; it < 4; it++) {
		const int i = lane + 64 * it;
		const bool f = i < n && er[i] != 0;
		const unsigned long long m = __ballot(f);
		const int slot = e + __popcll(m & ((1ull << lane) - 1ull));
		if (f && slot <= RS_R) x.pos[slot] = i;
		e += __popcll(m);
	}
	if (e > RS_R) return -1;
	if (__ballot(lane < RS_R && lS[lane] != GF_LZ) == 0ull) return 0;
	WAVE_SYNC();
	// ---- Gamma(x) = prod_k (1 + alpha^p_k x): lane i holds Gamma_i
	uint32_t g = lane == 0 ? 1u : 0u;
	for (int q = 0; q < e; q++) {
		const uint32_t p = (uint32_t)x.pos[q];
		const uint32_t sh = (uint32_t)__shfl_up((int)g, 1, 64);       // (every lane takes part: a cross-lane read under `lane ?` would find lane 0 switched off)
		const uint32_t up = lane ? sh : 0u;
		g ^= tb.exp2[(uint32_t)tb.log2[up] + p];
	}
	if (lane < RS_R + 2) x.lgam[lane] = tb.log2[g];
	WAVE_SYNC();
	// ---- modified syndromes T = Gamma S mod x^24: T_e..T_23 obey the error locator's recurrence alone
	if (lane < RS_R) {
		uint32_t t = 0;
		const int kmax = lane < e ? lane : e;
		for (int k = 0; k <= kmax; k++) t ^= tb.exp2[(uint32_t)x.lgam[k] + (uint32_t)lS[lane - k]];
		x.lT[lane] = tb.log2[t];
	}
	WAVE_SYNC();
	// ---- Berlekamp-Massey over U_m = T_{e+m}, m < N = 24 - e (started from the erasure count): lane i holds C_i and B_i, B kept
	// shifted (one lane up per step), the discrepancy is a wave-wide xor of one product per lane
	const int N = RS_R - e;
	uint32_t Cv = lane == 0 ? 1u : 0u, Bv = Cv, lb = 0u;
	int L = 0;
	for (int r = 0; r < N; r++) {
		const uint32_t term = (lane <= r && lane <= L) ? (uint32_t)tb.exp2[(uint32_t)tb.log2[Cv] + (uint32_t)x.lT[e + r - lane]] : 0u;
		const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)rsee_wave_xor(term));      // wave-uniform: so are L and every branch below
		const uint32_t Bsh = (uint32_t)__shfl_up((int)Bv, 1, 64);
		const uint32_t Bs = lane ? Bsh : 0u;
		if (d == 0u) {
			Bv = Bs;
		} else {
			const uint32_t ld = tb.log2[d];
			const uint32_t Cn = Cv ^ (uint32_t)tb.exp2[ld + 255u - lb + (uint32_t)tb.log2[Bs]];
			if (2 * L <= r) { Bv = Cv; lb = ld; L = r + 1 - L; }
			else Bv = Bs;
			Cv = Cn;
		}
	}
	{
		const unsigned long long nzl = __ballot(Cv != 0u);
		const int deg = 63 - __clzll((long long)nzl);            // C_0 = 1: never empty
		if (2 * L > N || deg != L) return -1;
	}
	if (lane < RS_T + 2) x.llam[lane] = tb.log2[Cv];
	WAVE_SYNC();
	// ---- Chien search over the non-erased positions of [0, n): L roots there, or no codeword within the bound
	int nroot = 0;
	if (L > 0) {
		for (int it = 0; it < 4; it++) {
			const uint32_t i = (uint32_t)(lane + 64 * it);
			const uint32_t st = (i && i < 255u) ? 255u - i : 0u;
			uint32_t v = 0, ex = 0;
			for (int k = 0; k <= L; k++) {
				v ^= tb.exp2[(uint32_t)x.llam[k] + ex];
				ex += st;
				if (ex >= 255u) ex -= 255u;
			}
			const bool root = (int)i < n && er[i] == 0 && v == 0u;
			const unsigned long long m = __ballot(root);
			const int slot = nroot + __popcll(m & ((1ull << lane) - 1ull));
			if (root && slot < RS_T) x.pos[e + slot] = (int)i;
			nroot += __popcll(m);
		}
	}
	if (nroot != L) return -1;
	// ---- errata locator Psi = Lambda Gamma (degree e + L <= 24), evaluator Omega = Psi S mod x^24
	if (lane < RS_R + 2) {
		uint32_t p = 0;
		const int kmax = lane < L ? lane : L;
		for (int k = 0; k <= kmax; k++) p ^= tb.exp2[(uint32_t)x.llam[k] + (uint32_t)x.lgam[lane - k]];
		x.lpsi[lane] = tb.log2[p];
	}
	WAVE_SYNC();
	if (lane < RS_R) {
		uint32_t om = 0;
		for (int k = 0; k <= lane; k++) om ^= tb.exp2[(uint32_t)x.lpsi[k] + (uint32_t)lS[lane - k]];
		x.lom[lane] = tb.log2[om];
	}
	WAVE_SYNC();
	// ---- Forney, one erratum per lane: value = X Omega(X^-1) / Psi'(X^-1)
	const int nerrata = e + L;
	bool bad = false;
	uint32_t ev = 0;
	int p = 0;
	if (lane < nerrata) {
		p = x.pos[lane];
		const uint32_t xi = p ? 255u - (uint32_t)p : 0u;
		uint32_t num = 0, den = 0, ex = 0;
		for (int k = 0; k < RS_R; k++) {
			num ^= tb.exp2[(uint32_t)x.lom[k] + ex];
			ex += xi;
			if (ex >= 255u) ex -= 255u;
		}
		uint32_t xi2 = 2u * xi;
		if (xi2 >= 255u) xi2 -= 255u;
		ex = 0;
		for (int k = 1; k < RS_R + 2; k += 2) {
			den ^= tb.exp2[(uint32_t)x.lpsi[k] + ex];
			ex += xi2;
			if (ex >= 255u) ex -= 255u;
		}
		if (!den) bad = true;
		else ev = tb.exp2[(uint32_t)p + (uint32_t)tb.log2[num] + 255u - (uint32_t)tb.log2[den]];
	}
	if (__ballot(bad) != 0ull) return -1;
	if (lane < nerrata) cw[p] ^= (uint8_t)ev;
	WAVE_SYNC();
	// ---- the result must be a codeword
	uint32_t syn = 0;
	if (lane < RS_R) syn = syndrome_swar(tb, cw, (n + 3) >> 2, lane, swar);
	if (__ballot(syn != 0u) != 0ull) {
		if (lane < nerrata) cw[p] ^= (uint8_t)ev;       // as it was
		WAVE_SYNC();
		return -1;
	}
	return __popcll(__ballot(ev != 0u));
}
