// detect.hip -- the sonde type detector (SondeDetector, include/sonde_abi.h; SPEC DESIGN.md 3.8).
//
// One workgroup per channel, one launch per submit on the caller's stream.  Per submit the kernel
//   A  runs the GFSK front-end: 2:1 boxcar, discriminator (SPEC 3.1), quantiser -> D at 24 kS/s;
//   B  runs the AFSK front-end: discriminator at 48 kS/s, the two tone mixers with block sums of 8 and their boxcars (SPEC 3.6),
//      discriminator, quantiser -> A_imet, A_c50 at 6 kS/s;
//   C  correlates every template with every window that ends in this submit, in exact integers: per chunk of 2048 lags the
//      stream is turned into prefix sums P (uint32, wrapping) and P2 (uint64) in LDS, and since a template is constant per
//      chip, SD = sum over its chip boundaries of +-1 / +-2 times P at that boundary: one LDS read with an immediate offset and
//      one add per boundary and lag.  A float screen picks the lags that can beat the lane's best; only those take the
//      double division of the SPEC, so the reported best is the exact maximum.
// The quantised streams live in HBM behind a history of the longest template (a window that straddles two submits is
// found); `sonde_detect_read` copies this submit's part back for the tests.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "sonde_dev.h"
#include "sd_input.h"
#include "sd_math.h"
#include "sd_rs41.h"
#include "sd_fixed.h"
#include "launch.h"
#include "sd_host.h"
#include "sd_devmem.h"
#include "sd_tables.h"
#include "sd_chanlist.h"
#include "../../include/sonde_abi.h"

#define DT_WG   256
#define DT_T    2048                    // lags per chunk of the correlation
#define DT_H24  320                     // history of the 24 kS/s stream D (the longest template, RS41, is 320 samples)
#define DT_H6   64                      // history of the 6 kS/s streams (iMet-4: 60 samples)
#define DT_K    ((DT_T + DT_H24 - 1 + DT_WG - 1) / DT_WG)     // stream samples per thread in the prefix scan
#define DT_E    (DT_WG * DT_K)
#define DT_MAXPTS 72
#define DT_QSCALE 4096.0f               // quantiser: 2^-12 quadrant per count, clamp +-4 quadrants

// ---------------------------------------------------------------- templates (compile-time, from the framers' constants)
struct DtTmpl {
	int L;                      // samples at the stream rate
	int T1;                     // sum of s
	int npts;                   // SD = sum_p coef[p] * P[t + off[p]]
	int off[DT_MAXPTS];
	int coef[DT_MAXPTS];
	int nchips;
	int chip[64];               // +-1, sign applied
	int fs, baud, dec;          // stream rate, chip rate, input samples per stream sample
};

// chip j of type K's on-air sync (0 / 1), in air order
template <int K>
constexpr int dt_chip01(int j)
{
	if (K == SONDE_RS41) return (int)(((((uint64_t)RS41_SYNC_HI) << 32 | RS41_SYNC_LO) >> j) & 1u);   // 10 B6 CA 11 22 96 12 F8, LSB first
	if (K == SONDE_DFM09) return (int)((SyncTraits<SONDE_DFM09>::SYNC >> j) & 1u);                   // Manchester(0x45CF)
	if (K == SONDE_M10) return (int)((SyncTraits<SONDE_M10>::SYNC >> j) & 1u);
	if (K == SONDE_MRZN1) return (int)(((((uint64_t)SyncTraits<SONDE_MRZN1>::SYNC_HI) << 32 | SyncTraits<SONDE_MRZN1>::SYNC_LO) >> j) & 1u);
	if (K == SONDE_IMET4) return (int)((IMET_SYNC >> j) & 1u);
	if (K == SONDE_C50) return (int)((C50_SYNC >> j) & 1u);
	// iMS-100: biphase-S of the 24 bits 0x049DCE (bit k of the framer's word at chip 2k); first chip 1, a transition at every bit
	// boundary and a second one mid-bit for a 0
	const uint64_t w = ((uint64_t)SyncTraits<SONDE_IMS100>::SYNC_HI) << 32 | SyncTraits<SONDE_IMS100>::SYNC_LO;
	int lvl = 0, c = 0;
	for (int k = 0; k <= j / 2; k++) {
		lvl = k == 0 ? 1 : 1 - lvl;
		c = lvl;
		if (2 * k + 1 <= j) { if (!((w >> (2 * k)) & 1u)) lvl = 1 - lvl; c = lvl; }
	}
	return c;
}

template <int K>
constexpr DtTmpl dt_make()
{
	DtTmpl t{};
	t.nchips = K == SONDE_RS41 ? 64 : (K == SONDE_IMS100 || K == SONDE_MRZN1) ? 48 : K == SONDE_IMET4 ? IMET_SYNC_BITS : K == SONDE_C50 ? C50_SYNC_BITS : 32;
	t.baud = K == SONDE_DFM09 ? 5000 : K == SONDE_M10 ? 9600 : K == SONDE_IMET4 ? 1200 : K == SONDE_C50 ? 2400 : 4800;
	t.fs = (K == SONDE_IMET4 || K == SONDE_C50) ? 6000 : 24000;
	t.dec = SD_FS / t.fs;
	// upright = positive: a GFSK 1 is the upper frequency; iMet's mark (1200 Hz) lies below its 1700 Hz mixer, C50's (4700 Hz) above 3800 Hz
	const int sgn = K == SONDE_IMET4 ? -1 : 1;
	for (int j = 0; j < t.nchips; j++) t.chip[j] = sgn * (2 * dt_chip01<K>(j) - 1);
	t.L = (t.nchips * t.fs + t.baud - 1) / t.baud;                         // ceil(Nchips fs' / baud)
	// chip j covers [ceil(j fs'/baud), ceil((j+1) fs'/baud)): SD = -c0 P[0] + sum_(j>0, c_j != c_(j-1)) (c_(j-1) - c_j) P[b_j] + c_last P[L]
	t.T1 = 0;
	for (int n = 0; n < t.L; n++) t.T1 += t.chip[n * t.baud / t.fs];
	t.npts = 0;
	t.off[t.npts] = 0; t.coef[t.npts] = -t.chip[0]; t.npts++;
	for (int j = 1; j < t.nchips; j++) {
		if (t.chip[j] == t.chip[j - 1]) continue;
		t.off[t.npts] = (j * t.fs + t.baud - 1) / t.baud;
		t.coef[t.npts] = t.chip[j - 1] - t.chip[j];
		t.npts++;
	}
	t.off[t.npts] = t.L; t.coef[t.npts] = t.chip[t.nchips - 1]; t.npts++;
	return t;
}

// ---------------------------------------------------------------- per-channel state
struct SdDetState {
	float2   y_prev;            // GFSK branch: the last 2:1 boxcar output (IQ kinds)
	float2   x_prev;            // AFSK branch: the last input sample (IQ kinds)
	float2   bi[5];             // iMet block sums before the next one, oldest first
	float2   bc[2];             // SRS-C50 block sums
	uint64_t n;                 // input samples since create / reset
	double   best[SONDE_NTYPES];
	uint64_t pos[SONDE_NTYPES];
	uint32_t neg;               // bit k: type k's best has a negative sign
	uint32_t pad;
};

__device__ __forceinline__ int32_t dt_qz(float v)
{
	v = __builtin_fminf(__builtin_fmaxf(v, -4.0f), 4.0f);
	return (int32_t)__builtin_rintf(v * DT_QSCALE);
}

template <int KIND>      // sample i of a row of an IQ kind (sd_input.h)
__device__ __forceinline__ float2 dt_iq(const void *row, int64_t i) { return sd_iq_f2<KIND>(reinterpret_cast<const sd_iq_t<KIND> *>(row)[i]); }

struct DtLds {
	uint32_t P[DT_E + 1];
	uint64_t P2[DT_E + 1];
	uint64_t w2[DT_WG / 64];
	uint32_t w1[DT_WG / 64];
	double   rb[DT_WG / 64];
	uint32_t ru[DT_WG / 64];
	uint32_t rn[DT_WG / 64];
	float2   bi[DT_WG + 5];
	float2   bc[DT_WG + 2];
};

// (best, lag) of lane a beats lane b: larger |r|, then the earlier lag
__device__ __forceinline__ bool dt_better(double ba, uint32_t ua, double bb, uint32_t ub) { return ba > bb || (ba == bb && ua < ub); }

// One template against the prefix sums of the current chunk: lags u0 + tid + 256 i
template <int K>
__device__ __forceinline__ void dt_lags(const DtLds &s, uint32_t u0, uint32_t ncur, uint64_t m0, int H, double &lb, uint32_t &lu, uint32_t &ln)
{
	constexpr DtTmpl TP = dt_make<K>();
	constexpr int64_t Et = (int64_t)TP.L * TP.L - (int64_t)TP.T1 * TP.T1;
	const float lbf = (float)lb * (1.0f - 1.0f / 1024.0f);
#pragma unroll 2
	for (int i = 0; i < DT_T / DT_WG; i++) {
		const uint32_t ul = threadIdx.x + DT_WG * i;
		const uint32_t u = u0 + ul;
		if (u >= ncur) break;
		if (m0 + u + 1 < (uint64_t)TP.L) continue;                // the window starts before create / reset
		const uint32_t *p = s.P + (ul + H - TP.L);
		uint32_t sd = 0;
#pragma unroll
		for (int q = 0; q < TP.npts; q++) sd += (uint32_t)TP.coef[q] * p[TP.off[q]];
		const int32_t S1 = (int32_t)(p[TP.L] - p[0]);
		const uint64_t *p2 = s.P2 + (ul + H - TP.L);
		const int64_t S2 = (int64_t)(p2[TP.L] - p2[0]);
		const int64_t N = (int64_t)TP.L * (int32_t)sd - (int64_t)TP.T1 * S1;
		const int64_t Ed = (int64_t)TP.L * S2 - (int64_t)S1 * S1;
		if (Ed <= 0) continue;                                    // r = 0 never beats a best >= 0
		const float rf = __builtin_fabsf((float)N) * rsqrtf((float)Et * (float)Ed);
		if (rf < lbf) continue;
		const double r = (double)N / sqrt((double)Et * (double)Ed);
		if (fabs(r) > lb) { lb = fabs(r); lu = u; ln = r < 0.0; }
	}
}

// Block-wide reduction of one type's lane bests and the update of the channel's record (thread 0)
template <int K>
__device__ __forceinline__ void dt_commit(DtLds &s, SdDetState *st, uint64_t m0, double lb, uint32_t lu, uint32_t ln)
{
	constexpr DtTmpl TP = dt_make<K>();
	for (int o = 32; o > 0; o >>= 1) {
		const double ob = __shfl_xor(lb, o, 64);
		const uint32_t ou = (uint32_t)__shfl_xor((int)lu, o, 64), on = (uint32_t)__shfl_xor((int)ln, o, 64);
		if (dt_better(ob, ou, lb, lu)) { lb = ob; lu = ou; ln = on; }
	}
	const int w = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { s.rb[w] = lb; s.ru[w] = lu; s.rn[w] = ln; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int j = 1; j < DT_WG / 64; j++)
			if (dt_better(s.rb[j], s.ru[j], lb, lu)) { lb = s.rb[j]; lu = s.ru[j]; ln = s.rn[j]; }
		if (lb > st->best[K]) {
			st->best[K] = lb;
			st->pos[K] = (uint64_t)TP.dec * (m0 + lu + 1 - (uint64_t)TP.L);
			const uint32_t bit = 1u << K;
			st->neg = (ln && K != SONDE_IMS100) ? (st->neg | bit) : (st->neg & ~bit);     // iMS-100: differential code, no polarity
		}
	}
	__syncthreads();
}

// Prefix sums of the stream samples ext[u0 + 1 ..] of row (= [H history | ncur current]) into s.P / s.P2
__device__ __forceinline__ void dt_scan(DtLds &s, const int32_t *row, int H, uint32_t ncur, uint32_t u0)
{
	const int tid = threadIdx.x;
	const uint32_t lim = (uint32_t)H + ncur, E = DT_T + (uint32_t)H - 1;
	int32_t v[DT_K];
	uint32_t a1 = 0;
	uint64_t a2 = 0;
#pragma unroll
	for (int k = 0; k < DT_K; k++) {
		const uint32_t j = (uint32_t)tid * DT_K + k, e = u0 + 1 + j;
		v[k] = (j < E && e < lim) ? row[e] : 0;
		a1 += (uint32_t)v[k];
		a2 += (uint64_t)((int64_t)v[k] * v[k]);
	}
	// inclusive scan of the per-thread totals: within the wave, then over the waves
	uint32_t i1 = a1;
	uint64_t i2 = a2;
	const int lane = tid & 63;
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t t1 = (uint32_t)__shfl_up((int)i1, o, 64);
		const uint64_t t2 = (uint64_t)__shfl_up((long long)i2, o, 64);
		if (lane >= o) { i1 += t1; i2 += t2; }
	}
	if (lane == 63) { s.w1[tid >> 6] = i1; s.w2[tid >> 6] = i2; }
	__syncthreads();
	uint32_t b1 = i1 - a1;
	uint64_t b2 = i2 - a2;
	for (int w = 0; w < (tid >> 6); w++) { b1 += s.w1[w]; b2 += s.w2[w]; }
	if (tid == 0) { s.P[0] = 0; s.P2[0] = 0; }
#pragma unroll
	for (int k = 0; k < DT_K; k++) {
		b1 += (uint32_t)v[k];
		b2 += (uint64_t)((int64_t)v[k] * v[k]);
		s.P[tid * DT_K + k + 1] = b1;
		s.P2[tid * DT_K + k + 1] = b2;
	}
	__syncthreads();
}

template <int KIND>      // what the rows hold (SONDE_INPUT_*)
__global__ __launch_bounds__(DT_WG) void sd_detect_kernel(
	const void *__restrict__ in, size_t row_bytes, uint32_t n, SdDetState *__restrict__ states,
	int32_t *__restrict__ dD, size_t rowD, int32_t *__restrict__ dA, size_t rowA,
	const float2 *__restrict__ wi, const float2 *__restrict__ wc)
{
	__shared__ DtLds s;
	const int tid = threadIdx.x;
	const uint32_t ch = blockIdx.x;
	SdDetState *st = states + ch;
	const void *row = reinterpret_cast<const char *>(in) + (size_t)ch * row_bytes;
	const uint64_t n_abs = st->n;
	int32_t *D = dD + (size_t)ch * rowD;                          // [DT_H24 history | n / 2]
	int32_t *Ai = dA + (size_t)(2 * ch) * rowA, *Ac = Ai + rowA;  // [DT_H6 history | n / 8] each
	const uint32_t n2 = n >> 1, n8 = n >> 3;

	// A: GFSK branch, 24 kS/s
	const float2 y_prev = st->y_prev;
	for (uint32_t m = tid; m < n2; m += DT_WG) {
		float d;
		if (KIND == SONDE_INPUT_REAL) {
			const float *r = reinterpret_cast<const float *>(row);
			d = r[2 * m] + r[2 * m + 1];
		} else {
			const float2 a = dt_iq<KIND>(row, 2 * m), b = dt_iq<KIND>(row, 2 * m + 1);
			float2 yp = y_prev;
			if (m) { const float2 c = dt_iq<KIND>(row, 2 * m - 2), e = dt_iq<KIND>(row, 2 * m - 1); yp = make_float2(c.x + e.x, c.y + e.y); }
			d = sd_disc(a.x + b.x, a.y + b.y, yp.x, yp.y);
		}
		D[DT_H24 + m] = dt_qz(d);
	}

	// B: AFSK branch, 6 kS/s: one block of 8 input samples per thread and 2048-sample tile
	if (tid < 5) s.bi[tid] = st->bi[tid];
	if (tid < 2) s.bc[tid] = st->bc[tid];
	const float2 x_prev = st->x_prev;
	uint32_t phi = (uint32_t)(n_abs % SD_AF_PER), phc = (uint32_t)(n_abs % SD_C50_PER);
	__syncthreads();
	for (uint32_t tile = 0; tile < n / SD_TILE; tile++) {
		const uint32_t s0 = tile * SD_TILE + 8u * (uint32_t)tid;
		float d[8];
		if (KIND == SONDE_INPUT_REAL) {
#pragma unroll
			for (int i = 0; i < 8; i++) d[i] = reinterpret_cast<const float *>(row)[s0 + i];
		} else {
			float2 p = s0 ? dt_iq<KIND>(row, (int64_t)s0 - 1) : x_prev;
#pragma unroll
			for (int i = 0; i < 8; i++) {
				const float2 c = dt_iq<KIND>(row, s0 + i);
				d[i] = sd_disc(c.x, c.y, p.x, p.y);
				p = c;
			}
		}
		uint32_t ki = (phi + 8u * (uint32_t)tid) % SD_AF_PER, kc = (phc + 8u * (uint32_t)tid) % SD_C50_PER;
		float br = 0.0f, bim = 0.0f, cr = 0.0f, cim = 0.0f;
#pragma unroll
		for (int i = 0; i < 8; i++) {
			const float2 w1 = wi[ki], w2 = wc[kc];
			br = __builtin_fmaf(d[i], w1.x, br);
			bim = __builtin_fmaf(d[i], w1.y, bim);
			cr = __builtin_fmaf(d[i], w2.x, cr);
			cim = __builtin_fmaf(d[i], w2.y, cim);
			ki = (ki + 1 == SD_AF_PER) ? 0 : ki + 1;
			kc = (kc + 1 == SD_C50_PER) ? 0 : kc + 1;
		}
		s.bi[5 + tid] = make_float2(br, bim);
		s.bc[2 + tid] = make_float2(cr, cim);
		__syncthreads();
		{   // iMet: z[m] = (((b[m-4] + b[m-3]) + b[m-2]) + b[m-1]) + b[m]; q = atan2q(z[m] conj z[m-1])
			const float2 *b = s.bi + tid;
			const float z1r = (((b[1].x + b[2].x) + b[3].x) + b[4].x) + b[5].x, z1i = (((b[1].y + b[2].y) + b[3].y) + b[4].y) + b[5].y;
			const float z0r = (((b[0].x + b[1].x) + b[2].x) + b[3].x) + b[4].x, z0i = (((b[0].y + b[1].y) + b[2].y) + b[3].y) + b[4].y;
			Ai[DT_H6 + tile * DT_WG + tid] = dt_qz(sd_disc(z1r, z1i, z0r, z0i));
		}
		{   // SRS-C50: z[m] = b[m-1] + b[m]
			const float2 *b = s.bc + tid;
			Ac[DT_H6 + tile * DT_WG + tid] = dt_qz(sd_disc(b[1].x + b[2].x, b[1].y + b[2].y, b[0].x + b[1].x, b[0].y + b[1].y));
		}
		__syncthreads();
		if (tid < 5) s.bi[tid] = s.bi[DT_WG + tid];
		if (tid < 2) s.bc[tid] = s.bc[DT_WG + tid];
		phi = (phi + SD_TILE) % SD_AF_PER;
		phc = (phc + SD_TILE) % SD_C50_PER;
		__syncthreads();
	}

	// C: correlation.  Per-lane records start at the channel's: a lag must beat the best so far, so ties keep the earlier one.
	{
		const uint64_t m0 = n_abs >> 1;
		double b0 = st->best[SONDE_RS41], b1 = st->best[SONDE_DFM09], b2 = st->best[SONDE_IMS100], b3 = st->best[SONDE_M10], b6 = st->best[SONDE_MRZN1];
		uint32_t u0_ = ~0u, u1 = ~0u, u2 = ~0u, u3 = ~0u, u6 = ~0u, n0 = 0, n1 = 0, n2_ = 0, n3 = 0, n6 = 0;
		for (uint32_t u0 = 0; u0 < n2; u0 += DT_T) {
			dt_scan(s, D, DT_H24, n2, u0);
			dt_lags<SONDE_RS41>(s, u0, n2, m0, DT_H24, b0, u0_, n0);
			dt_lags<SONDE_DFM09>(s, u0, n2, m0, DT_H24, b1, u1, n1);
			dt_lags<SONDE_IMS100>(s, u0, n2, m0, DT_H24, b2, u2, n2_);
			dt_lags<SONDE_M10>(s, u0, n2, m0, DT_H24, b3, u3, n3);
			dt_lags<SONDE_MRZN1>(s, u0, n2, m0, DT_H24, b6, u6, n6);
			__syncthreads();
		}
		dt_commit<SONDE_RS41>(s, st, m0, b0, u0_, n0);
		dt_commit<SONDE_DFM09>(s, st, m0, b1, u1, n1);
		dt_commit<SONDE_IMS100>(s, st, m0, b2, u2, n2_);
		dt_commit<SONDE_M10>(s, st, m0, b3, u3, n3);
		dt_commit<SONDE_MRZN1>(s, st, m0, b6, u6, n6);
	}
	{
		const uint64_t m0 = n_abs >> 3;
		double b4 = st->best[SONDE_IMET4], b5 = st->best[SONDE_C50];
		uint32_t u4 = ~0u, u5 = ~0u, n4 = 0, n5 = 0;
		for (uint32_t u0 = 0; u0 < n8; u0 += DT_T) {
			dt_scan(s, Ai, DT_H6, n8, u0);
			dt_lags<SONDE_IMET4>(s, u0, n8, m0, DT_H6, b4, u4, n4);
			__syncthreads();
			dt_scan(s, Ac, DT_H6, n8, u0);
			dt_lags<SONDE_C50>(s, u0, n8, m0, DT_H6, b5, u5, n5);
			__syncthreads();
		}
		dt_commit<SONDE_IMET4>(s, st, m0, b4, u4, n4);
		dt_commit<SONDE_C50>(s, st, m0, b5, u5, n5);
	}

	// carry: the newest history of every stream moves to the head of its row (regions disjoint: n/2 >= 1024 > 320, n/8 >= 256 > 64)
	int32_t hD[2], hA[2];
	for (int r = 0; r < 2; r++) {
		const int e = tid + DT_WG * r;
		hD[r] = e < DT_H24 ? D[n2 + e] : 0;
		hA[r] = e < DT_H6 ? Ai[n8 + e] : (e < 2 * DT_H6 ? Ac[n8 + e - DT_H6] : 0);
	}
	__syncthreads();
	for (int r = 0; r < 2; r++) {
		const int e = tid + DT_WG * r;
		if (e < DT_H24) D[e] = hD[r];
		if (e < DT_H6) Ai[e] = hA[r];
		else if (e < 2 * DT_H6) Ac[e - DT_H6] = hA[r];
	}
	if (tid < 5) st->bi[tid] = s.bi[tid];
	if (tid < 2) st->bc[tid] = s.bc[tid];
	if (tid == 0) {
		st->n = n_abs + n;
		if (KIND != SONDE_INPUT_REAL) {
			const float2 a = dt_iq<KIND>(row, (int64_t)n - 2), b = dt_iq<KIND>(row, (int64_t)n - 1);
			st->y_prev = make_float2(a.x + b.x, a.y + b.y);
			st->x_prev = b;
		}
	}
}

// ---------------------------------------------------------------- host object
// theta_k: DESIGN 3.8's threshold table (the float64 reference over AWGN and over 30 dB signals of the other types)
static const float k_theta[SONDE_NTYPES] = { 0.52f, 0.79f, 0.85f, 0.82f, 0.83f, 0.91f, 0.86f };

struct __attribute__((visibility("hidden"))) SondeDetector {
	int device = 0, input_kind = 0;
	uint32_t n_channels = 0, max_samples = 0, last_n = 0;
	std::vector<uint8_t> mask;
	DevBuf<SdDetState> d_state;
	DevBuf<int32_t> d_D, d_A;
	size_t rowD = 0, rowA = 0;
	DevBuf<float2> d_wi, d_wc;
	hipStream_t last_stream = nullptr;
	bool submitted = false;
	SdChanLists restart_lists;              // sonde_detect_restart_channels
};

static DtTmpl dt_tmpl(int type)
{
	switch (type) {
	case SONDE_RS41: return dt_make<SONDE_RS41>();
	case SONDE_DFM09: return dt_make<SONDE_DFM09>();
	case SONDE_IMS100: return dt_make<SONDE_IMS100>();
	case SONDE_M10: return dt_make<SONDE_M10>();
	case SONDE_IMET4: return dt_make<SONDE_IMET4>();
	case SONDE_C50: return dt_make<SONDE_C50>();
	default: return dt_make<SONDE_MRZN1>();
	}
}

extern "C" int sonde_detect_templates(int type, int8_t *s, int cap)
{
	if (type < 0 || type >= SONDE_NTYPES || cap < 0) return sd_fail("sonde_detect_templates: bad argument");
	const DtTmpl t = dt_tmpl(type);
	for (int n = 0; s && n < t.L && n < cap; n++) s[n] = (int8_t)t.chip[n * t.baud / t.fs];
	return t.L;
}

extern "C" int sonde_detect_thresholds(float out[SONDE_NTYPES])
{
	if (!out) return sd_fail("sonde_detect_thresholds: null argument");
	for (int k = 0; k < SONDE_NTYPES; k++) out[k] = k_theta[k];
	return 0;
}

extern "C" void sonde_detect_destroy(SondeDetector *d)
{
	if (!d) return;
	(void)hipSetDevice(d->device);
	if (d->submitted) (void)hipStreamSynchronize(d->last_stream);
	delete d;
}

static int dt_clear(SondeDetector *d)
{
	hipError_t e;
	if ((e = hipMemset(d->d_state, 0, d->n_channels * sizeof(SdDetState))) != hipSuccess ||
	    (e = hipMemset(d->d_D, 0, d->n_channels * d->rowD * sizeof(int32_t))) != hipSuccess ||
	    (e = hipMemset(d->d_A, 0, 2 * (size_t)d->n_channels * d->rowA * sizeof(int32_t))) != hipSuccess ||
	    (e = hipDeviceSynchronize()) != hipSuccess)
		return sd_fail("sonde_detect: clearing the state", e);
	d->last_n = 0;
	return 0;
}

// Everything behind the argument checks: the mixer tables, the records and the carried streams, cleared as sonde_detect_reset clears
// them; on failure sonde_detect_create destroys what has been built so far.
static int dt_build(SondeDetector *d)
{
	float wi[2 * SD_AF_PER], wc[2 * SD_C50_PER];
	make_mixer(wi, 17, SD_AF_PER);
	make_mixer(wc, 19, SD_C50_PER);
	HIPCHK(d->d_wi.upload((const float2 *)wi, SD_AF_PER));
	HIPCHK(d->d_wc.upload((const float2 *)wc, SD_C50_PER));
	HIPCHK(d->d_state.alloc(d->n_channels));
	HIPCHK(d->d_D.alloc(d->n_channels * d->rowD));
	HIPCHK(d->d_A.alloc(2 * (size_t)d->n_channels * d->rowA));
	return dt_clear(d);
}

extern "C" int sonde_detect_create(uint32_t n_channels, uint32_t max_samples, int input_kind, const uint8_t *type_mask, int device, SondeDetector **out)
{
	if (!out) return sd_fail("sonde_detect_create: null argument");
	*out = nullptr;
	if (!n_channels || !max_samples || max_samples % SD_TILE) return sd_fail("sonde_detect_create: n_channels must be > 0 and max_samples a positive multiple of SONDE_TILE");
	if (!sd_input_known(input_kind)) return sd_fail("sonde_detect_create: bad input kind");
	if (sd_select_device(device, "sonde_detect_create")) return -1;
	SondeDetector *d = new SondeDetector;
	d->device = device; d->n_channels = n_channels; d->max_samples = max_samples; d->input_kind = input_kind;
	d->mask.assign(n_channels, 0x7F);
	if (type_mask) for (uint32_t c = 0; c < n_channels; c++) d->mask[c] = type_mask[c] & 0x7F;
	d->rowD = (DT_H24 + max_samples / 2 + 63) & ~(size_t)63;
	d->rowA = (DT_H6 + max_samples / 8 + 63) & ~(size_t)63;
	if (dt_build(d)) { sonde_detect_destroy(d); return -1; }       // (destroy leaves the error text alone)
	*out = d;
	return 0;
}

extern "C" int sonde_detect_submit(SondeDetector *d, const void *samples, size_t n_samples, size_t channel_stride, void *stream)
{
	if (!d || !samples) return sd_fail("sonde_detect_submit: null argument");
	if (n_samples == 0 || n_samples % SD_TILE || n_samples > d->max_samples) return sd_fail("sonde_detect_submit: n_samples must be a positive multiple of SONDE_TILE and <= max_samples");
	if (channel_stride < n_samples) return sd_fail("sonde_detect_submit: channel_stride < n_samples");
	const size_t eb = sd_sample_bytes(d->input_kind);
	if ((uintptr_t)samples % eb) return sd_fail("sonde_detect_submit: samples not aligned to the sample size");
	HIPCHK(hipSetDevice(d->device));
	hipStream_t s = (hipStream_t)stream;
	sd_input_dispatch(d->input_kind, [&](auto k) {
		hipLaunchKernelGGL(sd_detect_kernel<decltype(k)::value>, dim3(d->n_channels), dim3(DT_WG), 0, s, samples, channel_stride * eb, (uint32_t)n_samples,
			d->d_state, d->d_D, d->rowD, d->d_A, d->rowA, d->d_wi, d->d_wc);
	});
	HIPCHK_IN("sonde_detect_submit", hipGetLastError());
	d->last_stream = s;
	d->last_n = (uint32_t)n_samples;
	d->submitted = true;
	return 0;
}

static int dt_sync(SondeDetector *d)
{
	hipError_t e = hipSetDevice(d->device);
	if (e == hipSuccess && d->submitted) e = hipStreamSynchronize(d->last_stream);
	if (e != hipSuccess) return sd_fail("sonde_detect: synchronise", e);
	return 0;
}

extern "C" int sonde_detect_results(SondeDetector *d, SondeDetection *out, size_t cap)
{
	if (!d || !out) return sd_fail("sonde_detect_results: null argument");
	if (dt_sync(d)) return -1;
	const uint32_t nc = (uint32_t)(cap < d->n_channels ? cap : d->n_channels);
	std::vector<SdDetState> h(nc);
	hipError_t e = hipMemcpy(h.data(), d->d_state, nc * sizeof(SdDetState), hipMemcpyDeviceToHost);
	if (e != hipSuccess) return sd_fail("sonde_detect_results: copy", e);
	for (uint32_t c = 0; c < nc; c++) {
		SondeDetection &r = out[c];
		r.inverted = h[c].neg;
		// decision (SPEC 3.8): argmax best_k / theta_k over the types of the channel's mask with best_k >= theta_k
		int32_t type = -1;
		double vbest = 0.0;
		for (int k = 0; k < SONDE_NTYPES; k++) {
			r.best[k] = h[c].best[k];
			r.pos[k] = h[c].pos[k];
			const double th = (double)k_theta[k];
			if (!((d->mask[c] >> k) & 1) || r.best[k] < th) continue;
			const double v = r.best[k] / th;
			if (v > vbest) { vbest = v; type = k; }
		}
		r.type = type;
	}
	return (int)nc;
}

extern "C" int sonde_detect_reset(SondeDetector *d)
{
	if (!d) return sd_fail("sonde_detect_reset: null argument");
	if (dt_sync(d)) return -1;
	return dt_clear(d);
}

// the listed channels back to their state after create (SPEC 3.12): records, front-end state and the carried streams, zeros all
__global__ __launch_bounds__(DT_WG) void sd_detect_restart_kernel(const uint32_t *__restrict__ list, SdDetState *__restrict__ state,
	int32_t *__restrict__ D, size_t rowD, int32_t *__restrict__ A, size_t rowA)
{
	const uint32_t c = list[blockIdx.x], tid = threadIdx.x;
	if (tid < sizeof(SdDetState) / 4) ((uint32_t *)(state + c))[tid] = 0u;
	for (size_t i = tid; i < rowD; i += DT_WG) D[c * rowD + i] = 0;
	for (size_t i = tid; i < 2 * rowA; i += DT_WG) A[2 * c * rowA + i] = 0;
}

extern "C" int sonde_detect_restart_channels(SondeDetector *d, const uint32_t *channels, size_t n)
{
	if (!d || (!channels && n)) return sd_fail("sonde_detect_restart_channels: null argument");
	for (size_t i = 0; i < n; i++)
		if (channels[i] >= d->n_channels) return sd_fail("sonde_detect_restart_channels: no such channel");
	if (n == 0 || !d->submitted) return 0;      // nothing has run: the state is what create set
	HIPCHK(hipSetDevice(d->device));
	SdChanLists::Buf *lb = d->restart_lists.put(channels, n);
	if (!lb) return sd_fail("sonde_detect_restart_channels: no pinned memory for the channel list");
	// on the stream of the last submit: behind its kernel; a submit on another stream is the caller's to order, as between submits
	hipLaunchKernelGGL(sd_detect_restart_kernel, dim3((unsigned)n), dim3(DT_WG), 0, d->last_stream, lb->list.dev(), d->d_state, d->d_D, d->rowD, d->d_A, d->rowA);
	HIPCHK_IN("sonde_detect_restart_channels", hipGetLastError());
	HIPCHK_IN("sonde_detect_restart_channels", d->restart_lists.done(lb, d->last_stream));
	return 0;
}

// test introspection (DESIGN "Stream age"): the listed channels become "the same stream, begun samples[i] input samples earlier".
// SdDetState's absolute positions are n and the pos[k] of the types that have a match (best[k] > 0; a type without one keeps pos 0);
// the front-end state, the records' values and signs and the carried streams are relative.  entry i of the list: 4 words
// { channel, 0, samples lo, hi }.
__global__ __launch_bounds__(64) void sd_detect_shift_age_kernel(const uint32_t *__restrict__ list, uint32_t n, SdDetState *__restrict__ state)
{
	const uint32_t i = 64 * blockIdx.x + threadIdx.x;
	if (i >= n) return;
	SdDetState *st = state + list[4 * (size_t)i];
	const uint64_t samples = (uint64_t)list[4 * (size_t)i + 2] | (uint64_t)list[4 * (size_t)i + 3] << 32;
	st->n += samples;
	for (int k = 0; k < SONDE_NTYPES; k++)
		if (st->best[k] > 0.0) st->pos[k] += samples;
}

extern "C" int sonde_detect_test_shift_age(SondeDetector *d, const uint32_t *channels, size_t n, const uint64_t *samples)
{
	if (!d || !channels || !samples || !n) return sd_fail("sonde_detect_test_shift_age: null argument");
	if (!d->submitted) return sd_fail("sonde_detect_test_shift_age: nothing has run yet (shift after the first submit)");
	std::vector<uint8_t> seen(d->n_channels, 0);
	std::vector<uint32_t> words(4 * n, 0u);
	for (size_t i = 0; i < n; i++) {
		if (channels[i] >= d->n_channels) return sd_fail("sonde_detect_test_shift_age: no such channel");
		if (seen[channels[i]]) return sd_fail("sonde_detect_test_shift_age: a channel listed twice");
		if (samples[i] % 30720u || samples[i] >> 62)
			return sd_fail("sonde_detect_test_shift_age: samples must be a multiple of 30720 (tile phase and both tone-mixer phases stay) below 2^62");
		seen[channels[i]] = 1;
		words[4 * i] = channels[i]; words[4 * i + 2] = (uint32_t)samples[i]; words[4 * i + 3] = (uint32_t)(samples[i] >> 32);
	}
	HIPCHK(hipSetDevice(d->device));
	SdChanLists::Buf *lb = d->restart_lists.put(words.data(), words.size());
	if (!lb) return sd_fail("sonde_detect_test_shift_age: no pinned memory for the list");
	// ordered as sonde_detect_restart_channels orders its kernel: on the stream of the last submit, behind its kernel
	hipLaunchKernelGGL(sd_detect_shift_age_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, d->last_stream, lb->list.dev(), (uint32_t)n, d->d_state);
	HIPCHK_IN("sonde_detect_test_shift_age", hipGetLastError());
	HIPCHK_IN("sonde_detect_test_shift_age", d->restart_lists.done(lb, d->last_stream));
	return 0;
}

extern "C" int sonde_detect_read(SondeDetector *d, uint32_t channel, int32_t *D, int32_t *a_imet, int32_t *a_c50)
{
	if (!d || !D || !a_imet || !a_c50) return sd_fail("sonde_detect_read: null argument");
	if (channel >= d->n_channels) return sd_fail("sonde_detect_read: no such channel");
	if (dt_sync(d)) return -1;
	const size_t n2 = d->last_n / 2, n8 = d->last_n / 8;
	hipError_t e;
	if ((e = hipMemcpy(D, d->d_D + channel * d->rowD + DT_H24, n2 * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = hipMemcpy(a_imet, d->d_A + 2 * channel * d->rowA + DT_H6, n8 * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = hipMemcpy(a_c50, d->d_A + (2 * channel + 1) * d->rowA + DT_H6, n8 * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess)
		return sd_fail("sonde_detect_read: copy", e);
	return (int)d->last_n;
}
