// sd_combine.h -- the weights of the coherent combiner (DESIGN SPEC 3.14), one routine for the kernel and for the pure-host
// sonde_combine_weights: double, only + - * / sqrt, contraction off (the Makefile's -ffp-contract=off), so both give the same numbers.
#pragma once
#include <hip/hip_runtime.h>

#define SD_CB_KMAX 4

// element (a, c) of the Hermitian M = sum x x^H from the 16 doubles of SondeCombineBlock.m
static __host__ __device__ inline void sd_combine_m(const double *m, int a, int c, double &re, double &im)
{
	if (a == c) { re = m[a]; im = 0.0; return; }
	const int lo = a < c ? a : c, hi = a < c ? c : a;
	const int p = lo == 0 ? hi - 1 : lo == 1 ? hi + 1 : 5;      // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
	re = m[4 + 2 * p];
	im = a < c ? m[5 + 2 * p] : -m[5 + 2 * p];
}

// w_prev: 2 K doubles, or null after a restart; w: 2 K doubles (may be w_prev)
static __host__ __device__ inline void sd_combine_weights(int K, const double *m, const double *w_prev, double *w)
{
	double vr[SD_CB_KMAX], vi[SD_CB_KMAX], pr[SD_CB_KMAX], pi[SD_CB_KMAX];
	if (w_prev) {
		for (int a = 0; a < K; a++) { pr[a] = vr[a] = w_prev[2 * a]; pi[a] = vi[a] = w_prev[2 * a + 1]; }
	} else {
		int best = 0;
		for (int a = 1; a < K; a++) if (m[a] > m[best]) best = a;
		for (int a = 0; a < K; a++) { pr[a] = pi[a] = 0.0; vr[a] = a == best ? 1.0 : 0.0; vi[a] = 0.0; }
	}
	for (int it = 0; it < 4; it++) {
		double ur[SD_CB_KMAX], ui[SD_CB_KMAX], s = 0.0;
		for (int a = 0; a < K; a++) {
			double sr = 0.0, si = 0.0;
			for (int c = 0; c < K; c++) {
				double mr, mi;
				sd_combine_m(m, a, c, mr, mi);
				sr = sr + (mr * vr[c] - mi * vi[c]);
				si = si + (mr * vi[c] + mi * vr[c]);
			}
			ur[a] = sr; ui[a] = si;
			s = s + (sr * sr + si * si);
		}
		const double nrm = sqrt(s);
		if (!(nrm > 0.0)) break;                             // M v = 0: the start vector stays
		for (int a = 0; a < K; a++) { vr[a] = ur[a] / nrm; vi[a] = ui[a] / nrm; }
	}
	// the phase rule: rho = w_prev^H v
	double rr = 0.0, ri = 0.0;
	for (int a = 0; a < K; a++) {
		rr = rr + (pr[a] * vr[a] + pi[a] * vi[a]);
		ri = ri + (pr[a] * vi[a] - pi[a] * vr[a]);
	}
	const double ab = sqrt(rr * rr + ri * ri);
	if (ab > 0.0) {
		const double cr = rr / ab, ci = -(ri / ab);          // conj(rho) / |rho|
		for (int a = 0; a < K; a++) {
			const double xr = vr[a] * cr - vi[a] * ci, xi = vr[a] * ci + vi[a] * cr;
			vr[a] = xr; vi[a] = xi;
		}
	}
	for (int a = 0; a < K; a++) { w[2 * a] = vr[a]; w[2 * a + 1] = vi[a]; }
}
