// combine.hip -- coherent antenna combiner (DESIGN SPEC 3.14): the K antennas' complex64 rows of one sonde at rate R (the rows K tuners
// with the same VFO list write; row a * S + i = sonde i on antenna a) are added with complex weights that align their phases and favour
// the stronger ones, y[m] = sum_a conj(w_a) x_a[m], |w| = 1, and one row per sonde goes to the decoder, whatever its type.  The
// antennas share one sample clock and start together.
//
// Three launches per submit on the caller's stream, and no workgroup ever waits for another:
//   sd_combine_stats_kernel    one 256-lane workgroup per (sonde, block of L samples): M = sum x x^H, K powers and K (K - 1) / 2 complex
//                              cross terms, in the carrier meter's arithmetic (sd_blocksum.h: float32 products with one fmaf, each
//                              aligned 256-sample block in the meter's lane and butterfly order, block sums into doubles in ascending order)
//   sd_combine_weights_kernel  one lane per sonde walks its blocks in order: sd_combine_weights (sd_combine.h) from M and the previous
//                              block's weights; the sonde's last weights are all that is carried to the next submit
//   sd_combine_apply_kernel    one workgroup per (sonde, block): the float32 fmaf chain, 16-byte loads and nontemporal 16-byte stores
//                              where the rows are 16-byte aligned, 8-byte ones where they are not (rows an odd stride apart)
// A block's numbers depend on its samples and the weights before it alone, never on how the stream was cut into submits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "launch.h"
#include "sd_host.h"
#include "sd_devmem.h"
#include "sd_combine.h"
#include "sd_blocksum.h"
#include "../../include/sonde_abi.h"

#define CB_WG     SD_BS_WG              // the apply kernel's workgroup too
#define CB_NQ     16                    // doubles of M
#define CB_VMAX   512                   // sondes per weights launch: their restart bits travel with the launch, by value
#define CB_MAXLB  16384                 // largest block, in summation blocks

typedef float cb_f32x4 __attribute__((ext_vector_type(4)));
typedef float cb_f32x2 __attribute__((ext_vector_type(2)));
struct SdCombineFresh { uint32_t bits[CB_VMAX / 32]; };

// grid (blocks of the submit, sondes).  stat[(sonde * max_blocks + b) * 16 + q]
template <int K> __global__ __launch_bounds__(CB_WG) void sd_combine_stats_kernel(const float2 *__restrict__ rows, size_t stride, uint32_t S, uint32_t LB,
	uint32_t max_blocks, double *__restrict__ stat)
{
	constexpr int NP = K * (K - 1) / 2, NQ = K + 2 * NP;
	__shared__ float s_bs[NQ][SD_BS_CHUNK];
	const uint32_t tid = threadIdx.x;
	const uint32_t b = blockIdx.x, sonde = blockIdx.y;
	const float2 *x[K];
#pragma unroll
	for (int a = 0; a < K; a++) x[a] = rows + ((size_t)a * S + sonde) * stride + (size_t)b * LB * SD_BS_BLK;
	// quantity tid < NQ -> its place among the 16 doubles: powers first, then the pairs (a, c), a < c, in the K = 4 numbering
	int slot = 0;
	if (tid < (uint32_t)K) slot = (int)tid;
	else if (tid < (uint32_t)NQ) {
		int p = ((int)tid - K) >> 1, a = 0, c = 1;
		for (int i = 0; i < p; i++) { if (++c == K) { a++; c = a + 1; } }
		const int p4 = a == 0 ? c - 1 : a == 1 ? c + 1 : 5;
		slot = 4 + 2 * p4 + (((int)tid - K) & 1);
	}
	// the K powers, then re and im of x_a conj(x_c) for the pairs a < c, of sample m of the block
	struct Across { float2 x[K]; };
	const double acc = sd_blocksum<NQ>(0u, LB, 0.0, s_bs,
		[&](int64_t m) {
			Across v;
#pragma unroll
			for (int a = 0; a < K; a++) v.x[a] = x[a][m];
			return v;
		},
		[](const Across &v, float (&p)[NQ]) {
			int k = 0;
#pragma unroll
			for (int a = 0; a < K; a++, k++) p[k] = __builtin_fmaf(v.x[a].x, v.x[a].x, v.x[a].y * v.x[a].y);
#pragma unroll
			for (int a = 0; a < K; a++)
#pragma unroll
				for (int c = a + 1; c < K; c++, k += 2) {
					p[k] = __builtin_fmaf(v.x[a].x, v.x[c].x, v.x[a].y * v.x[c].y);
					p[k + 1] = __builtin_fmaf(v.x[a].y, v.x[c].x, -(v.x[a].x * v.x[c].y));
				}
		});
	if (tid < (uint32_t)NQ) stat[((size_t)sonde * max_blocks + b) * CB_NQ + slot] = acc;
}

// one lane per sonde of [vbase, vbase + nv): state[sonde * 8] = the weights carried; w / wf[(sonde * max_blocks + b) * 8]
template <int K> __global__ __launch_bounds__(64) void sd_combine_weights_kernel(uint32_t vbase, uint32_t nv, uint32_t nblk, uint32_t max_blocks,
	SdCombineFresh fr, const double *__restrict__ stat, double *__restrict__ state, double *__restrict__ w, float *__restrict__ wf)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nv) return;
	const uint32_t sonde = vbase + i;
	bool fresh = (fr.bits[i >> 5] >> (i & 31u)) & 1u;
	double cur[2 * K], m[CB_NQ];
#pragma unroll
	for (int k = 0; k < 2 * K; k++) cur[k] = state[(size_t)sonde * 8 + k];
	for (uint32_t b = 0; b < nblk; b++) {
		const size_t at = (size_t)sonde * max_blocks + b;
#pragma unroll
		for (int k = 0; k < CB_NQ; k++) m[k] = stat[at * CB_NQ + k];
		sd_combine_weights(K, m, fresh ? nullptr : cur, cur);
		fresh = false;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			w[at * 8 + k] = k < 2 * K ? cur[k] : 0.0;
			wf[at * 8 + k] = k < 2 * K ? (float)cur[k] : 0.0f;
		}
	}
#pragma unroll
	for (int k = 0; k < 2 * K; k++) state[(size_t)sonde * 8 + k] = cur[k];
}

// the chain of SPEC 3.14 for one sample: per component, a = 0 .. K - 1 in this order
template <int K> static __device__ __forceinline__ float2 cb_chain(const float2 (&x)[K], const float (&wr)[K], const float (&wi)[K])
{
	float yr = wr[0] * x[0].x, yi = wr[0] * x[0].y;
	yr = __builtin_fmaf(wi[0], x[0].y, yr);
	yi = __builtin_fmaf(-wi[0], x[0].x, yi);
#pragma unroll
	for (int a = 1; a < K; a++) {
		yr = __builtin_fmaf(wr[a], x[a].x, yr);
		yr = __builtin_fmaf(wi[a], x[a].y, yr);
		yi = __builtin_fmaf(wr[a], x[a].y, yi);
		yi = __builtin_fmaf(-wi[a], x[a].x, yi);
	}
	return make_float2(yr, yi);
}

// grid (blocks of the submit, sondes)
template <int K> __global__ __launch_bounds__(CB_WG) void sd_combine_apply_kernel(const float2 *__restrict__ rows, size_t stride, uint32_t S, uint32_t L,
	uint32_t max_blocks, const float *__restrict__ wf, float2 *__restrict__ out, size_t out_stride)
{
	const uint32_t tid = threadIdx.x, b = blockIdx.x, sonde = blockIdx.y;
	const float *wv = wf + ((size_t)sonde * max_blocks + b) * 8;
	float wr[K], wi[K];
	const float2 *x[K];
	float2 *y = out + (size_t)sonde * out_stride + (size_t)b * L;
	uintptr_t bits = (uintptr_t)y;
#pragma unroll
	for (int a = 0; a < K; a++) {
		wr[a] = wv[2 * a]; wi[a] = wv[2 * a + 1];
		x[a] = rows + ((size_t)a * S + sonde) * stride + (size_t)b * L;
		bits |= (uintptr_t)x[a];
	}
	if ((bits & 15u) == 0) {                                 // every row 16-byte aligned: two samples per access
		for (uint32_t j = tid; j < L / 2; j += CB_WG) {
			float2 u[K], v[K];
#pragma unroll
			for (int a = 0; a < K; a++) {
				const cb_f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const cb_f32x4 *>(x[a]) + j);
				u[a] = make_float2(q.x, q.y); v[a] = make_float2(q.z, q.w);
			}
			const float2 y0 = cb_chain<K>(u, wr, wi), y1 = cb_chain<K>(v, wr, wi);
			cb_f32x4 o; o.x = y0.x; o.y = y0.y; o.z = y1.x; o.w = y1.y;
			__builtin_nontemporal_store(o, reinterpret_cast<cb_f32x4 *>(y) + j);
		}
	} else {
		for (uint32_t j = tid; j < L; j += CB_WG) {
			float2 u[K];
#pragma unroll
			for (int a = 0; a < K; a++) {
				const cb_f32x2 q = __builtin_nontemporal_load(reinterpret_cast<const cb_f32x2 *>(x[a]) + j);
				u[a] = make_float2(q.x, q.y);
			}
			const float2 y0 = cb_chain<K>(u, wr, wi);
			cb_f32x2 o; o.x = y0.x; o.y = y0.y;
			__builtin_nontemporal_store(o, reinterpret_cast<cb_f32x2 *>(y) + j);
		}
	}
}

// ---------------------------------------------------------------- host
struct SondeCombiner {
	int device = 0;
	uint32_t S = 0, K = 0, rate = 0, max_samples = 0, L = 0, max_blocks = 0, last_blocks = 0;
	hipStream_t last = nullptr;
	std::vector<uint8_t> fresh;         // the sonde's next block has no previous weights
	std::vector<uint64_t> block;        // index of the sonde's next block (from the last restart)
	std::vector<uint64_t> first;        // index of the first block of the last submit, per sonde
	DevBuf<double> d_stat, d_w, d_state;
	DevBuf<float> d_wf;
};

extern "C" void sonde_combine_destroy(SondeCombiner *c)
{
	if (!c) return;
	(void)hipSetDevice(c->device);
	delete c;
}

// Everything behind the argument checks; on failure sonde_combine_create destroys what has been built so far.
static int cb_build(SondeCombiner *c)
{
	const size_t nb = (size_t)c->S * c->max_blocks;
	HIPCHK(c->d_stat.zeros(nb * CB_NQ));
	HIPCHK(c->d_w.zeros(nb * 8));
	HIPCHK(c->d_wf.zeros(nb * 8));
	HIPCHK(c->d_state.zeros((size_t)c->S * 8));
	return 0;
}

extern "C" int sonde_combine_defaults(uint32_t rate, uint32_t *block)
{
	if (rate < 5000u || rate > 100000u) return sd_fail("sonde_combine_defaults: rate must be 5000 .. 100 000 Hz");
	if (block) *block = SONDE_COMBINE_BLOCK;
	return 0;
}

extern "C" int sonde_combine_create(uint32_t n_sondes, uint32_t antennas, uint32_t rate, uint32_t max_samples, uint32_t block, int input_kind,
	int device, SondeCombiner **out)
{
	if (!out || !n_sondes || n_sondes > 65535u) return sd_fail("sonde_combine_create: bad argument (n_sondes must be 1 .. 65 535)");
	if (antennas < 2 || antennas > SONDE_COMBINE_MAX_ANTENNAS) return sd_fail("sonde_combine_create: antennas must be 2 .. 4");
	if (input_kind != SONDE_INPUT_IQ)
		return sd_fail("sonde_combine_create: input_kind must be SONDE_INPUT_IQ (the combiner takes the tuner's complex64 rows; REAL rows carry no phase to align)");
	uint32_t L0;
	if (sonde_combine_defaults(rate, &L0)) return sd_fail("sonde_combine_create: rate must be 5000 .. 100 000 Hz");
	const uint32_t L = block ? block : L0;
	if (L % SD_BS_BLK || L / SD_BS_BLK > CB_MAXLB) return sd_fail("sonde_combine_create: block must be a multiple of 256, at most 4 194 304 (0 = 1024)");
	if (!max_samples || max_samples % L || max_samples >= (1u << 30)) return sd_fail("sonde_combine_create: max_samples must be a positive multiple of the block length below 2^30");
	if (sd_select_device(device, "sonde_combine_create")) return -1;
	SondeCombiner *c = new SondeCombiner;
	c->device = device; c->S = n_sondes; c->K = antennas; c->rate = rate; c->max_samples = max_samples; c->L = L; c->max_blocks = max_samples / L;
	c->fresh.assign(n_sondes, 1); c->block.assign(n_sondes, 0); c->first.assign(n_sondes, 0);
	if (cb_build(c)) { sonde_combine_destroy(c); return -1; }     // (destroy leaves the error text alone)
	*out = c;
	return 0;
}

extern "C" int sonde_combine_block(const SondeCombiner *c) { return c ? (int)c->L : sd_fail("sonde_combine_block: null argument"); }

template <int K> static void cb_launch(SondeCombiner *c, const float2 *rows, size_t stride, uint32_t nblk, float2 *out, size_t out_stride, hipStream_t s)
{
	const dim3 grid(nblk, c->S);
	hipLaunchKernelGGL(sd_combine_stats_kernel<K>, grid, dim3(CB_WG), 0, s, rows, stride, c->S, c->L / SD_BS_BLK, c->max_blocks, (double *)c->d_stat);
	for (uint32_t vb = 0; vb < c->S; vb += CB_VMAX) {
		const uint32_t nv = c->S - vb < CB_VMAX ? c->S - vb : CB_VMAX;
		SdCombineFresh fr = {};
		for (uint32_t i = 0; i < nv; i++)
			if (c->fresh[vb + i]) fr.bits[i >> 5] |= 1u << (i & 31u);
		hipLaunchKernelGGL(sd_combine_weights_kernel<K>, dim3((nv + 63) / 64), dim3(64), 0, s, vb, nv, nblk, c->max_blocks, fr, (const double *)c->d_stat,
			(double *)c->d_state, (double *)c->d_w, (float *)c->d_wf);
	}
	hipLaunchKernelGGL(sd_combine_apply_kernel<K>, grid, dim3(CB_WG), 0, s, rows, stride, c->S, c->L, c->max_blocks, (const float *)c->d_wf, out, out_stride);
}

extern "C" int sonde_combine_process(SondeCombiner *c, const void *rows_dev, size_t n, size_t row_stride, void *out_dev, size_t out_stride, void *stream)
{
	if (!c || !rows_dev || !out_dev) return sd_fail("sonde_combine_process: null argument");
	if (!n || n % c->L || n > c->max_samples)
		return sd_fail("sonde_combine_process: n must be a positive multiple of the block length and <= max_samples");
	if (row_stride < n || out_stride < n) return sd_fail("sonde_combine_process: row_stride / out_stride shorter than the row");
	if (((uintptr_t)rows_dev | (uintptr_t)out_dev) & 7u) return sd_fail("sonde_combine_process: rows and out must be 8-byte aligned");
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = (hipStream_t)stream;
	const uint32_t nblk = (uint32_t)(n / c->L);
	const float2 *rows = (const float2 *)rows_dev;
	float2 *out = (float2 *)out_dev;
	if (c->K == 2) cb_launch<2>(c, rows, row_stride, nblk, out, out_stride, s);
	else if (c->K == 3) cb_launch<3>(c, rows, row_stride, nblk, out, out_stride, s);
	else cb_launch<4>(c, rows, row_stride, nblk, out, out_stride, s);
	HIPCHK_IN("sonde_combine_process", hipGetLastError());
	for (uint32_t i = 0; i < c->S; i++) {
		c->first[i] = c->block[i];
		c->block[i] += nblk;
		c->fresh[i] = 0;
	}
	c->last_blocks = nblk;
	c->last = s;
	return 0;
}

extern "C" int sonde_combine_restart(SondeCombiner *c, uint32_t sonde)
{
	if (!c) return sd_fail("sonde_combine_restart: null argument");
	if (sonde >= c->S) return sd_fail("sonde_combine_restart: no such sonde");
	c->fresh[sonde] = 1; c->block[sonde] = 0;
	return 0;
}

extern "C" int sonde_combine_readout(SondeCombiner *c, SondeCombineBlock *out, size_t cap)
{
	if (!c || (!out && cap)) return sd_fail("sonde_combine_readout: null argument");
	const size_t count = (size_t)c->S * c->last_blocks;
	if (cap < count) return sd_fail("sonde_combine_readout: the buffer is shorter than n_sondes * (n / block) of the last submit");
	if (!count) return 0;
	HIPCHK(hipSetDevice(c->device));
	hipError_t e = hipStreamSynchronize(c->last);
	if (e != hipSuccess) return sd_fail("sonde_combine_readout: hipStreamSynchronize", e);
	const size_t nb = (size_t)c->S * c->max_blocks;
	std::vector<double> st(nb * CB_NQ), w(nb * 8);
	std::vector<float> wf(nb * 8);
	if ((e = hipMemcpy(st.data(), c->d_stat, st.size() * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = hipMemcpy(w.data(), c->d_w, w.size() * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess ||
	    (e = hipMemcpy(wf.data(), c->d_wf, wf.size() * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess)
		return sd_fail("sonde_combine_readout: hipMemcpy", e);
	size_t k = 0;
	for (uint32_t i = 0; i < c->S; i++)
		for (uint32_t b = 0; b < c->last_blocks; b++, k++) {
			const size_t at = (size_t)i * c->max_blocks + b;
			out[k].sonde = i; out[k].reserved = 0; out[k].block = c->first[i] + b;
			for (int q = 0; q < CB_NQ; q++) out[k].m[q] = st[at * CB_NQ + q];
			for (int q = 0; q < 8; q++) { out[k].w[q] = w[at * 8 + q]; out[k].wf[q] = wf[at * 8 + q]; }
		}
	return (int)count;
}

// ---------------------------------------------------------------- pure host
extern "C" int sonde_combine_weights(uint32_t antennas, const double *m, const double *w_prev, double *w)
{
	if (!m || !w) return sd_fail("sonde_combine_weights: null argument");
	if (antennas < 2 || antennas > SONDE_COMBINE_MAX_ANTENNAS) return sd_fail("sonde_combine_weights: antennas must be 2 .. 4");
	sd_combine_weights((int)antennas, m, w_prev, w);
	return 0;
}

extern "C" double sonde_combine_share(const double *w, uint32_t a) { return w ? w[2 * a] * w[2 * a] + w[2 * a + 1] * w[2 * a + 1] : 0.0; }
