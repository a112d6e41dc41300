// scan.hip -- band scanner (DESIGN SPEC 3.10): the averaged power spectrum of one wideband complex stream (Welch: segments of N
// samples, 50 % overlap, periodic Hann window) on the GPU, and the candidate search over it (offset, occupied bandwidth, C/N0) on the
// host, in double, from the float32 spectrum.  It stands where a person looks at the SDR++ waterfall and drags a VFO onto a carrier
// (/root/reference/src/main.cpp:55-68): its candidates are the offsets SondeTuner / SondeDetector / WidebandReceiver take.
//
// One workgroup per segment, the whole segment in LDS (8.5 N bytes with its padding: 136 KB at N = 16384, one workgroup per CU).  Load (raw block or
// the carried tail) -> convert (sd_input.h) -> window -> in-place decimation-in-frequency FFT, radix 4, two stages per trip through LDS (one radix-2
// stage first where log2 N is odd), twiddles from a float table made in double on the host -> |.|^2 -> the power row, unscrambled through LDS so that
// the row is written in natural bin order, coalesced.  No segment, window product or transform ever reaches HBM.  A second kernel,
// one lane per bin, adds the launch's rows to the double accumulator in ascending segment order: the accumulator depends on the
// samples and the absolute segment indices alone, never on how the stream was cut into submits.  The unfinished tail (at most N - 1
// raw samples, as float2) is double-buffered and refreshed by a third kernel behind the first, as the tuner's history is.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "launch.h"
#include "sd_host.h"
#include "sd_devmem.h"
#include "sd_design.h"
#include "sd_input.h"
#include "../../include/sonde_abi.h"

#define SC_MIN_LOG2 10
#define SC_MAX_LOG2 14
#define SC_ROW_BYTES (32u << 20)        // power rows per launch pair: 32 MB of them, at most 2048 (512 at N = 16384); a longer submit takes several
#define SC_ROWS_MAX 2048
#define SC_PAD(i)   ((i) + ((i) >> 4))  // the segment in LDS: one float2 of padding per 16, so that the short strides of the late stages spread over the banks
#define SC_ACC_BINS 64                  // the adding kernel: 64 bins per workgroup of 16 waves, tiles of 256 rows through LDS
#define SC_ACC_WAVES 16
#define SC_ACC_PER  16
#define SC_ACC_TILE (SC_ACC_WAVES * SC_ACC_PER)

static __device__ __forceinline__ float2 sc_cmul(float2 a, float2 w)
{
	return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * w.y)), __builtin_fmaf(a.x, w.y, a.y * w.x));
}

// the radix-4 decimation-in-frequency butterfly without its twiddles: y_p = sum_m a_m (-i)^(p m), in place
static __device__ __forceinline__ void sc_bfly4(float2 &a0, float2 &a1, float2 &a2, float2 &a3)
{
	const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
	const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
	a0 = make_float2(t0.x + t2.x, t0.y + t2.y); a2 = make_float2(t0.x - t2.x, t0.y - t2.y);
	a1 = make_float2(t1.x + t3.y, t1.y - t3.x); a3 = make_float2(t1.x - t3.y, t1.y + t3.x);
}

// position in the transformed array -> frequency bin: the digits of the position, most significant first, are the digits of the bin,
// least significant first (radix 2 first where LOG2N is odd, then radix 4)
template <int LOG2N> static __device__ __forceinline__ uint32_t sc_bin_of(uint32_t pos)
{
	uint32_t k = 0;
	int sh = LOG2N, m = 0;
	if (LOG2N & 1) { sh -= 1; k = pos >> sh; pos &= (1u << sh) - 1u; m = 1; }
#pragma unroll
	for (; sh >= 2; m += 2) { sh -= 2; k |= (pos >> sh) << m; pos &= (1u << sh) - 1u; }
	return k;
}

// The twiddles, one table per stage so that the lanes of a wave read neighbours: the radix-2 stage's W_N^j (j < N / 2) where log2 N is
// odd, then per radix-4 stage of block length L = 2^lg > 4 the three rows W_L^(p j), p = 1 .. 3, j < L / 4.  Offset of stage lg:
static constexpr __host__ __device__ int sc_tw_off(int log2n, int lg)
{
	int o = (log2n & 1) ? (1 << (log2n - 1)) : 0;
	for (int l = log2n - (log2n & 1); l > lg; l -= 2) o += 3 << (l - 2);
	return o;
}

template <int LOG2N> struct ScCfg {
	static constexpr int N = 1 << LOG2N;
	static constexpr int TH = N / 16 < 128 ? 128 : N / 16;        // one 16-point pass per thread: 1024 threads at N = 16384
};

// segment blockIdx.x of the launch: absolute samples [first + blockIdx.x N/2, + N), first = seg0 N/2; the sample with absolute index
// a lies in the tail at a - tail_base (a < n_base) or in the block at a - n_base.  rel = first - n_base, tail_len = n_base - tail_base.
template <int K, int LOG2N>
__global__ __launch_bounds__(ScCfg<LOG2N>::TH) void sd_scan_kernel(const void *__restrict__ xin, const float2 *__restrict__ tail, int64_t rel,
	int64_t tail_len, const float *__restrict__ win, const float2 *__restrict__ tw, float *__restrict__ rows)
{
	constexpr int N = ScCfg<LOG2N>::N, TH = ScCfg<LOG2N>::TH, PER = N / TH;
	__shared__ float2 s[SC_PAD(N)];
	const sd_iq_t<K> *x = (const sd_iq_t<K> *)xin;
	const int tid = threadIdx.x;
	const int64_t off = rel + (int64_t)blockIdx.x * (N / 2);
	{
		float2 v[PER];              // every load of the thread in flight before the first use
#pragma unroll
		for (int r = 0; r < PER; r++) {
			const int64_t a = off + tid + r * TH;
			v[r] = a < 0 ? tail[tail_len + a] : sd_iq_f2<K>(x[a]);
		}
#pragma unroll
		for (int r = 0; r < PER; r++) {
			const int i = tid + r * TH;
			const float w = win[i];
			s[SC_PAD(i)] = make_float2(w * v[r].x, w * v[r].y);
		}
	}
	__syncthreads();
	int lg = LOG2N;                     // log2 of the current block length L
	if (LOG2N & 1) {
		constexpr int q = N / 2;
		for (int j = tid; j < q; j += TH) {
			const float2 a = s[SC_PAD(j)], b = s[SC_PAD(j + q)];
			s[SC_PAD(j)] = make_float2(a.x + b.x, a.y + b.y);
			s[SC_PAD(j + q)] = sc_cmul(make_float2(a.x - b.x, a.y - b.y), tw[j]);       // table 0: W_N^j
		}
		__syncthreads();
		lg -= 1;
	}
	// two radix-4 stages per pass, in registers: a thread takes the 16 points base + m q + m2 q2 (q = L / 4, q2 = L / 16), does the four
	// butterflies of block length L over m, then the four of block length L / 4 over m2: the butterflies, their operands and their
	// order are those of one stage after the other, at half the trips through LDS and half the barriers
#pragma unroll
	for (; lg >= 4; lg -= 4) {
		const int q = 1 << (lg - 2), ql2 = lg - 4, q2 = 1 << ql2;
		const float2 *__restrict__ tw1 = tw + sc_tw_off(LOG2N, lg);         // W_L^(p j) = tw1[(p - 1) q + j]
		const float2 *__restrict__ tw2 = tw + sc_tw_off(LOG2N, lg - 2);     // W_(L/4)^(p j2) = tw2[(p - 1) q2 + j2]
		for (int b = tid; b < N / 16; b += TH) {
			const int j2 = b & (q2 - 1), base = ((b >> ql2) << lg) + j2;
			float2 a[4][4];
#pragma unroll
			for (int m = 0; m < 4; m++)
#pragma unroll
				for (int m2 = 0; m2 < 4; m2++) a[m][m2] = s[SC_PAD(base + m * q + m2 * q2)];
#pragma unroll
			for (int m2 = 0; m2 < 4; m2++) {
				const int j = j2 + m2 * q2;
				sc_bfly4(a[0][m2], a[1][m2], a[2][m2], a[3][m2]);
				a[1][m2] = sc_cmul(a[1][m2], tw1[j]);
				a[2][m2] = sc_cmul(a[2][m2], tw1[q + j]);
				a[3][m2] = sc_cmul(a[3][m2], tw1[2 * q + j]);
			}
#pragma unroll
			for (int m = 0; m < 4; m++) {
				sc_bfly4(a[m][0], a[m][1], a[m][2], a[m][3]);
				if (lg > 4) {       // the last stage's twiddles are all 1
					a[m][1] = sc_cmul(a[m][1], tw2[j2]);
					a[m][2] = sc_cmul(a[m][2], tw2[q2 + j2]);
					a[m][3] = sc_cmul(a[m][3], tw2[2 * q2 + j2]);
				}
			}
#pragma unroll
			for (int m = 0; m < 4; m++)
#pragma unroll
				for (int m2 = 0; m2 < 4; m2++) s[SC_PAD(base + m * q + m2 * q2)] = a[m][m2];
		}
		__syncthreads();
	}
	if (lg == 2) {              // one radix-4 stage is left (log2 N = 2 mod 4): blocks of 4, no twiddles
		for (int b = tid; b < N / 4; b += TH) {
			float2 *sb = s + SC_PAD(4 * b);                 // four neighbours: no pad between them
			float2 a0 = sb[0], a1 = sb[1], a2 = sb[2], a3 = sb[3];
			sc_bfly4(a0, a1, a2, a3);
			sb[0] = a0; sb[1] = a1; sb[2] = a2; sb[3] = a3;
		}
		__syncthreads();
	}
	float p[PER];
#pragma unroll
	for (int r = 0; r < PER; r++) {
		const float2 v = s[SC_PAD(tid + r * TH)];
		p[r] = __builtin_fmaf(v.x, v.x, v.y * v.y);
	}
	__syncthreads();
	float *sp = (float *)s;
#pragma unroll
	for (int r = 0; r < PER; r++) sp[sc_bin_of<LOG2N>((uint32_t)(tid + r * TH))] = p[r];
	__syncthreads();
	float *row = rows + (size_t)blockIdx.x * N;
#pragma unroll
	for (int r = 0; r < PER; r++) row[tid + r * TH] = sp[tid + r * TH];
}

// A[k] += (double) p_s[k], s ascending, one lane per bin: the chain of double additions is serial by the SPEC, so the work is to keep
// it fed.  64 bins per workgroup; its 16 waves fetch a tile of 256 rows (16 loads in flight per lane) into LDS, the first wave adds
// the tile in row order.
__global__ __launch_bounds__(SC_ACC_WAVES * 64) void sd_scan_acc_kernel(const float *__restrict__ rows, uint32_t n_rows, uint32_t n, double *__restrict__ acc)
{
	__shared__ float tile[SC_ACC_TILE][SC_ACC_BINS];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t k = blockIdx.x * SC_ACC_BINS + lane;              // < n: n is a multiple of 64
	double a = w == 0 ? acc[k] : 0.0;
	for (uint32_t r0 = 0; r0 < n_rows; r0 += SC_ACC_TILE) {
		float v[SC_ACC_PER];
#pragma unroll
		for (int u = 0; u < SC_ACC_PER; u++) {
			const uint32_t r = r0 + w * SC_ACC_PER + u;
			v[u] = r < n_rows ? rows[(size_t)r * n + k] : 0.0f;
		}
#pragma unroll
		for (int u = 0; u < SC_ACC_PER; u++) tile[w * SC_ACC_PER + u][lane] = v[u];
		__syncthreads();
		if (w == 0) {
			const uint32_t cnt = min((uint32_t)SC_ACC_TILE, n_rows - r0);
			for (uint32_t i = 0; i < cnt; i++) a += (double)tile[i][lane];
		}
		__syncthreads();
	}
	if (w == 0) acc[k] = a;
}

// the tail of the next submit: the last t_out samples of (tail ++ block), as float2
template <int K>
__global__ __launch_bounds__(256) void sd_scan_tail_kernel(const void *__restrict__ xin, const float2 *__restrict__ t_in, float2 *__restrict__ t_out,
	uint32_t len_in, uint32_t len_out, uint64_t skip)
{
	const sd_iq_t<K> *x = (const sd_iq_t<K> *)xin;
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= len_out) return;
	const uint64_t w = skip + i;
	t_out[i] = w < len_in ? t_in[w] : sd_iq_f2<K>(x[w - len_in]);
}

// ---------------------------------------------------------------- host
struct __attribute__((visibility("hidden"))) SondeScanner {
	int device = 0, input_kind = SONDE_INPUT_IQ, log2n = 0;
	uint32_t fs = 0, n = 0;
	size_t max_in = 0;
	int64_t total = 0;                  // samples since create / reset
	int64_t segs = 0;                   // whole segments launched since create / reset
	uint32_t tail_len = 0;              // raw samples carried: total - segs N / 2
	hipStream_t last = nullptr;
	uint32_t max_rows = 0;              // power rows per launch pair
	DevBuf<float> d_win, d_rows;
	DevBuf<float2> d_tw;
	DevPair<float2> d_tail;
	DevBuf<double> d_acc;
};

static int sc_rate_ok(uint32_t fs, const char *fn)
{
	if (fs < 1000000u || fs > 20000000u) return sd_fail((std::string(fn) + ": rate_in must be 1 000 000 .. 20 000 000 Hz").c_str());
	return 0;
}

static int sc_log2(uint32_t n)
{
	for (int l = SC_MIN_LOG2; l <= SC_MAX_LOG2; l++) if (n == (1u << l)) return l;
	return -1;
}

static uint32_t sc_auto_n(uint32_t fs)
{
	uint32_t n = 1u << SC_MIN_LOG2;
	while (n < (1u << SC_MAX_LOG2) && (uint64_t)n * 1000u < fs) n <<= 1;      // Fs / N <= 1000 Hz
	return n;
}

static void sc_window(uint32_t n, float *w)
{
	for (uint32_t i = 0; i < n; i++) w[i] = (float)(0.5 - 0.5 * cos(2.0 * SD_PI * (double)i / (double)n));
}

extern "C" int sonde_scan_window(uint32_t n, float *w, size_t cap)
{
	if (sc_log2(n) < 0) return sd_fail("sonde_scan_window: fft_size must be a power of two, 1024 .. 16384");
	if (w && cap) {
		std::vector<float> v(n);
		sc_window(n, v.data());
		for (size_t i = 0; i < n && i < cap; i++) w[i] = v[i];
	}
	return (int)n;
}

extern "C" int sonde_scan_auto_fft_size(uint32_t rate_in)
{
	if (sc_rate_ok(rate_in, "sonde_scan_auto_fft_size")) return -1;
	return (int)sc_auto_n(rate_in);
}

extern "C" void sonde_scan_destroy(SondeScanner *s)
{
	if (!s) return;
	(void)hipSetDevice(s->device);
	delete s;
}

// Everything behind the argument checks: the window, the twiddles, the power rows, the zeroed accumulator and tail; on failure
// sonde_scan_create destroys what has been built so far.
static int sc_build(SondeScanner *s)
{
	const uint32_t n = s->n;
	const int lg = s->log2n;
	std::vector<float> w(n);
	sc_window(n, w.data());
	// the twiddles W_L^m = exp(-2 pi i m / L), double on the host, stored as float; exactly 1 at m = 0
	const auto tw_of = [](uint64_t m, uint64_t L) {
		const double a = -2.0 * SD_PI * (double)(m % L) / (double)L;
		return m % L ? make_float2((float)cos(a), (float)sin(a)) : make_float2(1.0f, 0.0f);
	};
	const size_t ntw = (size_t)sc_tw_off(lg, 2);
	std::vector<float2> tw(ntw);
	if (lg & 1) for (uint32_t j = 0; j < n / 2; j++) tw[j] = tw_of(j, n);
	for (int l = lg - (lg & 1); l > 2; l -= 2) {
		const uint32_t q = 1u << (l - 2);
		float2 *t = tw.data() + sc_tw_off(lg, l);
		for (uint32_t p = 1; p <= 3; p++) for (uint32_t j = 0; j < q; j++) t[(p - 1) * q + j] = tw_of((uint64_t)p * j, (uint64_t)1 << l);
	}
	const size_t cap_rows = std::min<size_t>(SC_ROWS_MAX, SC_ROW_BYTES / (n * sizeof(float)));
	const size_t max_rows = std::min<size_t>(cap_rows, (s->max_in + n - 1) / (n / 2) + 1);
	s->max_rows = (uint32_t)max_rows;
	HIPCHK(s->d_win.upload(w.data(), n));
	HIPCHK(s->d_tw.upload(tw.data(), ntw));
	HIPCHK(s->d_rows.alloc(max_rows * n));
	HIPCHK(s->d_acc.zeros(n));
	HIPCHK(s->d_tail.zeros(n));
	return 0;
}

extern "C" int sonde_scan_create(uint32_t rate_in, uint32_t fft_size, size_t max_in, int input_kind, int device, SondeScanner **out)
{
	if (!out) return sd_fail("sonde_scan_create: bad argument");
	if (sc_rate_ok(rate_in, "sonde_scan_create")) return -1;
	const uint32_t n = fft_size ? fft_size : sc_auto_n(rate_in);
	const int lg = sc_log2(n);
	if (lg < 0) return sd_fail("sonde_scan_create: fft_size must be a power of two, 1024 .. 16384 (0 = by rate_in)");
	if (!sd_input_complex(input_kind))
		return sd_fail("sonde_scan_create: input_kind must be SONDE_INPUT_IQ, SONDE_INPUT_IQ16 or SONDE_INPUT_IQ8 (the scanner takes complex samples)");
	if (!max_in || max_in >= ((size_t)1 << 31)) return sd_fail("sonde_scan_create: max_in must be 1 .. 2^31 - 1");
	if (sd_select_device(device, "sonde_scan_create")) return -1;
	SondeScanner *s = new SondeScanner;
	s->device = device; s->input_kind = input_kind; s->log2n = lg; s->fs = rate_in; s->n = n; s->max_in = max_in;
	if (sc_build(s)) { sonde_scan_destroy(s); return -1; }       // (destroy leaves the error text alone)
	*out = s;
	return 0;
}

extern "C" int sonde_scan_fft_size(const SondeScanner *s) { return s ? (int)s->n : sd_fail("sonde_scan_fft_size: null argument"); }

template <int K, int LOG2N>
static void sc_launch(SondeScanner *s, hipStream_t st, const void *x, const float2 *tail, int64_t rel, uint32_t rows)
{
	hipLaunchKernelGGL((sd_scan_kernel<K, LOG2N>), dim3(rows), dim3(ScCfg<LOG2N>::TH), 0, st, x, tail, rel, (int64_t)s->tail_len, s->d_win, s->d_tw, s->d_rows);
}

extern "C" int sonde_scan_submit(SondeScanner *s, const void *wide_dev, size_t n_in, void *stream)
{
	if (!s) return sd_fail("sonde_scan_submit: null argument");
	if (!n_in || n_in > s->max_in) return sd_fail("sonde_scan_submit: n_in must be 1 .. max_in");
	if (!wide_dev) return sd_fail("sonde_scan_submit: null argument");
	if ((uintptr_t)wide_dev % sd_sample_bytes(s->input_kind)) return sd_fail("sonde_scan_submit: the block is not aligned to the sample size");
	HIPCHK(hipSetDevice(s->device));
	hipStream_t st = (hipStream_t)stream;
	const int64_t N = s->n, half = N / 2;
	const int64_t total = s->total + (int64_t)n_in;
	const int64_t segs = total < N ? 0 : (total - N) / half + 1;          // whole segments since create / reset
	const int64_t n_base = s->total;                                      // absolute index of the block's first sample
	const float2 *t_in = s->d_tail.in();
	float2 *t_out = s->d_tail.out();
	const uint32_t tail_out = (uint32_t)(total - segs * half);            // < N
	sd_input_dispatch(s->input_kind, [&](auto kk) {
		constexpr int K = decltype(kk)::value;
		if constexpr (K != SONDE_INPUT_REAL) {
			for (int64_t s0 = s->segs; s0 < segs; s0 += s->max_rows) {
				const uint32_t rows = (uint32_t)std::min<int64_t>(s->max_rows, segs - s0);
				const int64_t rel = s0 * half - n_base;                     // >= -tail_len
				switch (s->log2n) {
				case 10: sc_launch<K, 10>(s, st, wide_dev, t_in, rel, rows); break;
				case 11: sc_launch<K, 11>(s, st, wide_dev, t_in, rel, rows); break;
				case 12: sc_launch<K, 12>(s, st, wide_dev, t_in, rel, rows); break;
				case 13: sc_launch<K, 13>(s, st, wide_dev, t_in, rel, rows); break;
				default: sc_launch<K, 14>(s, st, wide_dev, t_in, rel, rows); break;
				}
				hipLaunchKernelGGL(sd_scan_acc_kernel, dim3(s->n / SC_ACC_BINS), dim3(SC_ACC_WAVES * 64), 0, st, s->d_rows, rows, s->n, s->d_acc);
			}
			if (tail_out)
				hipLaunchKernelGGL(sd_scan_tail_kernel<K>, dim3((tail_out + 255) / 256), dim3(256), 0, st, wide_dev, t_in, t_out, s->tail_len, tail_out,
					(uint64_t)s->tail_len + n_in - tail_out);
		}
	});
	HIPCHK_IN("sonde_scan_submit", hipGetLastError());
	s->d_tail.flip();
	s->total = total;
	s->segs = segs;
	s->tail_len = tail_out;
	s->last = st;
	return 0;
}

static int sc_sync(SondeScanner *s, const char *fn)
{
	HIPCHK(hipSetDevice(s->device));
	const hipError_t e = hipStreamSynchronize(s->last);
	if (e != hipSuccess) return sd_fail((std::string(fn) + ": hipStreamSynchronize").c_str(), e);
	return 0;
}

extern "C" int sonde_scan_reset(SondeScanner *s)
{
	if (!s) return sd_fail("sonde_scan_reset: null argument");
	if (sc_sync(s, "sonde_scan_reset")) return -1;
	hipError_t e = hipMemset(s->d_acc, 0, s->n * sizeof(double));
	if (e != hipSuccess) return sd_fail("sonde_scan_reset: hipMemset", e);
	s->total = 0; s->segs = 0; s->tail_len = 0;
	return 0;
}

extern "C" long long sonde_scan_segments(SondeScanner *s)
{
	if (!s) return sd_fail("sonde_scan_segments: null argument");
	if (sc_sync(s, "sonde_scan_segments")) return -1;
	return (long long)s->segs;
}

extern "C" int sonde_scan_spectrum(SondeScanner *s, float *P, size_t cap)
{
	if (!s || !P) return sd_fail("sonde_scan_spectrum: null argument");
	if (cap < s->n) return sd_fail("sonde_scan_spectrum: the buffer is shorter than fft_size");
	if (!s->segs) return sd_fail("sonde_scan_spectrum: no whole segment yet (fft_size samples are needed)");
	if (sc_sync(s, "sonde_scan_spectrum")) return -1;
	std::vector<double> a(s->n);
	hipError_t e = hipMemcpy(a.data(), s->d_acc, s->n * sizeof(double), hipMemcpyDeviceToHost);
	if (e != hipSuccess) return sd_fail("sonde_scan_spectrum: hipMemcpy", e);
	const uint32_t n = s->n, half = n / 2;
	const double S = (double)s->segs;
	for (uint32_t k = 0; k < n; k++) P[(k + half) & (n - 1)] = (float)(a[k] / S);      // ascending frequency: bin i <-> (i - N / 2) Fs / N
	return (int)n;
}

// ---------------------------------------------------------------- the search (SPEC 3.10: host, double, from the float32 P)
static double sc_rnd(double x) { return floor(x + 0.5); }

extern "C" int sonde_scan_search(const float *P, uint32_t n, uint32_t rate_in, const SondeScanParams *p, SondeScanCandidate *out, size_t cap)
{
	if (!P || (!out && cap)) return sd_fail("sonde_scan_search: null argument");
	if (sc_log2(n) < 0) return sd_fail("sonde_scan_search: fft_size must be a power of two, 1024 .. 16384");
	if (sc_rate_ok(rate_in, "sonde_scan_search")) return -1;
	if (p && p->struct_size != sizeof(SondeScanParams)) return sd_fail("sonde_scan_search: SondeScanParams.struct_size is not sizeof(SondeScanParams)");
	const double smooth_hz = p && p->smooth_hz ? p->smooth_hz : 8000.0, min_sep_hz = p && p->min_sep_hz ? p->min_sep_hz : 10000.0;
	const double centroid_hz = p && p->centroid_hz ? p->centroid_hz : 16000.0;
	const double thr = p && p->threshold != 0.0f ? (double)p->threshold : 4.0;
	if (!(thr > 0.0)) return sd_fail("sonde_scan_search: threshold must be positive (a linear power ratio)");
	const double delta = (double)rate_in / (double)n;
	const int64_t N = n;
	const int64_t h = std::max<int64_t>(1, (int64_t)sc_rnd(smooth_hz / (2.0 * delta))), W = 2 * h + 1;
	const int64_t g = std::max<int64_t>(1, (int64_t)sc_rnd(centroid_hz / (2.0 * delta)));
	const int64_t D = std::max<int64_t>(1, (int64_t)sc_rnd(min_sep_hz / delta));
	if (N - 2 * h < 1 || N - 2 * g < 1) return sd_fail("sonde_scan_search: smooth_hz or centroid_hz is wider than the band");
	std::vector<double> c(N + 1), S(N, 0.0);
	c[0] = 0.0;
	for (int64_t j = 0; j < N; j++) c[j + 1] = c[j] + (double)P[j];
	for (int64_t i = h; i <= N - 1 - h; i++) S[i] = c[i + h + 1] - c[i - h];
	std::vector<double> srt(S.begin() + h, S.begin() + (N - h));
	std::sort(srt.begin(), srt.end());
	const size_t m = srt.size();
	const double floor_ = (m & 1) ? srt[m / 2] : (srt[m / 2 - 1] + srt[m / 2]) / 2.0;
	const double n0 = floor_ / (double)W;
	const int64_t lo = std::max(h, g), hi = N - 1 - std::max(h, g);
	size_t count = 0;
	for (int64_t i = lo; i <= hi; i++) {
		if (!(S[i] >= thr * floor_)) continue;
		const int64_t a0 = std::max(h, i - D), b0 = std::min(N - 1 - h, i + D);
		bool peak = true;
		for (int64_t j = a0; j < i && peak; j++) peak = S[j] < S[i];
		for (int64_t j = i + 1; j <= b0 && peak; j++) peak = S[j] <= S[i];
		if (!peak) continue;
		double se = 0.0, sj = 0.0;
		for (int64_t j = i - g; j <= i + g; j++) {
			const double e = (double)P[j] - n0;
			se += e;
			sj += e * (double)j;
		}
		if (!(se > 0.0)) continue;
		const double cen = sj / se;
		const int64_t a = std::max<int64_t>(0, i - D), b = std::min(N - 1, i + D);
		double E = 0.0;
		for (int64_t j = a; j <= b; j++) E += std::max((double)P[j] - n0, 0.0);
		int64_t j05 = -1, j95 = -1;
		double run = 0.0;
		for (int64_t j = a; j <= b; j++) {
			run += std::max((double)P[j] - n0, 0.0);
			if (j05 < 0 && run >= 0.05 * E) j05 = j;
			if (j95 < 0 && run >= 0.95 * E) j95 = j;
		}
		if (count < cap) {
			SondeScanCandidate &o = out[count];
			o.offset_hz = (int32_t)sc_rnd((cen - (double)(N / 2)) * delta);
			o.bandwidth_hz = (uint32_t)sc_rnd((double)(j95 - j05 + 1) * delta);
			o.cn0_dbhz = (float)(10.0 * log10(E * delta / n0));
			o.excess_db = (float)(10.0 * log10(S[i] / floor_));
			o.bin = (uint32_t)i;
		}
		count++;
	}
	return (int)count;
}

extern "C" int sonde_scan_candidates(SondeScanner *s, const SondeScanParams *p, SondeScanCandidate *out, size_t cap)
{
	if (!s) return sd_fail("sonde_scan_candidates: null argument");
	std::vector<float> P(s->n);
	if (sonde_scan_spectrum(s, P.data(), P.size()) < 0) return -1;
	return sonde_scan_search(P.data(), s->n, s->fs, p, out, cap);
}
