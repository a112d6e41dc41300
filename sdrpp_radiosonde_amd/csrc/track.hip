// track.hip -- carrier meter (DESIGN SPEC 3.11): per row of complex samples at rate R (the rows sonde_tuner_process writes) and per
// look of L samples, the lag-d autocorrelation A = sum x[m] conj(x[m - d]) and the power P = sum |x[m]|^2, from which the host reads
// how far the carrier is from the VFO's centre (arg A), how strong it is (P) and how much of it is carrier (|A| / P); and the
// pure-host step rule that turns one look into the VFO's next offset (sonde_track_step).  It stands where a person watches the
// SDR++ waterfall and drags the VFO after a drifting sonde (/root/reference/src/main.cpp:55-68).
//
// One workgroup per (row, look-piece): the part of one look that lies in this submit, summed in sd_blocksum.h's order -- float32
// products with one explicit fmaf, 256-sample blocks, block sums into three doubles in ascending order, the carry being what they
// start from.  A look's sums therefore depend on the row's samples and its restart points alone, never on how the stream was cut
// into submits.  A finished look goes to the row's ring, an unfinished one to the carry; the carry and the lag history (the row's
// last d samples) are double-buffered, because the workgroup that writes them is not the one that reads them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <deque>
#include <string>
#include <vector>
#include "launch.h"
#include "sd_host.h"
#include "sd_devmem.h"
#include "sd_design.h"
#include "sd_blocksum.h"
#include "../../include/sonde_abi.h"

#define TK_VMAX   512                   // rows per launch: their look phases and ring slots travel with the launch, by value (2 KB)
#define TK_DMAX   64                    // largest lag
#define TK_MAXLB  16384                 // largest look, in blocks (the phase travels in 15 bits)
#define TK_FRESH  0x8000u               // the row starts here: no lag history, no carry

struct SdTrackRows { uint16_t ph[TK_VMAX]; uint16_t slot[TK_VMAX]; };     // blocks into the row's current look (| TK_FRESH); ring slot of its next look

__global__ __launch_bounds__(SD_BS_WG) void sd_track_kernel(const float2 *__restrict__ rows, size_t stride, uint32_t nb, uint32_t LB, uint32_t d,
	SdTrackRows rs, uint32_t vbase, const float2 *__restrict__ hist_in, float2 *__restrict__ hist_out,
	const double *__restrict__ carry_in, double *__restrict__ carry_out, double *__restrict__ ring, uint32_t ring_len)
{
	__shared__ float s_bs[3][SD_BS_CHUNK];
	const uint32_t tid = threadIdx.x;
	const uint32_t row = vbase + blockIdx.y;
	const uint32_t ph = rs.ph[blockIdx.y] & (TK_FRESH - 1u);
	const bool fresh = (rs.ph[blockIdx.y] & TK_FRESH) != 0;
	// piece p of the row: blocks [b0, b1) of the submit
	const uint32_t first = LB - ph;                                       // blocks of piece 0 if the submit is long enough
	const uint32_t p = blockIdx.x;
	const uint32_t b0 = p == 0 ? 0u : first + (p - 1u) * LB;
	if (b0 >= nb) return;
	const uint32_t b1 = min(nb, p == 0 ? first : b0 + LB);
	const float2 *x = rows + (size_t)row * stride;
	const float2 *hi = hist_in + (size_t)row * TK_DMAX;
	double acc = 0.0;
	if (p == 0 && ph > 0 && tid < 3) acc = carry_in[(size_t)row * 3 + tid];
	// A (re, im) and P of sample m: x[m] against x[m - d], which in front of the submit is the row's history, or nothing
	struct Pair { float2 x, y; };
	acc = sd_blocksum<3>(b0, b1, acc, s_bs,
		[&](int64_t m) {
			const int64_t ml = m - (int64_t)d;
			return Pair{ x[m], ml >= 0 ? x[ml] : (fresh ? make_float2(0.0f, 0.0f) : hi[ml + (int64_t)d]) };
		},
		[](const Pair &v, float (&q)[3]) {
			q[0] = __builtin_fmaf(v.x.x, v.y.x, v.x.y * v.y.y);
			q[1] = __builtin_fmaf(v.x.y, v.y.x, -(v.x.x * v.y.y));
			q[2] = __builtin_fmaf(v.x.x, v.x.x, v.x.y * v.x.y);
		});
	const bool done = (p == 0 ? ph : 0u) + (b1 - b0) == LB;                // the look ends in this submit
	if (tid < 3) {
		if (done) ring[((size_t)row * ring_len + (rs.slot[blockIdx.y] + p) % ring_len) * 3 + tid] = acc;
		else carry_out[(size_t)row * 3 + tid] = acc;
	}
	if (b1 == nb && tid < d) hist_out[(size_t)row * TK_DMAX + tid] = x[(size_t)nb * SD_BS_BLK - d + tid];
}

// ---------------------------------------------------------------- host
struct SdTrackPending { uint64_t seq, look; };
struct SondeTracker {
	int device = 0;
	uint32_t n_rows = 0, rate = 0, max_samples = 0, L = 0, LB = 0, d = 0, ring_len = 0;
	hipStream_t last = nullptr;
	std::vector<uint32_t> ph;           // blocks into the current look, per row
	std::vector<uint8_t> fresh;         // the row starts at the next submit
	std::vector<uint64_t> look, seq;    // index of the look in progress (from the last restart); looks finished since create
	std::vector<std::deque<SdTrackPending>> pending;
	std::vector<uint64_t> dropped;
	DevPair<float2> d_hist;
	DevPair<double> d_carry;
	DevBuf<double> d_ring;
};

extern "C" void sonde_track_destroy(SondeTracker *t)
{
	if (!t) return;
	(void)hipSetDevice(t->device);
	delete t;
}

// Everything behind the argument checks; on failure sonde_track_create destroys what has been built so far.
static int tk_build(SondeTracker *t)
{
	HIPCHK(t->d_hist.zeros((size_t)t->n_rows * TK_DMAX));
	HIPCHK(t->d_carry.zeros((size_t)t->n_rows * 3));
	HIPCHK(t->d_ring.zeros((size_t)t->n_rows * 3 * t->ring_len));
	return 0;
}

extern "C" int sonde_track_defaults(uint32_t rate, uint32_t *look_samples, uint32_t *lag)
{
	if (rate < 5000u || rate > 100000u) return sd_fail("sonde_track_defaults: rate must be 5000 .. 100 000 Hz");
	if (look_samples) *look_samples = SD_BS_BLK * ((rate + 2559u) / 2560u);
	if (lag) *lag = rate / 24000u > 1u ? rate / 24000u : 1u;
	return 0;
}

extern "C" int sonde_track_create(uint32_t n_rows, uint32_t rate, uint32_t max_samples, uint32_t look_samples, uint32_t lag, int input_kind,
	int device, SondeTracker **out)
{
	if (!out || !n_rows) return sd_fail("sonde_track_create: bad argument");
	if (input_kind != SONDE_INPUT_IQ)
		return sd_fail("sonde_track_create: input_kind must be SONDE_INPUT_IQ (the meter takes the tuner's complex64 rows; REAL rows carry no carrier)");
	uint32_t L0, d0;
	if (sonde_track_defaults(rate, &L0, &d0)) return sd_fail("sonde_track_create: rate must be 5000 .. 100 000 Hz");
	const uint32_t L = look_samples ? look_samples : L0, d = lag ? lag : d0;
	if (L % SD_BS_BLK || L / SD_BS_BLK > TK_MAXLB) return sd_fail("sonde_track_create: look_samples must be a multiple of 256, at most 4 194 304 (0 = about 0.1 s)");
	if (d > TK_DMAX) return sd_fail("sonde_track_create: lag must be 1 .. 64 (0 = by rate)");
	if (!max_samples || max_samples % SD_BS_BLK || max_samples >= (1u << 30)) return sd_fail("sonde_track_create: max_samples must be a positive multiple of 256 below 2^30");
	if ((max_samples / SD_BS_BLK) / (L / SD_BS_BLK) + 2 > 65535u) return sd_fail("sonde_track_create: max_samples holds more than 65 533 looks");
	if (sd_select_device(device, "sonde_track_create")) return -1;
	SondeTracker *t = new SondeTracker;
	t->device = device; t->n_rows = n_rows; t->rate = rate; t->max_samples = max_samples; t->L = L; t->LB = L / SD_BS_BLK; t->d = d;
	const uint32_t per_submit = (max_samples / SD_BS_BLK) / t->LB + 2;       // looks one submit can finish, and one more
	t->ring_len = per_submit > 16u ? per_submit : 16u;
	t->ph.assign(n_rows, 0); t->fresh.assign(n_rows, 1); t->look.assign(n_rows, 0); t->seq.assign(n_rows, 0);
	t->pending.resize(n_rows); t->dropped.assign(n_rows, 0);
	if (tk_build(t)) { sonde_track_destroy(t); return -1; }       // (destroy leaves the error text alone)
	*out = t;
	return 0;
}

extern "C" int sonde_track_look_samples(const SondeTracker *t) { return t ? (int)t->L : sd_fail("sonde_track_look_samples: null argument"); }
extern "C" int sonde_track_lag(const SondeTracker *t) { return t ? (int)t->d : sd_fail("sonde_track_lag: null argument"); }
extern "C" int sonde_track_ring(const SondeTracker *t) { return t ? (int)t->ring_len : sd_fail("sonde_track_ring: null argument"); }

extern "C" int sonde_track_submit(SondeTracker *t, const void *rows_dev, size_t n_samples, size_t row_stride, void *stream)
{
	if (!t || !rows_dev) return sd_fail("sonde_track_submit: null argument");
	if (!n_samples || n_samples % SD_BS_BLK || n_samples > t->max_samples)
		return sd_fail("sonde_track_submit: n_samples must be a positive multiple of 256 and <= max_samples");
	if (row_stride < n_samples) return sd_fail("sonde_track_submit: row_stride shorter than the row");
	if ((uintptr_t)rows_dev & 7u) return sd_fail("sonde_track_submit: rows must be 8-byte aligned");
	HIPCHK(hipSetDevice(t->device));
	hipStream_t s = (hipStream_t)stream;
	const uint32_t nb = (uint32_t)(n_samples / SD_BS_BLK), LB = t->LB;
	const dim3 wg(SD_BS_WG);
	for (uint32_t vb = 0; vb < t->n_rows; vb += TK_VMAX) {
		const uint32_t nv = t->n_rows - vb < TK_VMAX ? t->n_rows - vb : TK_VMAX;
		SdTrackRows rs = {};
		for (uint32_t i = 0; i < nv; i++) {
			rs.ph[i] = (uint16_t)(t->ph[vb + i] | (t->fresh[vb + i] ? TK_FRESH : 0u));
			rs.slot[i] = (uint16_t)(t->seq[vb + i] % t->ring_len);
		}
		const dim3 grid((nb + LB - 1) / LB + 1, nv);
		hipLaunchKernelGGL(sd_track_kernel, grid, wg, 0, s, (const float2 *)rows_dev, row_stride, nb, LB, t->d, rs, vb, t->d_hist.in(), t->d_hist.out(),
			t->d_carry.in(), t->d_carry.out(), t->d_ring, t->ring_len);
	}
	HIPCHK_IN("sonde_track_submit", hipGetLastError());
	for (uint32_t r = 0; r < t->n_rows; r++) {
		const uint32_t tot = t->ph[r] + nb, fin = tot / LB;
		for (uint32_t i = 0; i < fin; i++) {
			t->pending[r].push_back({t->seq[r]++, t->look[r]++});
			if (t->pending[r].size() > t->ring_len) { t->pending[r].pop_front(); t->dropped[r]++; }
		}
		t->ph[r] = tot % LB;
		t->fresh[r] = 0;
	}
	t->d_hist.flip();
	t->d_carry.flip();
	t->last = s;
	return 0;
}

extern "C" int sonde_track_restart(SondeTracker *t, uint32_t row)
{
	if (!t) return sd_fail("sonde_track_restart: null argument");
	if (row >= t->n_rows) return sd_fail("sonde_track_restart: no such row");
	t->ph[row] = 0; t->fresh[row] = 1; t->look[row] = 0;
	return 0;
}

extern "C" int sonde_track_results(SondeTracker *t, SondeTrackLook *out, size_t cap, uint64_t *dropped)
{
	if (!t || (!out && cap)) return sd_fail("sonde_track_results: null argument");
	size_t count = 0;
	for (uint32_t r = 0; r < t->n_rows; r++) count += t->pending[r].size();
	if (cap < count) return sd_fail("sonde_track_results: the buffer is shorter than n_rows * sonde_track_ring()");
	HIPCHK(hipSetDevice(t->device));
	hipError_t e = hipStreamSynchronize(t->last);
	if (e != hipSuccess) return sd_fail("sonde_track_results: hipStreamSynchronize", e);
	std::vector<double> ring((size_t)t->n_rows * t->ring_len * 3);
	if (count && (e = hipMemcpy(ring.data(), t->d_ring, ring.size() * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
		return sd_fail("sonde_track_results: hipMemcpy", e);
	size_t k = 0;
	for (uint32_t r = 0; r < t->n_rows; r++) {
		for (const SdTrackPending &p : t->pending[r]) {
			const double *v = ring.data() + ((size_t)r * t->ring_len + p.seq % t->ring_len) * 3;
			out[k].row = r; out[k].reserved = 0; out[k].look = p.look; out[k].a_re = v[0]; out[k].a_im = v[1]; out[k].p = v[2];
			k++;
		}
		t->pending[r].clear();
		if (dropped) dropped[r] = t->dropped[r];
		t->dropped[r] = 0;
	}
	return (int)count;
}

// ---------------------------------------------------------------- the host conversions and the step rule (SPEC 3.11: pure host, double)
extern "C" double sonde_track_err_hz(uint32_t rate, uint32_t lag, double a_re, double a_im)
{
	return (double)rate / (2.0 * SD_PI * (double)lag) * atan2(a_im, a_re);
}

extern "C" double sonde_track_level_db(double p, uint32_t look_samples) { return 10.0 * log10(p / (double)look_samples); }

extern "C" double sonde_track_quality(double a_re, double a_im, double p) { return p > 0.0 ? sqrt(a_re * a_re + a_im * a_im) / p : 0.0; }

extern "C" int sonde_track_step(int32_t offset_hz, uint32_t bandwidth_hz, uint32_t rate_in, uint32_t rate, uint32_t lag, const SondeTrackLook *look,
	const SondeTrackParams *p, int32_t *new_offset)
{
	if (!look || !new_offset) return sd_fail("sonde_track_step: null argument");
	if (p && p->struct_size != sizeof(SondeTrackParams)) return sd_fail("sonde_track_step: SondeTrackParams.struct_size is not sizeof(SondeTrackParams)");
	if (!rate || !lag || !rate_in || bandwidth_hz > rate_in) return sd_fail("sonde_track_step: rate, lag and rate_in must be positive, bandwidth_hz at most rate_in");
	const double deadband = p && p->deadband_hz ? p->deadband_hz : (double)SONDE_TRACK_DEADBAND_HZ;
	const double max_step = p && p->max_step_hz ? p->max_step_hz : (double)SONDE_TRACK_MAX_STEP_HZ;
	const double err = sonde_track_err_hz(rate, lag, look->a_re, look->a_im);
	int64_t f = offset_hz;
	if (fabs(err) >= deadband) {
		double step = floor(err + 0.5);
		step = step > max_step ? max_step : step < -max_step ? -max_step : step;
		f += (int64_t)step;
		const int64_t lim = ((int64_t)rate_in - (int64_t)bandwidth_hz) / 2;      // |offset| + bandwidth / 2 <= rate_in / 2
		f = f > lim ? lim : f < -lim ? -lim : f;
	}
	*new_offset = (int32_t)f;
	return f != offset_hz;
}
