// tuner.hip -- wideband tuner (DESIGN SPEC 3.9): a bank of VFOs over one wideband complex stream at Fs, each at its own integer-Hz
// offset f_k and bandwidth B_k, each mixed to DC, low-pass filtered and resampled by up/down = R/Fs to complex rows at R.  It stands
// where the SDR++ VFO stands in the reference's chain (/root/reference/src/main.cpp:55-68): its rows are the IQ rows SondeBatch,
// SondeVfo and SondeDetector take.
//
// One workgroup per (VFO, tile of TN_JT outputs).  The tile's input window (T_k - 1 samples in front of its first output's i0 up to
// its last output's i0) is streamed through LDS in segments of TN_SEG samples, newest first; each segment is read from the raw
// block (or the carried history), converted exactly (sd_input.h), mixed with the VFO's phasor and stored once.  A wave owns every
// fourth output of the tile; lane l takes the taps t = l (mod 64) of each output, ascending, in one fmaf chain per component that
// runs on from segment to segment, and a fixed xor butterfly adds the 64 chains.  The order of output j's sum therefore depends on
// j alone: rows are bit-identical however the stream is cut into submits.  The history (the last H = max_k T_k - 1 raw samples, as
// float2) is double-buffered and refreshed by a second kernel behind the first.
//
// SLOTS (SPEC 3.12): the VFOs are slots that are active or idle.  The tap sets are per listed bandwidth, the history is shared and the
// mixer's phase is a function of the absolute sample index, so a VFO has no device state of its own: the mixing kernel is launched
// over the active slots only (slot, tap set, f and theta travel with the launch), a fill kernel writes zeros to the idle slots' rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <map>
#include <string>
#include <vector>
#include "launch.h"
#include "sd_host.h"
#include "sd_devmem.h"
#include "sd_design.h"
#include "sd_input.h"
#include "../../include/sonde_abi.h"

#define TN_WG    256
#define TN_JT    64                     // outputs per workgroup (16 per wave)
#define TN_SEG   4096                   // samples per LDS segment (32 KB of float2)
#define TN_VMAX  64                     // VFOs per launch: their mixer steps and phase offsets travel with the launch, by value (512 B of arguments)
#define TN_LOB   12                     // mixer: phi = hi * 2^12 + lo, two tables
#define TN_MAXUP 64

// f_k mod Fs, the phase offset theta_k, the slot (= output row) and the tap set of the launch's VFOs
struct SdTunerOffs { uint32_t F[TN_VMAX], TH[TN_VMAX], SLOT[TN_VMAX]; uint8_t SET[TN_VMAX]; };
struct SdTunerIdle { uint32_t SLOT[TN_VMAX]; };

// e = H[hi] (1 + D[lo]), D = exp(-2 pi i lo / Fs) - 1 (|D| <= 0.026): about 2^-24 per component (SPEC 3.9 allows 2^-22)
static __device__ __forceinline__ float2 tn_phasor(uint32_t phi, const float2 *__restrict__ th, const float2 *__restrict__ tl)
{
	const float2 h = th[phi >> TN_LOB], d = tl[phi & ((1u << TN_LOB) - 1u)];
	return make_float2(h.x + __builtin_fmaf(h.x, d.x, -(h.y * d.y)), h.y + __builtin_fmaf(h.x, d.y, h.y * d.x));
}

template <int K>
__global__ __launch_bounds__(TN_WG) void sd_tuner_kernel(const void *__restrict__ xin, const float2 *__restrict__ hist, uint32_t H,
	uint32_t n_out, int64_t n_base, uint32_t up, uint32_t down, uint32_t fs,
	const float *__restrict__ taps, const uint64_t *__restrict__ tapoff, const uint32_t *__restrict__ vT,
	const float2 *__restrict__ th, const float2 *__restrict__ tl, SdTunerOffs offs,
	float2 *__restrict__ out, size_t out_stride)
{
	__shared__ float2 s_v[TN_SEG];
	const sd_iq_t<K> *x = (const sd_iq_t<K> *)xin;        // (a void pointer in the signature: sd_iq_t names an anonymous enum, mangled apart on host and device)
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t k = offs.SLOT[blockIdx.y], F = offs.F[blockIdx.y], TH = offs.TH[blockIdx.y], set = offs.SET[blockIdx.y];
	const int32_t T = (int32_t)vT[set];
	const float *g = taps + tapoff[set];
	const uint32_t jt0 = blockIdx.x * TN_JT;
	const uint32_t nj = min((uint32_t)TN_JT, n_out - jt0);
	// window index w: absolute sample n_base - H + w (w < H: the history, H <= w < H + n_in: the block)
	int32_t w0[TN_JT / 4];
	uint32_t ph[TN_JT / 4];
	float ar[TN_JT / 4], ai[TN_JT / 4];
#pragma unroll
	for (int r = 0; r < TN_JT / 4; r++) {
		const uint64_t q = (uint64_t)(jt0 + min((uint32_t)(wave + 4 * r), nj - 1)) * down;      // j down - n_base up (n_base up = j_base down)
		w0[r] = (int32_t)(H + q / up);
		ph[r] = (uint32_t)(q % up);
		ar[r] = 0.0f; ai[r] = 0.0f;
	}
	const int32_t w_min = (int32_t)(H + (uint64_t)jt0 * down / up) - (T - 1);                     // >= 0: H >= T - 1
	const int32_t w_max = (int32_t)(H + (uint64_t)(jt0 + nj - 1) * down / up);
	// the mixer phase of the first sample this thread stores, then steps of 256 samples (all 32-bit: phi, D < Fs <= 2e7)
	const uint32_t d256 = (uint32_t)((256ull * F) % fs);
	for (int32_t seg_hi = w_max + 1; seg_hi > w_min;) {
		const int32_t seg_lo = max(w_min, seg_hi - TN_SEG), len = seg_hi - seg_lo;
		const int64_t s0 = n_base - (int64_t)H + seg_lo + tid;
		uint32_t phi = (uint32_t)(((uint64_t)F * (uint64_t)(((s0 % (int64_t)fs) + (int64_t)fs) % (int64_t)fs)) % fs) + TH;      // both < Fs <= 2e7
		phi -= phi >= fs ? fs : 0u;
		for (int32_t i = tid; i < len; i += TN_WG) {
			const int32_t w = seg_lo + i;
			const float2 xv = w < (int32_t)H ? hist[w] : sd_iq_f2<K>(x[w - (int32_t)H]);
			const float2 e = tn_phasor(phi, th, tl);
			s_v[i] = make_float2(__builtin_fmaf(xv.x, e.x, -(xv.y * e.y)), __builtin_fmaf(xv.x, e.y, xv.y * e.x));
			phi += d256;
			phi -= phi >= fs ? fs : 0u;
		}
		__syncthreads();
#pragma unroll
		for (int r = 0; r < TN_JT / 4; r++) {
			if ((uint32_t)(wave + 4 * r) >= nj) continue;
			// output r reads samples w0 - t for t in [t_a, t_b]: the part of its window in this segment
			const int32_t t_a = max(0, w0[r] - seg_hi + 1), t_b = min(T - 1, w0[r] - seg_lo);
			const float *gp = g + (size_t)ph[r] * (uint32_t)T;
			const float2 *vp = s_v + (w0[r] - seg_lo);
			for (int32_t t = (t_a & ~63) + lane; t <= t_b; t += 64) {
				if (t < t_a) continue;
				const float gv = gp[t];
				const float2 v = vp[-t];
				ar[r] = __builtin_fmaf(gv, v.x, ar[r]);
				ai[r] = __builtin_fmaf(gv, v.y, ai[r]);
			}
		}
		__syncthreads();
		seg_hi = seg_lo;
	}
#pragma unroll
	for (int r = 0; r < TN_JT / 4; r++) {
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) { ar[r] += __shfl_xor(ar[r], o, 64); ai[r] += __shfl_xor(ai[r], o, 64); }
		const uint32_t q = wave + 4 * r;
		if (lane == 0 && q < nj) out[(size_t)k * out_stride + jt0 + q] = make_float2(ar[r], ai[r]);
	}
}

// the rows of idle slots: zeros (bytes only, no arithmetic), so that whatever reads all rows of a submit reads defined ones
__global__ __launch_bounds__(TN_WG) void sd_tuner_fill_kernel(SdTunerIdle idle, uint32_t n_out, float2 *__restrict__ out, size_t out_stride)
{
	const uint32_t j = blockIdx.x * TN_WG + threadIdx.x;
	if (j < n_out) out[(size_t)idle.SLOT[blockIdx.y] * out_stride + j] = make_float2(0.0f, 0.0f);
}

// the history of the next submit: the last H samples of (history ++ block), as float2
template <int K>
__global__ __launch_bounds__(TN_WG) void sd_tuner_hist_kernel(const void *__restrict__ xin, const float2 *__restrict__ h_in,
	float2 *__restrict__ h_out, uint32_t H, uint32_t n_in)
{
	const sd_iq_t<K> *x = (const sd_iq_t<K> *)xin;
	const uint32_t i = blockIdx.x * TN_WG + threadIdx.x;
	if (i >= H) return;
	const uint64_t w = (uint64_t)n_in + i;
	h_out[i] = w < H ? h_in[w] : sd_iq_f2<K>(x[w - H]);
}

// ---------------------------------------------------------------- host
struct SondeTuner {
	int device = 0, input_kind = SONDE_INPUT_IQ;
	uint32_t fs = 0, rate_out = 0, up = 0, down = 0, n_vfos = 0, H = 0;
	size_t max_in = 0;
	std::vector<int32_t> offset;        // Hz, per VFO
	std::vector<uint32_t> theta;        // the mixer's phase offset, 0 .. Fs - 1, per VFO (0 unless retuned continuously)
	std::vector<uint32_t> bw;           // Hz, per VFO
	std::vector<uint8_t> set, active;   // per VFO (slot): its tap set, and whether it is tuned at all
	std::map<uint32_t, uint32_t> set_of;        // listed bandwidth -> tap set (ascending bandwidth)
	int64_t n_base = 0;                 // absolute input index of the next submit's first sample
	bool started = false;               // it has processed or been retuned (sonde_tuner_test_set_base refuses it then)
	DevBuf<float> d_taps;
	DevBuf<uint64_t> d_tapoff;
	DevBuf<uint32_t> d_T;
	DevBuf<float2> d_th, d_tl;
	DevPair<float2> d_hist;
};

static uint64_t tn_gcd(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }

static int tn_ratio(uint32_t fs, uint32_t r, uint32_t *up, uint32_t *down, const char *fn)
{
	if (fs < 1000000u || fs > 20000000u) return sd_fail((std::string(fn) + ": rate_in must be 1 000 000 .. 20 000 000 Hz").c_str());
	if (r == 0 || r > 100000u || 8ull * r > fs) return sd_fail((std::string(fn) + ": rate_out must be 1 .. 100 000 Hz and at most rate_in / 8").c_str());
	const uint64_t g = tn_gcd(fs, r);
	if (r / g > TN_MAXUP) return sd_fail((std::string(fn) + ": rate_out / rate_in in lowest terms has a numerator above 64").c_str());
	*up = (uint32_t)(r / g);
	*down = (uint32_t)(fs / g);
	return 0;
}

static uint32_t tn_T(uint32_t fs, uint32_t b) { return 32u * ((fs + b - 1) / b); }

// SPEC 3.9: the prototype of SPEC 3.7 (sd_design.h) with N = up T taps, cutoff B / 2 at Fs up, as `up` rows of unit DC gain
static void tn_taps(uint32_t up, uint32_t T, double fs_up, double cutoff_hz, float *g)
{
	sd_design_rows(sd_design_prototype((size_t)up * T, cutoff_hz / fs_up), up, T, g);
}

extern "C" int sonde_tuner_ratio(uint32_t rate_in, uint32_t rate_out, int *up, int *down)
{
	uint32_t u, d;
	if (tn_ratio(rate_in, rate_out, &u, &d, "sonde_tuner_ratio")) return -1;
	if (up) *up = (int)u;
	if (down) *down = (int)d;
	return 0;
}

extern "C" int sonde_tuner_taps(uint32_t rate_in, uint32_t rate_out, uint32_t bandwidth_hz, float *g, size_t cap)
{
	uint32_t up, down;
	if (tn_ratio(rate_in, rate_out, &up, &down, "sonde_tuner_taps")) return -1;
	const uint32_t b = bandwidth_hz ? bandwidth_hz : rate_out;
	if (b < 5000u || b > rate_out) return sd_fail("sonde_tuner_taps: bandwidth_hz must be 5000 .. rate_out (0 = rate_out)");
	const uint32_t T = tn_T(rate_in, b);
	const size_t N = (size_t)up * T;
	if (g && cap) {
		std::vector<float> v(N);
		tn_taps(up, T, (double)rate_in * up, 0.5 * b, v.data());
		for (size_t i = 0; i < N && i < cap; i++) g[i] = v[i];
	}
	return (int)N;
}

extern "C" void sonde_tuner_destroy(SondeTuner *t)
{
	if (!t) return;
	(void)hipSetDevice(t->device);
	delete t;
}

static int tn_check_offset(uint32_t fs, uint32_t b, int32_t f, const char *fn)
{
	if (2 * llabs((long long)f) + (long long)b > (long long)fs)
		return sd_fail((std::string(fn) + ": a VFO must lie inside the band (|offset_hz| + bandwidth_hz / 2 <= rate_in / 2)").c_str());
	return 0;
}

// Everything behind the argument checks: one tap set per listed bandwidth (ascending), the mixer tables and the zeroed history; on
// failure tn_create destroys what has been built so far.
static int tn_build(SondeTuner *t, const std::map<uint32_t, uint32_t> &sets /* bandwidth -> T */)
{
	const uint32_t rate_in = t->fs, up = t->up, n_slots = t->n_vfos;
	// the tap sets, one per distinct bandwidth, back to back
	const uint32_t n_sets = (uint32_t)sets.size();
	std::vector<uint64_t> tapoff(n_sets);
	std::vector<uint32_t> T(n_sets);
	size_t total = 0;
	uint32_t si = 0;
	for (auto &s : sets) { t->set_of[s.first] = si; tapoff[si] = total; T[si] = s.second; total += (size_t)up * s.second; si++; }
	std::vector<float> g(total);
	for (auto &s : sets) tn_taps(up, s.second, (double)rate_in * up, 0.5 * s.first, g.data() + tapoff[t->set_of[s.first]]);
	t->offset.assign(n_slots, 0);
	t->theta.assign(n_slots, 0);
	t->bw.assign(n_slots, 0);
	t->set.assign(n_slots, 0);
	t->active.assign(n_slots, 0);
	// the mixer tables (double on the host, stored as float): H[h] = exp(-2 pi i h 2^12 / Fs), D[l] = exp(-2 pi i l / Fs) - 1
	const uint32_t nh = (rate_in + (1u << TN_LOB) - 1) >> TN_LOB, nl = 1u << TN_LOB;
	std::vector<float2> th(nh), tl(nl);
	for (uint32_t h = 0; h < nh; h++) {
		const double a = -2.0 * SD_PI * (double)(((uint64_t)h << TN_LOB) % rate_in) / (double)rate_in;
		th[h] = make_float2((float)cos(a), (float)sin(a));
	}
	for (uint32_t l = 0; l < nl; l++) {
		const double a = -2.0 * SD_PI * (double)l / (double)rate_in, s = sin(0.5 * a);
		tl[l] = make_float2((float)(-2.0 * s * s), (float)sin(a));
	}
	HIPCHK(t->d_taps.upload(g.data(), total));
	HIPCHK(t->d_tapoff.upload(tapoff.data(), n_sets));
	HIPCHK(t->d_T.upload(T.data(), n_sets));
	HIPCHK(t->d_th.upload(th.data(), nh));
	HIPCHK(t->d_tl.upload(tl.data(), nl));
	HIPCHK(t->d_hist.zeros(t->H));
	return 0;
}

// the object over n_slots idle slots; H from the longest tap set (the narrowest bandwidth)
static int tn_create(uint32_t rate_in, uint32_t rate_out, uint32_t up, uint32_t down, uint32_t n_slots, const std::map<uint32_t, uint32_t> &sets /* bandwidth -> T */,
	size_t max_in, int input_kind, int device, const char *fn, SondeTuner **out)
{
	uint32_t Tmax = 0;
	for (auto &s : sets) Tmax = s.second > Tmax ? s.second : Tmax;
	if (sets.size() > 255) return sd_fail((std::string(fn) + ": more than 255 distinct bandwidths").c_str());
	if (max_in + Tmax >= (1u << 30) || (max_in / down) * up >= (1u << 30))
		return sd_fail((std::string(fn) + ": max_in too large (window indices are 32-bit)").c_str());
	if (sd_select_device(device, fn)) return -1;
	SondeTuner *t = new SondeTuner;
	t->device = device; t->input_kind = input_kind; t->fs = rate_in; t->rate_out = rate_out; t->up = up; t->down = down;
	t->n_vfos = n_slots; t->max_in = max_in; t->H = Tmax - 1;
	if (tn_build(t, sets)) { sonde_tuner_destroy(t); return -1; }       // (destroy leaves the error text alone)
	*out = t;
	return 0;
}

static int tn_check_create(uint32_t rate_in, uint32_t rate_out, size_t max_in, int input_kind, uint32_t *up, uint32_t *down, const char *fn)
{
	if (tn_ratio(rate_in, rate_out, up, down, fn)) return -1;
	if (!sd_input_complex(input_kind))
		return sd_fail((std::string(fn) + ": input_kind must be SONDE_INPUT_IQ, SONDE_INPUT_IQ16 or SONDE_INPUT_IQ8 (the tuner mixes complex samples)").c_str());
	if (max_in < *down) return sd_fail((std::string(fn) + ": max_in must be at least the ratio's denominator").c_str());
	return 0;
}

static void tn_set(SondeTuner *t, uint32_t slot, int32_t offset_hz, uint32_t b)
{
	t->offset[slot] = offset_hz;
	t->theta[slot] = 0;
	t->bw[slot] = b;
	t->set[slot] = (uint8_t)t->set_of[b];
	t->active[slot] = 1;
}

// "all slots active" over the slot structure: the tap sets of the VFOs' bandwidths, every slot set at create
extern "C" int sonde_tuner_create(uint32_t rate_in, uint32_t rate_out, uint32_t n_vfos, const SondeTunerVfo *vfos, size_t max_in, int input_kind,
	int device, SondeTuner **out)
{
	if (!out || !vfos || !n_vfos) return sd_fail("sonde_tuner_create: bad argument");
	uint32_t up, down;
	if (tn_check_create(rate_in, rate_out, max_in, input_kind, &up, &down, "sonde_tuner_create")) return -1;
	std::map<uint32_t, uint32_t> sets;      // bandwidth -> T
	for (uint32_t k = 0; k < n_vfos; k++) {
		const uint32_t b = vfos[k].bandwidth_hz ? vfos[k].bandwidth_hz : rate_out;
		if (b < 5000u || b > rate_out) return sd_fail("sonde_tuner_create: bandwidth_hz must be 5000 .. rate_out (0 = rate_out)");
		if (tn_check_offset(rate_in, b, vfos[k].offset_hz, "sonde_tuner_create")) return -1;
		sets[b] = tn_T(rate_in, b);
	}
	if (tn_create(rate_in, rate_out, up, down, n_vfos, sets, max_in, input_kind, device, "sonde_tuner_create", out)) return -1;
	for (uint32_t k = 0; k < n_vfos; k++) tn_set(*out, k, vfos[k].offset_hz, vfos[k].bandwidth_hz ? vfos[k].bandwidth_hz : rate_out);
	return 0;
}

extern "C" int sonde_tuner_create_slots(uint32_t rate_in, uint32_t rate_out, uint32_t n_slots, const uint32_t *bandwidths, uint32_t n_bandwidths,
	size_t max_in, int input_kind, int device, SondeTuner **out)
{
	if (!out || !n_slots || !bandwidths || !n_bandwidths) return sd_fail("sonde_tuner_create_slots: bad argument");
	uint32_t up, down;
	if (tn_check_create(rate_in, rate_out, max_in, input_kind, &up, &down, "sonde_tuner_create_slots")) return -1;
	std::map<uint32_t, uint32_t> sets;
	for (uint32_t i = 0; i < n_bandwidths; i++) {
		const uint32_t b = bandwidths[i] ? bandwidths[i] : rate_out;
		if (b < 5000u || b > rate_out) return sd_fail("sonde_tuner_create_slots: a bandwidth must be 5000 .. rate_out (0 = rate_out)");
		sets[b] = tn_T(rate_in, b);
	}
	return tn_create(rate_in, rate_out, up, down, n_slots, sets, max_in, input_kind, device, "sonde_tuner_create_slots", out);
}

extern "C" int sonde_tuner_slot_set(SondeTuner *t, uint32_t slot, int32_t offset_hz, uint32_t bandwidth_hz)
{
	if (!t) return sd_fail("sonde_tuner_slot_set: null argument");
	if (slot >= t->n_vfos) return sd_fail("sonde_tuner_slot_set: no such slot");
	const uint32_t b = bandwidth_hz ? bandwidth_hz : t->rate_out;
	if (!t->set_of.count(b)) return sd_fail("sonde_tuner_slot_set: bandwidth_hz is not one of the bandwidths listed at create");
	if (tn_check_offset(t->fs, b, offset_hz, "sonde_tuner_slot_set")) return -1;
	tn_set(t, slot, offset_hz, b);
	return 0;
}

extern "C" int sonde_tuner_slot_clear(SondeTuner *t, uint32_t slot)
{
	if (!t) return sd_fail("sonde_tuner_slot_clear: null argument");
	if (slot >= t->n_vfos) return sd_fail("sonde_tuner_slot_clear: no such slot");
	t->active[slot] = 0;
	return 0;
}

extern "C" int sonde_tuner_slot_active(const SondeTuner *t, uint32_t slot)
{
	if (!t) return sd_fail("sonde_tuner_slot_active: null argument");
	if (slot >= t->n_vfos) return sd_fail("sonde_tuner_slot_active: no such slot");
	return t->active[slot];
}

extern "C" size_t sonde_tuner_out_samples(const SondeTuner *t, size_t n_in) { return t ? n_in / t->down * t->up : 0; }

extern "C" int sonde_tuner_retune(SondeTuner *t, uint32_t vfo, int32_t offset_hz)
{
	if (!t) return sd_fail("sonde_tuner_retune: null argument");
	if (vfo >= t->n_vfos) return sd_fail("sonde_tuner_retune: no such VFO");
	if (!t->active[vfo]) return sd_fail("sonde_tuner_retune: the slot is idle (sonde_tuner_slot_set tunes it)");
	if (tn_check_offset(t->fs, t->bw[vfo], offset_hz, "sonde_tuner_retune")) return -1;
	t->offset[vfo] = offset_hz;
	t->theta[vfo] = 0;
	t->started = true;
	return 0;
}

static uint32_t tn_mod(int64_t f, uint32_t fs) { return (uint32_t)(((f % (int64_t)fs) + (int64_t)fs) % (int64_t)fs); }

// SPEC 3.9 "Continuous retune": theta' = (theta + (f_old - f_new) (n0 - T_k / 2)) mod Fs for the next submit's first index n0: the mixer's
// phase is what the old offset would have given at the sample the filter's group delay (T_k / 2 - 1 / (2 up) samples) puts under the
// submit's first output, so that the ROW's phase runs on across the boundary
extern "C" int sonde_tuner_retune_continuous(SondeTuner *t, uint32_t vfo, int32_t offset_hz)
{
	if (!t) return sd_fail("sonde_tuner_retune_continuous: null argument");
	if (vfo >= t->n_vfos) return sd_fail("sonde_tuner_retune_continuous: no such VFO");
	if (!t->active[vfo]) return sd_fail("sonde_tuner_retune_continuous: the slot is idle (sonde_tuner_slot_set tunes it)");
	if (tn_check_offset(t->fs, t->bw[vfo], offset_hz, "sonde_tuner_retune_continuous")) return -1;
	const uint64_t df = tn_mod((int64_t)t->offset[vfo] - (int64_t)offset_hz, t->fs);
	const uint64_t n0 = tn_mod(t->n_base - (int64_t)(tn_T(t->fs, t->bw[vfo]) / 2), t->fs);
	t->theta[vfo] = (uint32_t)((t->theta[vfo] + df * n0 % t->fs) % t->fs);
	t->offset[vfo] = offset_hz;
	t->started = true;
	return 0;
}

// test introspection (DESIGN "Stream age"): the absolute input index of the first sample the tuner will see.  Its history is zeros, so
// the tuner is one that was "tuned since create, with silence until n_base".  Only before the first process and the first retune.
extern "C" int sonde_tuner_test_set_base(SondeTuner *t, int64_t n_base)
{
	if (!t) return sd_fail("sonde_tuner_test_set_base: null argument");
	if (t->started) return sd_fail("sonde_tuner_test_set_base: the tuner has processed or been retuned already");
	if (n_base < 0 || n_base > ((int64_t)1 << 62) || n_base % (int64_t)t->down)
		return sd_fail("sonde_tuner_test_set_base: n_base must be 0 .. 2^62 and a multiple of the ratio's denominator");
	t->n_base = n_base;
	return 0;
}

extern "C" int sonde_tuner_process(SondeTuner *t, const void *wide_dev, size_t n_in, void *out_dev, size_t out_stride, void *stream)
{
	if (!t || !wide_dev || !out_dev) return sd_fail("sonde_tuner_process: null argument");
	if (!n_in || n_in > t->max_in || n_in % t->down) return sd_fail("sonde_tuner_process: n_in must be a multiple of the ratio's denominator and <= max_in");
	const size_t n_out = sonde_tuner_out_samples(t, n_in);
	if (out_stride < n_out) return sd_fail("sonde_tuner_process: out_stride shorter than the row");
	if ((uintptr_t)wide_dev % sd_sample_bytes(t->input_kind)) return sd_fail("sonde_tuner_process: the block is not aligned to the sample size");
	if ((uintptr_t)out_dev & 7u) return sd_fail("sonde_tuner_process: out must be 8-byte aligned");
	HIPCHK(hipSetDevice(t->device));
	hipStream_t s = (hipStream_t)stream;
	const float2 *h_in = t->d_hist.in();
	float2 *h_out = t->d_hist.out();
	sd_input_dispatch(t->input_kind, [&](auto kk) {
		constexpr int K = decltype(kk)::value;
		if constexpr (K != SONDE_INPUT_REAL) {
			const void *x = wide_dev;
			// the active slots, TN_VMAX per launch, in ascending slot order
			SdTunerOffs o = {};
			uint32_t nv = 0;
			for (uint32_t k = 0; k <= t->n_vfos; k++) {
				if (k < t->n_vfos && t->active[k]) {
					o.F[nv] = tn_mod((int64_t)t->offset[k], t->fs);
					o.TH[nv] = t->theta[k];
					o.SLOT[nv] = k;
					o.SET[nv] = t->set[k];
					nv++;
				}
				if (nv == TN_VMAX || (k == t->n_vfos && nv)) {
					const dim3 grid((unsigned)((n_out + TN_JT - 1) / TN_JT), nv);
					hipLaunchKernelGGL(sd_tuner_kernel<K>, grid, dim3(TN_WG), 0, s, x, h_in, t->H, (uint32_t)n_out, t->n_base, t->up, t->down, t->fs,
						t->d_taps, t->d_tapoff, t->d_T, t->d_th, t->d_tl, o, (float2 *)out_dev, out_stride);
					nv = 0;
				}
			}
			// the idle slots' rows: zeros
			SdTunerIdle z = {};
			uint32_t nz = 0;
			for (uint32_t k = 0; k <= t->n_vfos; k++) {
				if (k < t->n_vfos && !t->active[k]) z.SLOT[nz++] = k;
				if (nz == TN_VMAX || (k == t->n_vfos && nz)) {
					const dim3 grid((unsigned)((n_out + TN_WG - 1) / TN_WG), nz);
					hipLaunchKernelGGL(sd_tuner_fill_kernel, grid, dim3(TN_WG), 0, s, z, (uint32_t)n_out, (float2 *)out_dev, out_stride);
					nz = 0;
				}
			}
			hipLaunchKernelGGL(sd_tuner_hist_kernel<K>, dim3((t->H + TN_WG - 1) / TN_WG), dim3(TN_WG), 0, s, x, h_in, h_out, t->H, (uint32_t)n_in);
		}
	});
	HIPCHK_IN("sonde_tuner_process", hipGetLastError());
	t->d_hist.flip();
	t->n_base += (int64_t)n_in;
	t->started = true;
	return 0;
}
