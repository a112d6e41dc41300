// batch.hip -- host engine of libsonde_mi355.so: the B0 batch API of include/sonde_abi.h.
//
// Owns the per-channel device state (demod state, ring tail, bit ring, framer state, frame slots),
// launches kernel A (demod_kernel.hip) and kernel B (framer_kernel.hip) back to back on the caller's
// HIP stream, and hands corrected frames back.  There is no CPU fallback: every entry point fails
// with an error if HIP is unavailable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "sonde_dev.h"
#include "sd_input.h"
#include "../../include/sonde_abi.h"

#include "launch.h"
#include "parse.h"
#include "sd_chanlist.h"
#include <deque>
#include <memory>

// Events that only order streams of this device, or time kernels on it, need no system-scope release (a cache write-back
// towards the host): hipEventDisableSystemFence.  ev_done is what the host waits on before it reads frames: it keeps the fence.
#ifndef SD_EV_FLAGS
#define SD_EV_FLAGS hipEventDisableSystemFence
#endif
#define SD_EV_TIMING (SD_EV_FLAGS)
#define SD_EV_ORDER  (hipEventDisableTiming | SD_EV_FLAGS)
static thread_local std::string g_err;
static int fail(const char *what, hipError_t e = hipSuccess)
{
	g_err = what;
	if (e != hipSuccess) { g_err += ": "; g_err += hipGetErrorString(e); }
	return -1;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(#x, e_); } while (0)

extern "C" const char *sonde_last_error(void) { return g_err.c_str(); }
int sd_fail(const char *what, hipError_t e) { return fail(what, e); }     // for the other host objects of the library (vfo.hip)
int sd_fail_msg(const char *what) { return fail(what); }                  // the same for pure-host sources (sd_host.h)
extern "C" const char *sonde_version(void) { return "sonde_mi355 0.1 (gfx950)"; }

// ---------------------------------------------------------------- modem table (SPEC)
// Symbol (chip) rates: SURVEY.md Appendix B; the VFO bandwidths of /root/reference/src/main.hpp:44-52
// bound them from above.
struct ModemDef { double baud; float cutoff; int decim; int pre; };   // pre = 8: AFSK tone demodulator in front (SPEC 3.6)
static const ModemDef k_modems[SONDE_NTYPES] = {
	{ 4800.0, 0.65f, 4, 1 },   // RS41   4800 Bd GFSK NRZ; IQ decimated 4:1 before the discriminator: 12 kS/s (SPEC 3.0)
	{ 5000.0, 0.65f, 4, 1 },   // DFM    2500 bit/s Manchester -> 5000 chips/s; 12 kS/s
	{ 4800.0, 0.65f, 4, 1 },   // iMS100 2400 bit/s biphase    -> 4800 chips/s; 12 kS/s
	{ 9600.0, 0.65f, 2, 1 },   // M10    9600 chips/s Manchester; 2:1: 24 kS/s (2.5 samples per chip)
	{ 1200.0, 0.65f, 1, 8 },   // iMet-1/4 Bell-202 AFSK 1200 Bd: tone demodulator, then 6 kS/s through the same loop
	{ 2400.0, 0.65f, 1, 8 },   // SRS-C50 AFSK 2400 Bd (2900 / 4700 Hz): tone demodulator, then 6 kS/s (2.5 samples per symbol)
	{ 4800.0, 0.65f, 4, 1 },   // MRZ-N1  2400 bit/s Manchester -> 4800 chips/s; 12 kS/s
};
// (every GFSK sonde runs at about 2.5 samples per symbol behind the boxcar: each halving of the pre-detection bandwidth buys
// 2-2.5 dB of sensitivity and halves the discriminator arithmetic, profiles/r3_sensitivity.md; SONDE_FLAG_WIDE: one step less)

static int modem_div(const ModemDef *md, int type) { return md[type].decim * md[type].pre; }     // input samples per internal sample
static int32_t modem_period0(const ModemDef *md, int type) { return (int32_t)llrint(65536.0 * ((double)SD_FS / modem_div(md, type)) / md[type].baud); }
static int modem_nt(const ModemDef *md, int type) { return SD_NT_OF(modem_period0(md, type), md[type].pre); }
// demod-kernel class of a (decimation, taps) pair: the instantiations of sd_demod_kernel
static const int k_cls_decim[4] = { 1, 2, 4, 2 }, k_cls_nt[4] = { 16, 16, 8, 8 };
static int modem_class(const ModemDef *md, int type)
{
	const int d = md[type].decim, nt = modem_nt(md, type);
	for (int k = 0; k < 4; k++) if (k_cls_decim[k] == d && k_cls_nt[k] == nt) return k;
	return -1;
}

static void make_taps(const ModemDef *md, int type, float *out /* [32][32] */)
{
	const double PI = 3.14159265358979323846;
	const double fc = (double)md[type].cutoff * md[type].baud / ((double)SD_FS / modem_div(md, type));
	const int nt = modem_nt(md, type);                 // taps in use
	memset(out, 0, sizeof(float) * SD_NPHASE * SD_NTAPS);
	for (int p = 0; p < SD_NPHASE; p++) {
		double h[SD_NTAPS], sum = 0.0;
		for (int j = 0; j < nt; j++) {
			const double t = (double)j - (double)(nt / 2) + (double)p / (double)SD_NPHASE;
			const double x = (t + (double)(nt / 2)) / (double)nt;
			const double w = 0.42 - 0.5 * cos(2.0 * PI * x) + 0.08 * cos(4.0 * PI * x);
			const double s = (t == 0.0) ? 2.0 * fc : sin(2.0 * PI * fc * t) / (PI * t);
			h[j] = s * w;
			sum += h[j];
		}
		for (int j = 0; j < nt; j++) out[p * SD_NTAPS + j] = (float)(h[j] / sum);
	}
}

// mixer table of the AFSK tone demodulator: (cos, -sin) of 2 pi 17 k / 480 (1700 Hz at 48 kS/s), SPEC 3.6
void make_mixer(float *out, int cycles, int per)
{
	const double PI = 3.14159265358979323846;
	for (int k = 0; k < per; k++) {
		const double a = 2.0 * PI * (double)cycles * (double)k / (double)per;
		out[2 * k] = (float)cos(a);
		out[2 * k + 1] = (float)(-sin(a));
	}
}
extern "C" int sonde_get_afsk_table(float *out /* [480][2] */)
{
	if (!out) return fail("sonde_get_afsk_table: null argument");
	make_mixer(out, 17, SD_AF_PER);         // iMet: 1700 Hz
	return 0;
}

extern "C" int sonde_get_taps(int type, float *out)
{
	if (type < 0 || type >= SONDE_NTYPES || !out) return fail("sonde_get_taps: bad argument");
	make_taps(k_modems, type, out);
	return 0;
}

// ---------------------------------------------------------------- batch object
struct SondeBatch {
	uint32_t n_channels = 0, max_samples = 0;
	int input_kind = 0, device = 0;
	uint32_t ring_words = 0, max_frames = 0;
	uint32_t type_frames[SONDE_NTYPES] = {};   // upper bound of complete frames per submit, per sonde type (B2 grid)
	std::vector<uint8_t> types;
	std::vector<uint32_t> chlist[SONDE_NTYPES];
	ModemDef md[SONDE_NTYPES];             // this batch's modem table (k_modems, with the configuration flags applied)

	SdChanState *d_states = nullptr;
	SdFramerState *d_fstates = nullptr;
	float *d_hist = nullptr;
	uint32_t *d_bitring = nullptr;
	// frame slots, per-channel frame counts and the demod kernel's framer descriptor exist TWICE: submit k writes set k & 1, so
	// the frames of submit k stay readable while submit k + 1 is queued or running (sonde_batch_frames_of)
	SondeFrame *d_frames2[2] = {};
	uint32_t *d_counts2[2] = {};
	hipEvent_t ev_done[2] = {};            // recorded behind the last kernel of each submit once the host works with tickets
	bool ev_valid[2] = { false, false };   // (an event record is a bubble in the command stream: not paid by hosts that sync every submit)
	bool ticketing = false;
	hipEvent_t ev_xs = nullptr;            // orders a submit behind the previous one when the host changes streams
	uint64_t tickets = 0;                  // submits so far; submit number t (1-based) used set (t - 1) & 1
	float *d_taps = nullptr;
	SdModem *d_modems = nullptr;
	uint8_t *d_gfexp = nullptr, *d_gflog = nullptr, *d_g64 = nullptr;
	uint16_t *d_m10tab = nullptr;          // Meteomodem checksum as a GF(2) matrix product: rows A^k B, sd_fixed.h
	uint32_t fuse_fec = 1;                 // RS41 FEC in the demod kernel's epilogue (default) or as its own kernel (SONDE_FLAG_SPLIT_FEC)
	uint32_t fixed_epi = 1;                // the fixed-length framers' frames decoded in the demod kernel's epilogue too (round 6; not behind a channelizer: bins_kernel.hip)
	SdFramerOut *d_fo2[2] = {};            // where the demod kernel's in-kernel sync search keeps its state and lists frames (device copies)
	SdFramerOut h_fo2[2] = {};             // host copies: the bins decoder takes the descriptor by value (bins_kernel.hip)
	SdModem h_modems[SONDE_NTYPES] = {};
	uint32_t *d_gfswar = nullptr;          // byte-slice tables of the 24 syndrome multipliers alpha^(4j), framer_kernel.hip
	void *d_descs = nullptr;
	uint32_t *d_chlist[SONDE_NTYPES] = {};
	void *d_stage = nullptr;
	size_t stage_bytes = 0;
	// AFSK sondes (iMet): tone-demodulator state, mixer table, 6 kS/s scratch rows; the other channels' list for kernel A
	SdAfskState *d_astates = nullptr;
	float *d_wtab = nullptr, *d_wtab_c50 = nullptr, *d_afq = nullptr;
	// kernel A is instantiated per (decimation, taps) class (k_cls_*).  One class in the batch = one plain launch over all
	// channels.  Several (or AFSK channels) = LAUNCH UNITS: every sonde type's channel list is cut into n_chunks pieces, a unit is
	// (type, piece): its demod launch (the type's class) and its frame decoder behind it on the unit's OWN stream, so that the
	// units overlap on the GPU and a unit's submits stay ordered from submit to submit.  Units are launched piece by piece,
	// inside a piece the type with the longest-running workgroups first (M10: twice the symbols per tile; then RS41, whose
	// workgroups end with the FEC epilogue): with n_chunks > 1 every compute unit holds a mix of heavy (M10: VALU / LDS bound)
	// and light (HBM bound) workgroups at any time instead of a generation of M10 followed by generations of the others.
	uint32_t n_cls[4] = {};
	int cls_type[4] = { -1, -1, -1, -1 };  // the sonde type of a class whose channels are all of one type, else -1 (sd_launch_demod's utype)
	int n_classes = 0, only_class = 0;
	// Joined batches (the default: every submit ends in the caller's stream) launch per CLASS instead (type = -1: the types
	// of a class share one launch over the class's channel list, their frame decoders follow): measured 0.319 ms per step
	// against 0.336 per type for 4096 RS41 / M10 / DFM channels x 24 tiles; pipelined (SONDE_FLAG_PIPELINE) it is the other way
	// round, 0.321 per class against 0.289 per type, and more pieces than one only add launches (profiles/r3_notes.md).
	struct Unit { int type, cls; uint32_t off, n; size_t row0; hipStream_t st; hipEvent_t ev_join[2]; };      // ev_join[submit parity]
	std::vector<Unit> units;
	uint32_t *d_cls[4] = {};               // joined batches: the channel list of each class
	int n_chunks = 1;
	hipEvent_t ev_fork = nullptr;
	// How a submit of several launch units completes (include/sonde_abi.h): 0 (default): the unit streams are joined into the
	// caller's stream before sonde_batch_submit returns; 1 SONDE_FLAG_LATE_JOIN: one submit late -- submit t joins the units of submit
	// t - 1 into the caller's stream, so that a unit's submit t + 1 may start beside the other units' submit t; 2 SONDE_FLAG_PIPELINE:
	// never.  In modes 1 and 2 done_stream collects the unit streams for completion (sonde_batch_sync, tickets).
	int join_mode = 0;
	bool pipeline = false;                 // join_mode != 0
	hipStream_t done_stream = nullptr;
	uint32_t granule = SONDE_TILE;         // submit sizes must be a multiple of this
	// time slices (launch.h SdSlice): per-channel segment counters, the value they hold before the next sliced launch, the residency
	// the policy works with (demod workgroups the GPU holds at once) and the knob (SondeBatchConfig.time_slices; 0: the library's choice)
	uint32_t *d_prog = nullptr;
	uint32_t seg_base = 0;
	uint32_t residency = 1024;
	int seg_force = 0;
	bool sliced_once = false;
	// round 6: a batch of exactly the two default classes -- (4, 8): RS41 / DFM / iMS-100 / MRZ-N1 and (2, 8): M10; BASELINE config 3 --
	// at the default completion mode is ONE launch on the caller's stream (sd_demod_mixed_kernel: the classes interleaved block by
	// block), frame decoders in its epilogue: no fork, no join, no launch units
	bool mixed_one = false;

	static const int kEvSlots = 128;       // submits timed between two sonde_batch_kernel_ms() calls
	hipEvent_t ev[3 * kEvSlots] = {};
	int ev_used = 0;
	// mixed batches: the same for each class's demod kernel alone, on its class stream (sonde_batch_class_ms)
	hipEvent_t *evc = nullptr;             // [kEvSlots][units][2]
	int evc_used = 0;
	// an event record is a bubble of a few microseconds in the command stream (three of them cost a 0.29 ms step 3 %), so
	// only every timing_every-th submit is timed (0: none)
	int timing_every = 8;
	unsigned long n_submits = 0;
	bool ev_has_framer[kEvSlots] = {};
	hipStream_t last_stream = nullptr;
	bool pending = false;
	bool have_counts2[2] = { false, false };
	std::vector<uint32_t> h_counts2[2];
	long n_frames2[2] = { 0, 0 }, n_overflow2[2] = { 0, 0 };
	std::vector<SondeFrame> h_slots;
	// sonde_batch_poll: per-channel parsers (created on first use), fragments waiting to be fetched
	std::vector<std::unique_ptr<SondeParser>> parsers;
	std::deque<std::pair<uint32_t, SondeData>> frags;
	uint64_t polled_ticket = 0;            // submits up to this one have been parsed by sonde_batch_poll
	// sonde_batch_restart_channels (SPEC 3.12): the channel lists on their way to the reset kernel, the event that orders the next
	// submit's launch units behind it, and (submits so far, channel): the channel's parser is replaced before a later submit is parsed
	SdChanLists restart_lists;
	hipEvent_t ev_restart = nullptr;
	std::deque<std::pair<uint64_t, uint32_t>> parser_restarts;
	bool behind_channelizer = false;
	// SONDE_FLAG_RS41_RESCUE (SPEC 3.3c): per-channel layouts and counters of the second pass (rescue_kernel.hip); null: the flag is
	// off or the batch has no RS41 channel, and nothing of it is allocated or launched
	SdRescueState *d_rescue = nullptr;
};

static uint32_t pow2ceil(uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

extern "C" void sonde_batch_destroy(SondeBatch *b)
{
	if (!b) return;
	(void)hipSetDevice(b->device);
	if (b->pending) (void)hipStreamSynchronize(b->last_stream);
	(void)hipFree(b->d_states); (void)hipFree(b->d_fstates); (void)hipFree(b->d_hist); (void)hipFree(b->d_bitring);
	for (int k = 0; k < 2; k++) { (void)hipFree(b->d_frames2[k]); (void)hipFree(b->d_counts2[k]); (void)hipFree(b->d_fo2[k]); if (b->ev_done[k]) (void)hipEventDestroy(b->ev_done[k]); }
	if (b->ev_xs) (void)hipEventDestroy(b->ev_xs);
	if (b->ev_restart) (void)hipEventDestroy(b->ev_restart);
	b->restart_lists.destroy();
	(void)hipFree(b->d_taps); (void)hipFree(b->d_modems); (void)hipFree(b->d_prog); (void)hipFree(b->d_rescue);
	(void)hipFree(b->d_astates); (void)hipFree(b->d_wtab); (void)hipFree(b->d_wtab_c50); (void)hipFree(b->d_afq);
	for (auto &u : b->units) { if (u.st) (void)hipStreamDestroy(u.st); for (int k = 0; k < 2; k++) if (u.ev_join[k]) (void)hipEventDestroy(u.ev_join[k]); }
	for (int k = 0; k < 4; k++) (void)hipFree(b->d_cls[k]);
	if (b->done_stream) (void)hipStreamDestroy(b->done_stream);
	if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
	(void)hipFree(b->d_gfexp); (void)hipFree(b->d_gflog); (void)hipFree(b->d_gfswar); (void)hipFree(b->d_g64); (void)hipFree(b->d_m10tab); (void)hipFree(b->d_descs); (void)hipFree(b->d_stage);
	for (int t = 0; t < SONDE_NTYPES; t++) (void)hipFree(b->d_chlist[t]);
	for (int i = 0; i < 3 * SondeBatch::kEvSlots; i++) if (b->ev[i]) (void)hipEventDestroy(b->ev[i]);
	if (b->evc) { for (size_t i = 0; i < 2 * b->units.size() * SondeBatch::kEvSlots; i++) if (b->evc[i]) (void)hipEventDestroy(b->evc[i]); delete[] b->evc; }
	delete b;
}

extern "C" int sonde_batch_create(const SondeBatchConfig *cfg, SondeBatch **out)
{
	if (!cfg || !out) return fail("sonde_batch_create: null argument");
	*out = nullptr;
	//  a caller compiled against an older, shorter SondeBatchConfig, or one that did not zero the struct, must not hand
	// over garbage in the members it does not know about: the size it was compiled with is part of the struct
	if (cfg->struct_size != sizeof(SondeBatchConfig))
		return fail("sonde_batch_create: SondeBatchConfig.struct_size != sizeof(SondeBatchConfig) -- initialise with SONDE_BATCH_CONFIG_INIT (a host built against an older sonde_abi.h must be recompiled)");
	if (cfg->launch_units > 16) return fail("sonde_batch_create: launch_units must be 0 (the library's choice) or 1..16");
	if (cfg->time_slices > 16) return fail("sonde_batch_create: time_slices must be 0 (the library's choice) or 1..16");
	if (cfg->n_channels == 0) return fail("sonde_batch_create: n_channels == 0");
	if (cfg->max_samples == 0 || cfg->max_samples % SONDE_TILE) return fail("sonde_batch_create: max_samples must be a positive multiple of SONDE_TILE");
	if (!sd_input_known(cfg->input_kind)) return fail("sonde_batch_create: bad input_kind");
	int ndev = 0;
	HIPCHK(hipGetDeviceCount(&ndev));
	if (cfg->device < 0 || cfg->device >= ndev) return fail("sonde_batch_create: no such HIP device");
	HIPCHK(hipSetDevice(cfg->device));

	SondeBatch *b = new SondeBatch;
	b->n_channels = cfg->n_channels;
	b->max_samples = cfg->max_samples;
	b->input_kind = cfg->input_kind;
	b->device = cfg->device;
	for (int t = 0; t < SONDE_NTYPES; t++) b->md[t] = k_modems[t];
	if ((cfg->flags & (SONDE_FLAG_WIDE | SONDE_FLAG_WIDE_AUTO)) && cfg->input_kind != SONDE_INPUT_REAL)
		for (int t = 0; t < SONDE_NTYPES; t++) {
			// SONDE_FLAG_WIDE: every GFSK sonde; SONDE_FLAG_WIDE_AUTO: the types whose channel is 20 kHz or wider in the reference
			// (iMS-100 / RS-11G, MRZ-N1: 20 kHz, M10 / M20: 50 kHz, /root/reference/src/main.hpp:47-51) -- per type, for mixed batches
			const bool wide_type = (cfg->flags & SONDE_FLAG_WIDE) || t == SONDE_IMS100 || t == SONDE_MRZN1 || t == SONDE_M10;
			if (b->md[t].pre == 1 && wide_type) b->md[t].decim /= 2;       // one decimation step less (SPEC 3.0)
		}
	const ModemDef *md = b->md;
	b->types.assign(cfg->n_channels, SONDE_RS41);
	if (cfg->types) b->types.assign(cfg->types, cfg->types + cfg->n_channels);
	uint64_t max_bits = 0;
	for (uint32_t c = 0; c < b->n_channels; c++) {
		const int t = b->types[c];
		if (t < 0 || t >= SONDE_NTYPES) { delete b; return fail("sonde_batch_create: bad sonde type"); }
		b->chlist[t].push_back(c);
		const int32_t p = modem_period0(md, t) - (modem_period0(md, t) >> 8);      // fastest symbol clock the loop allows
		max_bits = std::max(max_bits, ((uint64_t)(cfg->max_samples / modem_div(md, t)) << 16) / (uint64_t)p + 2);
	}
	b->ring_words = pow2ceil((uint32_t)((max_bits + 8 * SONDE_FRAME_MAX + 1024 + 31) / 32));
	b->max_frames = 2;
	{	// frames per submit per type: submit bits (at that type's fastest period) / shortest frame of the type, + carry-over
		static const uint32_t min_frame_bits[SONDE_NTYPES] = { 320 * 8, 560, 1152, 1648, 140, 90, 768 };
		for (int t = 0; t < SONDE_NTYPES; t++) {
			if (b->chlist[t].empty()) continue;
			const int32_t p = modem_period0(md, t) - (modem_period0(md, t) >> 8);
			const uint64_t bits_t = ((uint64_t)(cfg->max_samples / modem_div(md, t)) << 16) / (uint64_t)p + 2;
			b->type_frames[t] = (uint32_t)(bits_t / min_frame_bits[t]) + 2;
			b->max_frames = std::max(b->max_frames, b->type_frames[t]);
		}
	}
	// the fixed-length framers stage the whole ring in LDS next to a few static words: keep it below the 64 KB workgroup limit
	if ((size_t)b->ring_words * 4 >= 65536) { delete b; return fail("sonde_batch_create: max_samples too large for the LDS-staged bit ring (< 64 KB)"); }

	const size_t C = b->n_channels;
#define ALLOC(p, bytes) do { hipError_t e_ = hipMalloc((void **)&(p), (bytes)); if (e_ != hipSuccess) { sonde_batch_destroy(b); return fail("hipMalloc " #p, e_); } } while (0)
	ALLOC(b->d_states, C * sizeof(SdChanState));
	ALLOC(b->d_fstates, C * sizeof(SdFramerState));
	ALLOC(b->d_hist, C * SD_HIST * sizeof(float));
	ALLOC(b->d_bitring, C * (size_t)b->ring_words * sizeof(uint32_t));
	for (int k = 0; k < 2; k++) {
		ALLOC(b->d_frames2[k], C * (size_t)b->max_frames * sizeof(SondeFrame));
		ALLOC(b->d_counts2[k], C * sizeof(uint32_t));
		ALLOC(b->d_fo2[k], sizeof(SdFramerOut));
	}
	ALLOC(b->d_taps, (size_t)SONDE_NTYPES * SD_NPHASE * SD_NTAPS * sizeof(float));
	ALLOC(b->d_modems, SONDE_NTYPES * sizeof(SdModem));
	ALLOC(b->d_prog, (C + 1) * sizeof(uint32_t));
	ALLOC(b->d_gfexp, 2304);      // zero-absorbing antilog table of the RS decoder (GF_EXP2 in framer_kernel.hip)
	ALLOC(b->d_gflog, 512);       // 256 x u16 logarithms, log 0 = 768
	ALLOC(b->d_gfswar, 24 * 8 * sizeof(uint32_t));
	ALLOC(b->d_g64, 192);
	ALLOC(b->d_m10tab, 99 * 8 * sizeof(uint16_t));
	ALLOC(b->d_descs, C * (size_t)b->max_frames * SD_DESC_BYTES);
	for (int t = 0; t < SONDE_NTYPES; t++)
		if (!b->chlist[t].empty()) ALLOC(b->d_chlist[t], b->chlist[t].size() * sizeof(uint32_t));
	const size_t n_afsk = b->chlist[SONDE_IMET4].size() + b->chlist[SONDE_C50].size();      // tone-demodulated sondes
	std::vector<uint32_t> cls[4];               // index: demod-kernel class (k_cls_decim, k_cls_nt)
	for (uint32_t c = 0; c < b->n_channels; c++) {
		if (b->types[c] == SONDE_IMET4 || b->types[c] == SONDE_C50) continue;
		const int k = modem_class(md, b->types[c]);
		if (k < 0) { sonde_batch_destroy(b); return fail("sonde_batch_create: no demodulator class for this sonde type"); }
		cls[k].push_back(c);
	}
	for (int k = 0; k < 4; k++) {
		b->n_cls[k] = (uint32_t)cls[k].size();
		if (b->n_cls[k]) { b->n_classes++; b->only_class = k; }
		for (uint32_t c : cls[k]) {
			if (c == cls[k][0]) b->cls_type[k] = b->types[c];
			else if (b->types[c] != b->cls_type[k]) { b->cls_type[k] = -1; break; }
		}
	}
	// Round 4: a ONE-class batch that is not joined at every submit (join_mode != 0) is cut into TWO launch units (halves of the channel list, each
	// with its own stream from submit to submit).  A workgroup lives for its channel's whole submit, so a launch whose
	// workgroup count is not a multiple of one residency (4 x 256 CUs) ends with a part-filled generation running alone; with
	// two units in flight the tail of one unit's submit t overlaps the other unit's submit t + 1.  Measured
	// (profiles/r4_notes.md): 1250 channels x 24 tiles 0.556 -> 0.743 of the HBM peak, 1280 x 96 0.634 -> 0.799, 1100 x 96
	// 0.565 -> 0.756, 8192 x 24 0.765 -> 0.782, 1024 x 96 (exactly one residency) 0.779 -> 0.789; three units: equal or worse
	// (1250 x 24: 0.626); four and more: 0.38-0.63 (more streams than the hardware runs side by side).  SondeBatchConfig.launch_units
	// overrides.  Round 5: also the DEFAULT (join_mode 1), with the caller's stream joined one submit late.
	// Round 6: ordinary stream semantics are the default again (join_mode 0); the lagging join is SONDE_FLAG_LATE_JOIN
	b->join_mode = (cfg->flags & SONDE_FLAG_PIPELINE) ? 2 : ((cfg->flags & SONDE_FLAG_LATE_JOIN) ? 1 : 0);
	int one_class_units = 1;
	if (b->join_mode != 0 && n_afsk == 0 && b->n_classes == 1) {
		int n_types = 0;
		for (int t = 0; t < SONDE_NTYPES; t++) n_types += !b->chlist[t].empty();
		// two units where a single launch would end with a part-filled generation of workgroups (one residency = 4 workgroups per CU);
		// a channel count that fills whole residencies stays ONE plain launch on the caller's stream (two units measured +1-2 % there:
		// not worth the lagging join; the headline shape, 1024 channels, and BASELINE config 5's shard, 8192, are such counts)
		hipDeviceProp_t prop0;
		const uint32_t residency = hipGetDeviceProperties(&prop0, cfg->device) == hipSuccess ? 4u * (uint32_t)prop0.multiProcessorCount : 1024u;
		one_class_units = (n_types == 1 && b->n_channels >= 512 && b->n_channels % residency != 0) ? 2 : 1;
		if (cfg->launch_units) one_class_units = std::max(1, std::min(16, (int)cfg->launch_units));      // (experiments: profiles/r4_units_sweep.txt)
	}
	const bool need_lists = n_afsk != 0 || b->n_classes > 1 || one_class_units > 1;
	if (n_afsk) {
		if (cfg->max_samples % (SONDE_TILE * SD_AF_DEC)) { sonde_batch_destroy(b); return fail("sonde_batch_create: with iMet channels max_samples must be a multiple of 16384"); }
		b->granule = SONDE_TILE * SD_AF_DEC;
		ALLOC(b->d_astates, C * sizeof(SdAfskState));
		ALLOC(b->d_wtab, SD_AF_PER * 2 * sizeof(float));
		ALLOC(b->d_wtab_c50, SD_C50_PER * 2 * sizeof(float));
		ALLOC(b->d_afq, n_afsk * (size_t)(cfg->max_samples / SD_AF_DEC) * sizeof(float));
	}
	if ((cfg->flags & SONDE_FLAG_RS41_RESCUE) && !b->chlist[SONDE_RS41].empty()) ALLOC(b->d_rescue, C * sizeof(SdRescueState));
#undef ALLOC
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { sonde_batch_destroy(b); return fail(#x, e_); } } while (0)
	// modem tables
	std::vector<float> taps((size_t)SONDE_NTYPES * SD_NPHASE * SD_NTAPS);
	SdModem modems[SONDE_NTYPES];
	for (int t = 0; t < SONDE_NTYPES; t++) {
		make_taps(md, t, &taps[(size_t)t * SD_NPHASE * SD_NTAPS]);
		const int32_t p0 = modem_period0(md, t);
		modems[t].period0 = p0;
		modems[t].kp = (float)p0 * 0.159154943f;       // half of 1/pi symbol per unit error
		modems[t].ki = modems[t].kp * (1.0f / 4096.0f);
		modems[t].pmin = p0 - (p0 >> 8);
		modems[t].pmax = p0 + (p0 >> 8);
		modems[t].decim = md[t].decim;
		modems[t].itile = SD_TILE / md[t].decim;      // AFSK: kernel A sees the 6 kS/s stream as plain real input
		modems[t].nt = modem_nt(md, t);
		const int rmax = SD_ROUND_MAX * SD_ROUND_SPL(modems[t].decim, modems[t].nt);
		modems[t].rounds = (int32_t)(((((int64_t)modems[t].itile << 16) / modems[t].pmin) + 2 + rmax - 1) / rmax);   // 1; 2: C50
	}
	CHK(hipMemcpy(b->d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
	CHK(hipMemcpy(b->d_modems, modems, sizeof(modems), hipMemcpyHostToDevice));
	memcpy(b->h_modems, modems, sizeof(modems));
	// GF(2^8) tables, primitive polynomial 0x11D
	uint8_t gexp[512], glog[256];
	{
		int x = 1;
		memset(glog, 0, sizeof(glog));
		for (int i = 0; i < 255; i++) { gexp[i] = (uint8_t)x; glog[x] = (uint8_t)i; x <<= 1; if (x & 0x100) x ^= 0x11D; }
		for (int i = 255; i < 512; i++) gexp[i] = gexp[i - 255];
	}
	{	// log domain without zero tests: log 0 = 768 (above any sum of valid logs), antilog periodic below 768, zero above
		std::vector<uint8_t> e2(2304, 0);
		for (int i = 0; i < 768; i++) e2[i] = gexp[i % 255];
		uint16_t l2[256];
		for (int v = 0; v < 256; v++) l2[v] = v ? (uint16_t)glog[v] : (uint16_t)768;
		CHK(hipMemcpy(b->d_gfexp, e2.data(), e2.size(), hipMemcpyHostToDevice));
		CHK(hipMemcpy(b->d_gflog, l2, sizeof(l2), hipMemcpyHostToDevice));
	}
	{	// byte-slice tables of the multipliers c_j = alpha^(4j), j = 0..23 (framer_kernel.hip gf_swar_mul):
		// words 0,1: c*x for x = 0..7;  words 2,3: c*(x << 3);  word 4: c*(x << 6), x = 0..3;  words 5..7 unused
		uint32_t sw[24 * 8];
		memset(sw, 0, sizeof(sw));
		auto mul = [&](int c, int v) -> uint32_t { return (c && v) ? gexp[glog[c] + glog[v]] : 0u; };
		for (int j = 0; j < 24; j++) {
			const int c = gexp[(4 * j) % 255];
			for (int x = 0; x < 8; x++) {
				sw[8 * j + 0 + x / 4] |= mul(c, x) << (8 * (x % 4));
				sw[8 * j + 2 + x / 4] |= mul(c, x << 3) << (8 * (x % 4));
				if (x < 4) sw[8 * j + 4] |= mul(c, x << 6) << (8 * x);
			}
		}
		CHK(hipMemcpy(b->d_gfswar, sw, sizeof(sw), hipMemcpyHostToDevice));
	}
	{	// GF(2^6)/x^6+x+1 tables for BCH(63,51): exp[128] then log[64]
		uint8_t g64[192];
		memset(g64, 0, sizeof(g64));
		int x = 1;
		for (int i = 0; i < 63; i++) { g64[i] = (uint8_t)x; g64[128 + x] = (uint8_t)i; x <<= 1; if (x & 0x40) x ^= 0x43; }
		for (int i = 63; i < 128; i++) g64[i] = g64[i - 63];
		CHK(hipMemcpy(b->d_g64, g64, sizeof(g64), hipMemcpyHostToDevice));
	}
	{	// M10 checksum: c' = f(c, b) is GF(2)-linear, c' = A c + B b; row k holds A^k B e_j for the eight unit bytes e_j
		auto step = [](unsigned c, unsigned bb) {
			const unsigned c1 = c & 0xFF;
			bb = ((bb >> 1) | ((bb & 1) << 7)) & 0xFF;
			bb ^= (bb >> 2) & 0xFF;
			const unsigned t6 = (c & 1) ^ ((c >> 2) & 1) ^ ((c >> 4) & 1);
			const unsigned t7 = ((c >> 1) & 1) ^ ((c >> 3) & 1) ^ ((c >> 5) & 1);
			const unsigned t = (c & 0x3F) | (t6 << 6) | (t7 << 7);
			unsigned sft = (c >> 7) & 0xFF;
			sft ^= (sft >> 2) & 0xFF;
			return ((c1 << 8) | (bb ^ t ^ sft)) & 0xFFFFu;
		};
		uint16_t tab[99 * 8];
		for (int j = 0; j < 8; j++) {
			unsigned c = step(0, 1u << j);
			for (int k = 0; k < 99; k++) { tab[8 * k + j] = (uint16_t)c; c = step(c, 0); }
		}
		CHK(hipMemcpy(b->d_m10tab, tab, sizeof(tab), hipMemcpyHostToDevice));
	}
	{
		b->fuse_fec = (cfg->flags & SONDE_FLAG_SPLIT_FEC) ? 0u : 1u;
		for (int k = 0; k < 2; k++) {
			// one residency of the GPU: 4 demod workgroups (39.7 KB of LDS, 8 waves each) per CU
			hipDeviceProp_t prop;
			CHK(hipGetDeviceProperties(&prop, cfg->device));
			const uint32_t loop_wg = 4u * (uint32_t)prop.multiProcessorCount;
			if (!b->fuse_fec) b->fixed_epi = 0;
			const SdFramerOut fo = { b->d_fstates, b->d_descs, b->d_counts2[k], b->max_frames, b->fuse_fec, loop_wg, b->d_gfexp, b->d_gflog, b->d_gfswar, b->d_g64, b->d_frames2[k],
			                         b->d_m10tab, b->fixed_epi };
			CHK(hipMemcpy(b->d_fo2[k], &fo, sizeof(fo), hipMemcpyHostToDevice));
			b->h_fo2[k] = fo;
			CHK(hipEventCreateWithFlags(&b->ev_done[k], hipEventDisableTiming));
		}
		CHK(hipEventCreateWithFlags(&b->ev_xs, SD_EV_ORDER));
		CHK(hipEventCreateWithFlags(&b->ev_restart, SD_EV_ORDER));
	}
	// initial channel state
	std::vector<SdChanState> st(C);
	for (size_t c = 0; c < C; c++) {
		memset(&st[c], 0, sizeof(SdChanState));
		const int t = b->types[c];
		st[c].type = t;
		st[c].period = modems[t].period0;
		st[c].t_next = ((int64_t)SD_NTAPS << 16) + modems[t].period0;
		st[c].amp = 0.25f;
	}
	CHK(hipMemcpy(b->d_states, st.data(), C * sizeof(SdChanState), hipMemcpyHostToDevice));
	CHK(hipMemset(b->d_fstates, 0, C * sizeof(SdFramerState)));
	CHK(hipMemset(b->d_prog, 0, (C + 1) * sizeof(uint32_t)));
	if (b->d_rescue) CHK(hipMemset(b->d_rescue, 0, C * sizeof(SdRescueState)));       // no layout, counters zero
	{
		hipDeviceProp_t pr;
		if (hipGetDeviceProperties(&pr, cfg->device) == hipSuccess && pr.multiProcessorCount > 0) b->residency = 4u * (uint32_t)pr.multiProcessorCount;
		b->seg_force = (int)cfg->time_slices;
	}
	CHK(hipMemset(b->d_hist, 0, C * SD_HIST * sizeof(float)));
	CHK(hipMemset(b->d_bitring, 0, C * (size_t)b->ring_words * sizeof(uint32_t)));
	for (int k = 0; k < 2; k++) CHK(hipMemset(b->d_counts2[k], 0, C * sizeof(uint32_t)));
	if (n_afsk) {
		float wtab[2 * SD_AF_PER];
		sonde_get_afsk_table(wtab);
		CHK(hipMemcpy(b->d_wtab, wtab, sizeof(wtab), hipMemcpyHostToDevice));
		float wc[2 * SD_C50_PER];
		make_mixer(wc, 19, SD_C50_PER);       // C50: 3800 Hz, midway between the 2900 / 4700 Hz tones
		CHK(hipMemcpy(b->d_wtab_c50, wc, sizeof(wc), hipMemcpyHostToDevice));
		CHK(hipMemset(b->d_astates, 0, C * sizeof(SdAfskState)));
	}
	for (int t = 0; t < SONDE_NTYPES; t++)
		if (!b->chlist[t].empty())
			CHK(hipMemcpy(b->d_chlist[t], b->chlist[t].data(), b->chlist[t].size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	for (int i = 0; i < 3 * SondeBatch::kEvSlots; i++) CHK(hipEventCreateWithFlags(&b->ev[i], SD_EV_TIMING));
	if (need_lists) {
		CHK(hipEventCreateWithFlags(&b->ev_fork, SD_EV_ORDER));
		const bool pipelined = b->join_mode != 0;
		// pieces per type: one (2-8 pieces of every type of a mixed batch measured 6-70 % slower, profiles/r3_notes.md); a one-type batch: two
		int R = 1;
		if (one_class_units > 1) R = one_class_units;
		b->n_chunks = pipelined ? R : 1;
		static const int order[] = { SONDE_M10, SONDE_RS41, SONDE_DFM09, SONDE_IMS100, SONDE_MRZN1 };
		if (pipelined) {
			for (int j = 0; j < R; j++)
				for (int t : order) {
					const size_t nt = b->chlist[t].size();
					const size_t lo = nt * (size_t)j / (size_t)R, hi = nt * (size_t)(j + 1) / (size_t)R;
					if (hi > lo) b->units.push_back({ t, modem_class(md, t), (uint32_t)lo, (uint32_t)(hi - lo), 0, nullptr, { nullptr, nullptr } });
				}
		} else {
			// class order: the class with the longest-running workgroups (M10: twice the symbols per tile) first, then the 4:1
			// class (whose RS41 workgroups end with the FEC epilogue): best of all orders in round 2 (profiles/r2_notes.md)
			for (int k : { 3, 0, 2, 1 }) {
				if (!b->n_cls[k]) continue;
				hipError_t e_ = hipMalloc((void **)&b->d_cls[k], cls[k].size() * sizeof(uint32_t));
				if (e_ == hipSuccess) e_ = hipMemcpy(b->d_cls[k], cls[k].data(), cls[k].size() * sizeof(uint32_t), hipMemcpyHostToDevice);
				if (e_ != hipSuccess) { sonde_batch_destroy(b); return fail("hipMalloc d_cls", e_); }
				b->units.push_back({ -1, k, 0, b->n_cls[k], 0, nullptr, { nullptr, nullptr } });
			}
		}
		size_t row0 = 0;
		for (int t : { SONDE_IMET4, SONDE_C50 }) {       // AFSK chains: tone demodulator -> 6 kS/s rows -> demod -> framer, one unit per type
			if (b->chlist[t].empty()) continue;
			b->units.push_back({ t, 0, 0, (uint32_t)b->chlist[t].size(), row0, nullptr, { nullptr, nullptr } });
			row0 += b->chlist[t].size();
		}
		{
			if (b->join_mode == 0 && n_afsk == 0 && b->n_classes == 2 && b->n_cls[2] && b->n_cls[3] && b->fuse_fec && b->fixed_epi) {
				b->mixed_one = true;
				b->units.clear();              // (d_cls[2], d_cls[3] stay: the kernel's two channel lists)
			}
		}
		for (auto &u : b->units) {
			CHK(hipStreamCreateWithFlags(&u.st, hipStreamNonBlocking));
			for (int k = 0; k < 2; k++) CHK(hipEventCreateWithFlags(&u.ev_join[k], SD_EV_ORDER));
		}
		const size_t nev = 2 * b->units.size() * SondeBatch::kEvSlots;
		b->evc = new hipEvent_t[nev]();
		for (size_t i = 0; i < nev; i++) CHK(hipEventCreateWithFlags(&b->evc[i], SD_EV_TIMING));
		if (b->join_mode != 0) {
			b->pipeline = true;
			CHK(hipStreamCreateWithFlags(&b->done_stream, hipStreamNonBlocking));
		}
	}
#undef CHK
	for (int k = 0; k < 2; k++) b->h_counts2[k].assign(C, 0);
	*out = b;
	return 0;
}

static int submit_impl(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride, void *stream_, const SdBinsArgs *bins_in);

extern "C" int sonde_batch_submit(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride, void *stream_)
{
	if (!b || !samples) return fail("sonde_batch_submit: null argument");
	if (n_samples == 0 || n_samples % b->granule || n_samples > b->max_samples) return fail("sonde_batch_submit: n_samples must be a multiple of SONDE_TILE (16384 with iMet channels) and <= max_samples");
	if (channel_stride < n_samples) return fail("sonde_batch_submit: channel_stride < n_samples");
	// the kernels read 16 bytes per lane: every channel row must start on a 16-byte boundary
	if (((uintptr_t)samples & 15u) || channel_stride % (16 / sd_sample_bytes(b->input_kind)))
		return fail("sonde_batch_submit: samples must be 16-byte aligned and channel_stride a multiple of 2 (IQ) / 4 (real, 16-bit IQ) / 8 (8-bit IQ) samples");
	return submit_impl(b, samples, n_samples, channel_stride, stream_, nullptr);
}

// The channelizer's decoder batch (created with SONDE_INPUT_REAL) takes its rows as 20 kS/s PHASE samples instead: n_steps 16-bit
// fractions of a turn per channel (a multiple of 2560 = 3 tiles of 48 kS/s output) behind the 16 carried ones; the per-bin
// discriminator (wrapped phase difference), the composite 12/5 resampler - 4:1 decimator (SPEC 3.5 / 3.5b) and everything behind
// them run in bins_kernel.hip, one wave per bin.  The 12 kS/s sondes only (class
// (4, 8)): a 19.5 kHz bin cannot carry an M10 channel (50 kHz in the reference, /root/reference/src/main.hpp:48), and the AFSK
// sondes want 48 kS/s rows.  Internal to the library (channelizer.hip).
int sd_batch_bins_capable(const SondeBatch *b)
{
	if (!b || b->input_kind != SONDE_INPUT_REAL) return 0;
	for (int t = 0; t < SONDE_NTYPES; t++) {
		if (b->chlist[t].empty()) continue;
		if (t == SONDE_IMET4 || t == SONDE_C50) return 0;                     // the tone demodulator wants 48 kS/s rows
		const int k = modem_class(b->md, t);
		if (!(k_cls_nt[k] == 8 && k_cls_decim[k] == 4)) return 0;
	}
	return 1;
}
int sd_batch_submit_bins(SondeBatch *b, const SdBinsArgs *ba, size_t n_steps, void *stream_)
{
	if (!b || !ba || !ba->phases || !ba->carry_rows || !ba->g_comp || !sd_batch_bins_capable(b)) return fail("sd_batch_submit_bins: bad argument");
	//  the launch-unit path knows nothing of phase rows: it would read them as float rows without an error
	if (!b->units.empty()) return fail("sd_batch_submit_bins: the decoder batch behind a channelizer must be one plain launch (no launch units)");
	if (b->d_rescue) return fail("sd_batch_submit_bins: SONDE_FLAG_RS41_RESCUE is not available for the decoder batch behind a channelizer");
	const size_t n_out = n_steps / 5 * 12;
	if (n_steps == 0 || n_steps % 2560 || n_out > b->max_samples || ba->row_stride < n_steps + 16)
		return fail("sd_batch_submit_bins: n_steps must be a multiple of 2560 within max_samples");
	//  sd_bins_kernel reads the rows as uint4 (eight phases) and writes the carry as dwords
	if ((ba->row_stride & 7) || (ba->carry_stride & 7) || ((uintptr_t)ba->phases & 15u) || ((uintptr_t)ba->carry_rows & 15u))
		return fail("sd_batch_submit_bins: phase rows and carry rows must be 16-byte aligned with strides that are multiples of 8 phases");
	return submit_impl(b, ba->phases, n_out, ba->row_stride, stream_, ba);
}

// Time slices of one demod launch that shares the GPU with total_wg workgroups in all: the number of segments S (1: unsliced).
// Cost model fitted to measurements (profiles/r6_ab_seg.txt, MI355X), in units of one tile of a fully occupied GPU (2.69 us): a
// generation of workgroups costs its tiles -- at the rate of its occupancy, a workgroup in a part-filled generation running up to
// 1 / 0.67 times faster -- plus 2.6 tile-times of start and epilogue (7 us: state -> taps -> first tile's round trip; the last rounds,
// K4's catch-up, the frame decoders).  Short segments lose to that overhead: at least 12 tiles per segment.  What it buys: 1280 x 96
// tiles 0.636 -> 0.713 of the HBM peak (S = 2 or 4), 1250 x 24 0.551 -> 0.58 (S = 2); launches that fill whole residencies, and the
// one-residency headline, stay unsliced (S = 2 there: -5 %).  Only at the default completion mode: the late-joined modes hide the tail
// behind the next submit instead.
static int choose_segments(const SondeBatch *b, uint32_t n_wg, uint32_t total_wg, int n_tiles)
{
	(void)n_wg;
	if (b->seg_force > 0) return (b->seg_force <= n_tiles && total_wg > 0) ? b->seg_force : 1;
	if (b->join_mode != 0 || total_wg <= b->residency) return 1;
	static const int cand[] = { 1, 2, 4, 8 };
	int best = 1;
	double best_cost = 1e30;
	for (int S : cand) {
		const int st = (n_tiles + S - 1) / S;
		if (S > 1 && (st < 12 || n_tiles % S)) continue;
		double cost = 0.0;
		for (uint64_t left = (uint64_t)total_wg * (uint64_t)S; left > 0;) {
			const uint64_t g = left < b->residency ? left : b->residency;
			const double occ = (double)g / (double)b->residency;
			cost += (double)st * (occ < 0.67 ? 0.67 : occ) + 2.6;
			left -= g;
		}
		if (cost < best_cost * 0.98) { best_cost = cost; best = S; }      // (a larger S must win by 2 %)
	}
	return best;
}

static int submit_impl(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride, void *stream_, const SdBinsArgs *bins_in)
{
	HIPCHK(hipSetDevice(b->device));
	hipStream_t stream = (hipStream_t)stream_;
	const int n_tiles = (int)(n_samples / SONDE_TILE);
	// the LAST submit of every group of timing_every -- never the first one behind sonde_batch_set_timing's synchronize, where the
	// host has just been idle -- and the very first submit of the batch's life (a one-submit host still gets a figure)
	const bool timed = b->timing_every > 0 && (b->n_submits % (unsigned long)b->timing_every == (unsigned long)b->timing_every - 1 || b->tickets == 0);
	b->n_submits++;
	hipEvent_t *ev = b->ev + 3 * (b->ev_used % SondeBatch::kEvSlots);
	if (timed) HIPCHK(hipEventRecord(ev[0], stream));
	const int slot = (int)(b->tickets & 1);
	SondeFrame *const d_frames = b->d_frames2[slot];
	uint32_t *const d_counts = b->d_counts2[slot];
	const SdFramerOut *fo = b->d_fo2[slot];    // the demod kernel runs the sync search itself and lists complete frames there
	// consecutive submits share the per-channel state: a submit on another stream waits for the previous one
	// (pipelined mixed batches: every class keeps its own stream from submit to submit, which orders them)
	const bool pipe = b->pipeline;
	if (!pipe && b->tickets && stream != b->last_stream) {
		HIPCHK(hipEventRecord(b->ev_xs, b->last_stream));
		HIPCHK(hipStreamWaitEvent(stream, b->ev_xs, 0));
	}
	// the framers of one sonde type, behind the demod launch that produced its bits, on that launch's stream
	// (d_counts: zeroed at creation; every sync kernel rewrites the entry of each channel it owns on every submit)
	bool framer_launched = false;
	// (off, nch: the piece of the type's channel list to work on; nch = 0: all of it)
	auto launch_framers = [&](int t, hipStream_t sk, uint32_t off = 0, uint32_t nch = 0) -> int {
		if (b->chlist[t].empty()) return 0;
		if (!nch) nch = (uint32_t)b->chlist[t].size();
		const uint32_t *list = b->d_chlist[t] + off;
		if (t == SONDE_RS41) {
			if (b->fuse_fec) return 0;             // sync search and FEC ran inside the demod kernel
			sd_launch_framer_rs41(nch, sk, b->d_bitring, b->ring_words, b->d_gfexp, b->d_gflog, b->d_gfswar, b->d_descs,
				d_frames, d_counts, b->max_frames, b->type_frames[SONDE_RS41], list);
		} else if (t == SONDE_C50) {
			sd_launch_framer_c50(nch, sk, b->d_states, b->d_fstates, b->d_bitring, b->ring_words, d_frames, d_counts, b->max_frames, list);
		} else if (t == SONDE_IMET4) {
			sd_launch_framer_imet(nch, sk, b->d_states, b->d_fstates, b->d_bitring, b->ring_words, d_frames, d_counts, b->max_frames, list);
		} else {
			if (b->fixed_epi && !bins_in) return 0;      // decoded in the demod kernel's epilogue (the bins decoder behind a channelizer still takes the kernel)
			sd_launch_framer_other(t, nch, sk, b->d_states, b->d_fstates, b->d_bitring, b->ring_words,
				t == SONDE_M10 ? (const uint8_t *)b->d_m10tab : b->d_g64, b->d_descs, d_frames, d_counts, b->max_frames, b->type_frames[t], list,
				/* with_sync = */ !b->fuse_fec);        // default: the demod kernel has run the sync search (K4) itself
		}
		HIPCHK(hipGetLastError());
		framer_launched = true;
		return 0;
	};
	// SONDE_FLAG_RS41_RESCUE: the second pass over the RS41 records of this submit (SPEC 3.3c), on the stream of the kernel that wrote
	// them and directly behind it (the demod kernel's epilogue, or sd_rsdec_rs41_kernel), before anything joins that stream or records
	// the submit's completion; list = null: every channel of the batch is RS41
	auto launch_rescue = [&](hipStream_t sk, const uint32_t *list, uint32_t nch) -> int {
		if (!b->d_rescue || !nch) return 0;
		sd_launch_rescue_rs41(nch, sk, b->d_gfexp, b->d_gflog, b->d_gfswar, d_frames, d_counts, b->max_frames, list, b->d_rescue);
		HIPCHK(hipGetLastError());
		framer_launched = true;
		return 0;
	};
	const uint32_t n_rs41 = (uint32_t)b->chlist[SONDE_RS41].size();
	const bool all_rs41 = n_rs41 == b->n_channels;
	const bool one_launch = b->units.empty();
	// time slices: every sliced launch of this submit shares seg_base (each channel belongs to exactly one launch)
	uint32_t total_wg = b->n_channels;
	if (!one_launch) { total_wg = 0; for (const SondeBatch::Unit &u : b->units) total_wg += u.n; }
	int max_seg = 1;
	auto slice_of = [&](uint32_t n_wg, int tiles, SdSlice &sl, int decim, int nt) -> const SdSlice * {
		if (!sd_slices_supported(b->input_kind, decim, nt)) return nullptr;
		// the library slices by itself only a submit that is ONE launch: the no-deadlock argument of launch.h (a segment's predecessor
		// has a lower block index of the same grid) is about one grid; several sliced grids side by side (launch units) run only when
		// SondeBatchConfig.time_slices asks for them (tests), under the poll's give-up guard
		if (!one_launch && b->seg_force <= 0) return nullptr;
		const int S = choose_segments(b, n_wg, total_wg, tiles);
		if (S <= 1) return nullptr;
		sl.seg_tiles = (tiles + S - 1) / S; sl.n_wg = n_wg; sl.seg_base = b->seg_base; sl.prog = b->d_prog; sl.err_index = b->n_channels;
		sl.n_seg = (tiles + sl.seg_tiles - 1) / sl.seg_tiles;
		max_seg = std::max(max_seg, (int)sl.n_seg);
		b->sliced_once = true;
		return &sl;
	};
	if (b->mixed_one && !bins_in) {
		sd_launch_demod_mixed(b->input_kind, b->n_cls[2], b->d_cls[2], b->cls_type[2], b->n_cls[3], b->d_cls[3], b->cls_type[3], stream, (const float *)samples, channel_stride,
			n_tiles, b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems, fo);
		HIPCHK(hipGetLastError());
		if (timed) HIPCHK(hipEventRecord(ev[1], stream));
		if (launch_rescue(stream, b->d_chlist[SONDE_RS41], n_rs41)) return -1;
	} else if (one_launch) {
		if (bins_in)      // channelizer bins: one wave per bin (bins_kernel.hip); n_tiles = 3 per block of 2560 phases
			sd_launch_bins(b->n_channels, stream, bins_in->phases, bins_in->row_stride, n_tiles / 3, bins_in->carry_rows, bins_in->carry_stride,
				b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->h_modems, &b->h_fo2[slot], bins_in->g_comp, b->cls_type[b->only_class]);
		else {
			SdSlice sl;
			sd_launch_demod(b->input_kind, k_cls_decim[b->only_class], k_cls_nt[b->only_class], b->n_channels, stream, (const float *)samples, channel_stride, n_tiles,
				b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems, nullptr, false, fo, b->cls_type[b->only_class],
				slice_of(b->n_channels, n_tiles, sl, k_cls_decim[b->only_class], k_cls_nt[b->only_class]));
		}
		HIPCHK(hipGetLastError());
		if (timed) HIPCHK(hipEventRecord(ev[1], stream));
		for (int t = 0; t < SONDE_NTYPES; t++) {
			if (launch_framers(t, stream)) return -1;
			if (t == SONDE_RS41 && launch_rescue(stream, all_rs41 ? nullptr : b->d_chlist[SONDE_RS41], n_rs41)) return -1;
		}
	} else {
		// fork: the launch units are independent (disjoint channels), let them share the GPU; a unit's frame decoder follows
		// its demod kernel on the unit's stream, so that it overlaps the other units' demodulators
		HIPCHK(hipEventRecord(b->ev_fork, stream));
		const size_t nq = n_samples / SD_AF_DEC;
		hipStream_t join_to = pipe ? b->done_stream : stream;
		for (size_t ui = 0; ui < b->units.size(); ui++) {
			const SondeBatch::Unit &u = b->units[ui];
			HIPCHK(hipStreamWaitEvent(u.st, b->ev_fork, 0));
			hipEvent_t *ec = b->evc + 2 * (b->units.size() * (size_t)(b->evc_used % SondeBatch::kEvSlots) + ui);
			if (timed) HIPCHK(hipEventRecord(ec[0], u.st));
			if (u.type == SONDE_IMET4 || u.type == SONDE_C50) {
				// AFSK channels: tone demodulator into 6 kS/s scratch rows, then kernel A's real-input path over those rows
				// (one kernel-A tile = 2048 scratch samples = 16384 input samples)
				float *rows = b->d_afq + u.row0 * (size_t)(b->max_samples / SD_AF_DEC);
				sd_launch_afsk(u.type, b->input_kind, u.n, u.st, (const float *)samples, channel_stride, n_tiles,
					b->d_chlist[u.type], b->d_astates, u.type == SONDE_C50 ? b->d_wtab_c50 : b->d_wtab, rows, nq);
				sd_launch_demod(SONDE_INPUT_REAL, 1, 16, u.n, u.st, rows, nq, (int)(nq / SONDE_TILE),
					b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems, b->d_chlist[u.type], true, fo, u.type);
			} else {
				SdSlice sl;
				sd_launch_demod(b->input_kind, k_cls_decim[u.cls], k_cls_nt[u.cls], u.n, u.st, (const float *)samples, channel_stride, n_tiles,
					b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems,
					u.type < 0 ? b->d_cls[u.cls] : b->d_chlist[u.type] + u.off, false, fo, u.type < 0 ? b->cls_type[u.cls] : u.type,
					slice_of(u.n, n_tiles, sl, k_cls_decim[u.cls], k_cls_nt[u.cls]));
			}
			HIPCHK(hipGetLastError());
			if (timed) HIPCHK(hipEventRecord(ec[1], u.st));
			if (u.type >= 0) {
				if (launch_framers(u.type, u.st, u.off, u.n)) return -1;
				if (u.type == SONDE_RS41 && launch_rescue(u.st, b->d_chlist[SONDE_RS41] + u.off, u.n)) return -1;
			} else {
				for (int t = 0; t < SONDE_NTYPES; t++) {
					if (t == SONDE_IMET4 || t == SONDE_C50 || modem_class(b->md, t) != u.cls) continue;
					if (launch_framers(t, u.st)) return -1;
					if (t == SONDE_RS41 && launch_rescue(u.st, b->d_chlist[SONDE_RS41], n_rs41)) return -1;
				}
			}
			// join: into the caller's stream (work queued there afterwards sees the submit finished), or -- pipelined -- into the
			// library's completion stream only, so that the next submit's units start behind their OWN predecessors and the
			// tail of one unit (its last workgroups draining, its frame decoder) overlaps the other units' next submit
			HIPCHK(hipEventRecord(u.ev_join[slot], u.st));
			HIPCHK(hipStreamWaitEvent(join_to, u.ev_join[slot], 0));
		}
		// join_mode 1: the caller's stream is joined with the PREVIOUS submit's units now (behind this submit's fork), i.e. one submit
		// late: work the caller queues on its stream after this call is ordered behind submit t - 1, and the tail of a unit's
		// submit t - 1 runs beside the other units' submit t
		if (b->join_mode == 1 && b->tickets)
			for (const SondeBatch::Unit &u : b->units) HIPCHK(hipStreamWaitEvent((hipStream_t)stream_, u.ev_join[slot ^ 1], 0));
		if (timed) b->evc_used++;
		if (pipe) stream = b->done_stream;      // where the submit completes: timing end, completion event, sonde_batch_sync
		if (timed) HIPCHK(hipEventRecord(ev[1], stream));
		framer_launched = false;               // inside the fork/join region: timed with the demodulators
	}
	if (timed) {
		if (framer_launched) HIPCHK(hipEventRecord(ev[2], stream));     // nothing behind the demod kernel: no third bubble
		b->ev_has_framer[b->ev_used % SondeBatch::kEvSlots] = framer_launched;
		b->ev_used++;
	}
	// time slices: segment s > 0 waits for the VALUE seg_base + s, which only segment s - 1 of the same launch writes; whatever a
	// channel's counter holds from earlier submits is <= seg_base (sliced or not, whichever launch it was in): never waited for
	if (max_seg > 1) b->seg_base += (uint32_t)max_seg;
	b->ev_valid[slot] = b->ticketing;
	if (b->ticketing) HIPCHK(hipEventRecord(b->ev_done[slot], stream));
	b->tickets++;
	b->last_stream = stream;
	b->pending = true;
	b->have_counts2[slot] = false;
	return 0;
}

// ---------------------------------------------------------------- restart of single channels (SPEC 3.12)
// One workgroup per listed channel puts back what sonde_batch_create set: SdChanState for the channel's type (which stays), zeros in
// the discriminator history, the bit ring, SdFramerState, SdAfskState and the time-slice progress word.  Stores only.
__global__ __launch_bounds__(256) void sd_batch_restart_kernel(const uint32_t *__restrict__ list, SdChanState *__restrict__ states,
	SdFramerState *__restrict__ fstates, float *__restrict__ hist, uint32_t *__restrict__ bitring, uint32_t ring_words,
	SdAfskState *__restrict__ astates, uint32_t *__restrict__ prog, const SdModem *__restrict__ modems)
{
	const uint32_t c = list[blockIdx.x], tid = threadIdx.x;
	uint32_t *ring = bitring + (size_t)c * ring_words;
	for (uint32_t i = tid; i < ring_words; i += 256) ring[i] = 0u;
	for (uint32_t i = tid; i < SD_HIST; i += 256) hist[(size_t)c * SD_HIST + i] = 0.0f;
	if (tid < sizeof(SdFramerState) / 4) ((uint32_t *)(fstates + c))[tid] = 0u;
	if (astates && tid < sizeof(SdAfskState) / 4) ((uint32_t *)(astates + c))[tid] = 0u;
	if (tid == 0) {
		const int32_t type = states[c].type, p0 = modems[type].period0;
		SdChanState st = {};
		st.type = type;
		st.period = p0;
		st.t_next = ((int64_t)SD_NTAPS << 16) + p0;
		st.amp = 0.25f;
		states[c] = st;
		prog[c] = 0u;
	}
}

void sd_batch_mark_channelizer(SondeBatch *b) { if (b) b->behind_channelizer = true; }

extern "C" int sonde_batch_restart_channels(SondeBatch *b, const uint32_t *channels, size_t n)
{
	if (!b || (!channels && n)) return fail("sonde_batch_restart_channels: null argument");
	if (b->behind_channelizer) return fail("sonde_batch_restart_channels: the batch sits behind a channelizer (its bins carry state the batch does not own)");
	for (size_t i = 0; i < n; i++)
		if (channels[i] >= b->n_channels) return fail("sonde_batch_restart_channels: no such channel");
	if (n == 0) return 0;
	// the poll parsers: an entry two submits old no longer separates anything a poll can still parse, so it is dropped (its parser
	// replaced, if there is one) -- the list stays short for a host that never polls
	while (!b->parser_restarts.empty() && b->parser_restarts.front().first + 2 <= b->tickets) {
		if (!b->parsers.empty()) b->parsers[b->parser_restarts.front().second].reset();
		b->parser_restarts.pop_front();
	}
	for (size_t i = 0; i < n; i++) b->parser_restarts.emplace_back(b->tickets, channels[i]);
	if (b->tickets == 0) return 0;             // nothing has run: the device state is what create set
	HIPCHK(hipSetDevice(b->device));
	SdChanLists::Buf *lb = b->restart_lists.put(channels, n);
	if (!lb) return fail("sonde_batch_restart_channels: no pinned memory for the channel list");
	// last_stream is where the last submit completes: the caller's stream (the launch units joined into it), or the completion
	// stream of the late-joined modes, which waits for every unit's last kernel.  The next submit follows it there (or through
	// ev_xs from another stream); launch units that are not joined keep their own streams from submit to submit, so each waits.
	hipStream_t s = b->last_stream;
	hipLaunchKernelGGL(sd_batch_restart_kernel, dim3((unsigned)n), dim3(256), 0, s, lb->dev, b->d_states, b->d_fstates, b->d_hist, b->d_bitring,
		b->ring_words, b->d_astates, b->d_prog, b->d_modems);
	HIPCHK(hipGetLastError());
	if (b->d_rescue) {                         // SPEC 3.3c: a restarted channel has no layout
		sd_launch_rescue_clear((uint32_t)n, s, lb->dev, b->d_rescue);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(b->restart_lists.done(lb, s));
	if (b->pipeline) {
		HIPCHK(hipEventRecord(b->ev_restart, s));
		for (const SondeBatch::Unit &u : b->units) HIPCHK(hipStreamWaitEvent(u.st, b->ev_restart, 0));
	}
	return 0;
}

// Device-side release of the last submit's sample buffer on `stream_` (include/sonde_abi.h).  Unit batches: the units' join events of
// the last submit (recorded behind each unit's last kernel: a superset of its readers); a plain launch: stream order on the submit's
// own stream, an event recorded there now for any other stream.
extern "C" int sonde_batch_wait_input(SondeBatch *b, void *stream_)
{
	if (!b) return fail("sonde_batch_wait_input: null argument");
	if (b->tickets == 0) return 0;
	HIPCHK(hipSetDevice(b->device));
	hipStream_t stream = (hipStream_t)stream_;
	if (!b->units.empty()) {
		const int slot = (int)((b->tickets - 1) & 1);
		for (const SondeBatch::Unit &u : b->units) HIPCHK(hipStreamWaitEvent(stream, u.ev_join[slot], 0));
		return 0;
	}
	if (stream == b->last_stream) return 0;
	HIPCHK(hipEventRecord(b->ev_xs, b->last_stream));
	HIPCHK(hipStreamWaitEvent(stream, b->ev_xs, 0));
	return 0;
}

// How the batch launches and joins (bench / tests label their figures with it): launch units per submit (1: one plain launch on the
// caller's stream) and the join mode (0 at every submit, 1 one submit late, 2 never; only meaningful with more than one unit)
extern "C" int sonde_batch_launch_info(const SondeBatch *b, uint32_t *n_units, int32_t *join_mode)
{
	if (!b) return fail("sonde_batch_launch_info: null argument");
	if (n_units) *n_units = b->units.empty() ? 1u : (uint32_t)b->units.size();
	if (join_mode) *join_mode = b->join_mode;      // what the FLAGS ask for, whatever the unit count (the contract does not depend on the device)
	return 0;
}

// Channel stride (in elements) this library recommends for rows of n_samples: the next power of two in BYTES from 64 KiB up.
// Measured (profiles/r3_stride_sweep.txt, three boxes): 1024 rows of 1.5 MiB streamed side by side run 2.3-5.5 % faster 2 MiB
// apart than back to back (rows 384 KiB -> 512 KiB: +0.8 %); strides a little off a power of two (2064 KiB) can be 7 % SLOWER
// than the contiguous layout: how the rows that are in flight together spread over the HBM channels.
extern "C" size_t sonde_sample_bytes(int input_kind)
{
	return sd_sample_bytes(input_kind);
}

extern "C" size_t sonde_row_stride(size_t n_samples, int input_kind)
{
	const size_t elem = sonde_sample_bytes(input_kind);
	const size_t bytes = n_samples * elem;
	if (bytes < 64 * 1024) return n_samples;
	size_t p = 64 * 1024;
	while (p < bytes) p <<= 1;
	// the padding is never read but it is allocated (the library's own staging buffer, a host's resident blocks): a power of two
	// only where it costs at most a third (1.5 MiB -> 2 MiB); rows just above a power of two would nearly double, and take an ODD
	// number of 64 KiB units instead (consecutive rows then start on different HBM channel groups)
	if (3 * p <= 4 * bytes) return p / elem;
	size_t units = (bytes + 65535) / 65536;
	units |= 1;
	// ... but never beyond the power of two (80 KiB rows got 3 x 64 KiB while 96 KiB rows got 128 KiB -- a stride that
	// shrinks as the row grows overruns buffers sized from the stride of max_samples; capped, the rule is monotonic)
	return std::min(units * 65536, p) / elem;
}

extern "C" int sonde_batch_submit_host(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride)
{
	if (!b || !samples) return fail("sonde_batch_submit_host: null argument");
	if (n_samples == 0 || n_samples % b->granule || n_samples > b->max_samples) return fail("sonde_batch_submit_host: bad n_samples");
	HIPCHK(hipSetDevice(b->device));
	const size_t elem = sonde_sample_bytes(b->input_kind);
	const size_t dstride = sonde_row_stride(n_samples, b->input_kind);            // rows on the recommended stride
	const size_t need = (size_t)b->n_channels * sonde_row_stride(b->max_samples, b->input_kind) * elem;
	if (b->stage_bytes < need) {
		(void)hipFree(b->d_stage);
		b->d_stage = nullptr;
		b->stage_bytes = 0;
		HIPCHK(hipMalloc(&b->d_stage, need));
		b->stage_bytes = need;
	}
	if (b->pending) HIPCHK(hipStreamSynchronize(b->last_stream));
	HIPCHK(hipMemcpy2D(b->d_stage, dstride * elem, samples, channel_stride * elem, n_samples * elem, b->n_channels, hipMemcpyHostToDevice));
	return sonde_batch_submit(b, b->d_stage, n_samples, dstride, nullptr);
}

// wait for submit number `ticket` (1-based) and read its per-channel frame counts; -1 if its slot set has been reused
static long sync_ticket(SondeBatch *b, uint64_t ticket)
{
	if (ticket == 0 || ticket > b->tickets) return fail("sonde_batch: no such submit");
	if (b->tickets - ticket >= 2) return fail("sonde_batch: the frames of that submit have been overwritten (two newer submits)");
	if (hipSetDevice(b->device) != hipSuccess) return fail("hipSetDevice");
	const int slot = (int)((ticket - 1) & 1);
	if (!b->have_counts2[slot]) {
		// with an event: wait for that submit only; without (the host did not ask for tickets before it): for the stream
		hipError_t e = b->ev_valid[slot] ? hipEventSynchronize(b->ev_done[slot]) : hipStreamSynchronize(b->last_stream);
		if (e != hipSuccess) return fail("hipEventSynchronize", e);
		if (ticket == b->tickets || !b->ev_valid[slot]) b->pending = false;
		e = hipMemcpy(b->h_counts2[slot].data(), b->d_counts2[slot], b->n_channels * sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return fail("hipMemcpy counts", e);
		if (b->sliced_once) {      // time slices: a workgroup whose predecessor never published gave up instead of hanging (launch.h SdSlice)
			uint32_t gave_up = 0;
			e = hipMemcpy(&gave_up, b->d_prog + b->n_channels, sizeof(uint32_t), hipMemcpyDeviceToHost);
			if (e != hipSuccess) return fail("hipMemcpy prog", e);
			if (gave_up) return fail("sonde_batch: a time-sliced demod launch found a segment whose predecessor never finished (workgroup dispatch out of order?); the batch's state is undefined -- recreate it");
		}
		long n = 0, over = 0;
		for (uint32_t c = 0; c < b->n_channels; c++) {
			n += std::min(b->h_counts2[slot][c], b->max_frames);
			if (b->h_counts2[slot][c] > b->max_frames) over += b->h_counts2[slot][c] - b->max_frames;
		}
		b->n_frames2[slot] = n;
		b->n_overflow2[slot] = over;
		b->have_counts2[slot] = true;
	}
	return b->n_frames2[slot];
}

extern "C" long sonde_batch_sync(SondeBatch *b)
{
	if (!b) return fail("sonde_batch_sync: null argument");
	if (b->tickets == 0) return 0;
	return sync_ticket(b, b->tickets);
}

extern "C" uint64_t sonde_batch_ticket(SondeBatch *b)
{
	if (!b) return 0;
	b->ticketing = true;        // from the next submit on, every submit records its own completion event
	return b->tickets;
}

extern "C" long sonde_batch_overflow(SondeBatch *b)
{
	if (!b) return fail("sonde_batch_overflow: null argument");
	if (b->tickets == 0) return 0;
	if (sync_ticket(b, b->tickets) < 0) return -1;
	return b->n_overflow2[(b->tickets - 1) & 1];
}

extern "C" long sonde_batch_frames_of(SondeBatch *b, uint64_t ticket, SondeFrame *out, size_t cap)
{
	if (!b) return fail("sonde_batch_frames_of: null argument");
	const long n = sync_ticket(b, ticket);
	if (n < 0) return n;
	if (!out || cap == 0) return n;          // count only: size the buffer from it
	if (n == 0) return 0;
	const int slot = (int)((ticket - 1) & 1);
	const std::vector<uint32_t> &h_counts = b->h_counts2[slot];
	const SondeFrame *d_frames = b->d_frames2[slot];
	// frames sit in per-channel slot groups (ordered by channel, then time): one bulk copy of the slot
	// array when it is small, else one copy per channel that has frames
	size_t k = 0;
	const size_t all = (size_t)b->n_channels * b->max_frames;
	if (all * sizeof(SondeFrame) <= (64u << 20)) {
		b->h_slots.resize(all);
		hipError_t e = hipMemcpy(b->h_slots.data(), d_frames, all * sizeof(SondeFrame), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return fail("hipMemcpy frames", e);
		for (uint32_t c = 0; c < b->n_channels && k < cap; c++) {
			const uint32_t cnt = std::min(h_counts[c], b->max_frames);
			const size_t take = std::min((size_t)cnt, cap - k);
			if (take) memcpy(out + k, b->h_slots.data() + (size_t)c * b->max_frames, take * sizeof(SondeFrame));
			k += take;
		}
		return (long)k;
	}
	for (uint32_t c = 0; c < b->n_channels && k < cap; c++) {
		const uint32_t cnt = std::min(h_counts[c], b->max_frames);
		if (!cnt) continue;
		const size_t take = std::min((size_t)cnt, cap - k);
		hipError_t e = hipMemcpy(out + k, d_frames + (size_t)c * b->max_frames, take * sizeof(SondeFrame), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return fail("hipMemcpy frames", e);
		k += take;
	}
	return (long)k;
}

extern "C" long sonde_batch_frames(SondeBatch *b, SondeFrame *out, size_t cap)
{
	if (!b) return fail("sonde_batch_frames: null argument");
	if (b->tickets == 0) return 0;
	return sonde_batch_frames_of(b, b->tickets, out, cap);
}

extern "C" long sonde_batch_poll(SondeBatch *b, SondeData *out, uint32_t *channel, size_t cap)
{
	if (!b || !out || !channel) return fail("sonde_batch_poll: null argument");
	// every submit since the last poll that is still resident (frame slots exist twice): a pipelined host may have queued
	// submit t + 1 before it polls; the per-channel parsers are stateful (RS41 calibration, DFM date, C50 position), so a
	// skipped submit would not only lose its own fragments
	while (b->polled_ticket < b->tickets) {
		const uint64_t t = b->polled_ticket + 1;
		if (b->tickets - t >= 2) {
			b->polled_ticket = b->tickets - 2;     // resume with what is left, but say so
			return fail("sonde_batch_poll: the frames of an unpolled submit have been overwritten (poll at least every second submit)");
		}
		const long n = sync_ticket(b, t);
		if (n < 0) return n;
		std::vector<SondeFrame> fr((size_t)n);
		const long got = n ? sonde_batch_frames_of(b, t, fr.data(), (size_t)n) : 0;
		if (got < 0) return got;
		if (b->parsers.empty()) b->parsers.resize(b->n_channels);
		// channels restarted before submit t was queued: their frames from here on belong to a new stream, a new parser
		while (!b->parser_restarts.empty() && b->parser_restarts.front().first < t) {
			b->parsers[b->parser_restarts.front().second].reset();
			b->parser_restarts.pop_front();
		}
		std::vector<SondeData> v;
		for (long i = 0; i < got; i++) {
			const uint32_t c = fr[(size_t)i].channel;
			if (c >= b->n_channels) continue;
			if (!b->parsers[c]) b->parsers[c].reset(new SondeParser((int)b->types[c]));
			v.clear();
			b->parsers[c]->feed(fr[(size_t)i], v);
			for (const SondeData &d : v) b->frags.emplace_back(c, d);
		}
		b->polled_ticket = t;
	}
	size_t k = 0;
	while (k < cap && !b->frags.empty()) {
		channel[k] = b->frags.front().first;
		out[k] = b->frags.front().second;
		b->frags.pop_front();
		k++;
	}
	return (long)k;
}

extern "C" int sonde_batch_kernel_ms(SondeBatch *b, float *demod_ms, float *framer_ms)
{
	if (!b) return fail("sonde_batch_kernel_ms: null argument");
	if (sonde_batch_sync(b) < 0) return -1;
	float a = 0.0f, c = 0.0f;
	const int n = std::min(b->ev_used, (int)SondeBatch::kEvSlots);
	if (n == 0) return fail("sonde_batch_kernel_ms: no timed submit since the last query (sonde_batch_set_timing)");
	for (int i = 0; i < n; i++) {
		float x = 0.0f, y = 0.0f;
		HIPCHK(hipEventElapsedTime(&x, b->ev[3 * i], b->ev[3 * i + 1]));
		if (b->ev_has_framer[i]) HIPCHK(hipEventElapsedTime(&y, b->ev[3 * i + 1], b->ev[3 * i + 2]));
		a += x; c += y;
	}
	a /= (float)n; c /= (float)n;
	b->ev_used = 0;
	if (demod_ms) *demod_ms = a;
	if (framer_ms) *framer_ms = c;
	return 0;
}

extern "C" int sonde_batch_set_timing(SondeBatch *b, int every_n)
{
	if (!b || every_n < 0) return fail("sonde_batch_set_timing: bad argument");
	if (sonde_batch_sync(b) < 0) return -1;
	b->timing_every = every_n;
	b->n_submits = 0;
	b->ev_used = 0;
	b->evc_used = 0;
	return 0;
}

// Mixed batches: average device time (ms) of each demodulator class's kernel alone over the timed submits since the last
// call / sonde_batch_set_timing; class index: 0 (decimation 1, 16 taps), 1 (2, 16), 2 (4, 8), 3 (2, 8); -1: class not in the
// batch.  Returns the number of timed submits averaged (0: the batch is one class -- use sonde_batch_kernel_ms).
extern "C" int sonde_batch_class_ms(SondeBatch *b, float out[4])
{
	if (!b || !out) return fail("sonde_batch_class_ms: null argument");
	for (int k = 0; k < 4; k++) out[k] = -1.0f;
	if (!b->evc) return 0;
	if (sonde_batch_sync(b) < 0) return -1;
	const int n = std::min(b->evc_used, (int)SondeBatch::kEvSlots);
	const size_t nu = b->units.size();
	for (int k = 0; k < 4 && n > 0; k++) {
		float acc = 0.0f;
		int cnt = 0;
		for (size_t ui = 0; ui < nu; ui++) {
			const SondeBatch::Unit &u = b->units[ui];
			if (u.type == SONDE_IMET4 || u.type == SONDE_C50 || u.cls != k) continue;
			for (int i = 0; i < n; i++) {
				float x = 0.0f;
				HIPCHK(hipEventElapsedTime(&x, b->evc[2 * (nu * (size_t)i + ui)], b->evc[2 * (nu * (size_t)i + ui) + 1]));
				acc += x;
				cnt++;
			}
		}
		if (cnt) out[k] = acc / (float)cnt;
	}
	b->evc_used = 0;
	return n;
}

// ---------------------------------------------------------------- introspection (staged parity tests)
// The RS(255,231) corrector alone: n_pairs codeword pairs of [2][256] bytes (positions >= n zero), corrected in place;
// status[2 * i + c]: 0 clean, > 0 corrected byte errors, -1 uncorrectable (word left as received).
extern "C" int sonde_batch_test_rs255(SondeBatch *b, uint8_t *cw_pairs, size_t n_pairs, int n, int32_t *status)
{
	if (!b || !cw_pairs || !status || !n_pairs || n < 25 || n > 255) return fail("sonde_batch_test_rs255: bad argument");
	HIPCHK(hipSetDevice(b->device));
	uint8_t *d_cw = nullptr;
	int32_t *d_st = nullptr;
	HIPCHK(hipMalloc((void **)&d_cw, n_pairs * 512));
	if (hipMalloc((void **)&d_st, n_pairs * 2 * sizeof(int32_t)) != hipSuccess) { (void)hipFree(d_cw); return fail("hipMalloc"); }
	hipError_t e = hipMemcpy(d_cw, cw_pairs, n_pairs * 512, hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		sd_launch_rs255_unit(d_cw, (uint32_t)n_pairs, n, d_st, b->d_gfexp, (const uint8_t *)b->d_gflog, b->d_gfswar, nullptr);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpy(cw_pairs, d_cw, n_pairs * 512, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(status, d_st, n_pairs * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
	(void)hipFree(d_cw); (void)hipFree(d_st);
	return e == hipSuccess ? 0 : fail("sonde_batch_test_rs255", e);
}

// The errors-and-erasures corrector of SONDE_FLAG_RS41_RESCUE alone (sd_rsee.h): as above, with erased[i][c][k] != 0 marking position k.
extern "C" int sonde_batch_test_rs255_erasures(SondeBatch *b, uint8_t *cw_pairs, size_t n_pairs, int n, const uint8_t *erased, int32_t *status)
{
	if (!b || !cw_pairs || !erased || !status || !n_pairs || n < 25 || n > 255) return fail("sonde_batch_test_rs255_erasures: bad argument");
	HIPCHK(hipSetDevice(b->device));
	uint8_t *d_cw = nullptr, *d_er = nullptr;
	int32_t *d_st = nullptr;
	hipError_t e = hipMalloc((void **)&d_cw, n_pairs * 512);
	if (e == hipSuccess) e = hipMalloc((void **)&d_er, n_pairs * 512);
	if (e == hipSuccess) e = hipMalloc((void **)&d_st, n_pairs * 2 * sizeof(int32_t));
	if (e == hipSuccess) e = hipMemcpy(d_cw, cw_pairs, n_pairs * 512, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(d_er, erased, n_pairs * 512, hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		sd_launch_rsee_unit(d_cw, d_er, (uint32_t)n_pairs, n, d_st, b->d_gfexp, (const uint8_t *)b->d_gflog, b->d_gfswar, nullptr);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpy(cw_pairs, d_cw, n_pairs * 512, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(status, d_st, n_pairs * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
	(void)hipFree(d_cw); (void)hipFree(d_er); (void)hipFree(d_st);
	return e == hipSuccess ? 0 : fail("sonde_batch_test_rs255_erasures", e);
}

extern "C" int sonde_batch_rescue_info(SondeBatch *b, uint32_t channel, SondeRs41Layout out[2], uint32_t *tried, uint32_t *rescued)
{
	if (!b || channel >= b->n_channels) return fail("sonde_batch_rescue_info: bad argument");
	if (b->behind_channelizer) return fail("sonde_batch_rescue_info: SONDE_FLAG_RS41_RESCUE is not available for the batch behind a channelizer");
	if (!b->d_rescue) return fail("sonde_batch_rescue_info: the batch was created without SONDE_FLAG_RS41_RESCUE (or has no RS41 channel)");
	if (b->types[channel] != SONDE_RS41) return fail("sonde_batch_rescue_info: not an RS41 channel");
	if (sonde_batch_sync(b) < 0) return -1;
	SdRescueState st;
	HIPCHK(hipMemcpy(&st, b->d_rescue + channel, sizeof(st), hipMemcpyDeviceToHost));
	if (out) { out[0] = st.lay[0]; out[1] = st.lay[1]; }
	if (tried) *tried = st.tried;
	if (rescued) *rescued = st.rescued;
	return 0;
}

extern "C" uint64_t sonde_batch_nbits(SondeBatch *b, uint32_t channel)
{
	if (!b || channel >= b->n_channels) { fail("sonde_batch_nbits: bad argument"); return 0; }
	if (sonde_batch_sync(b) < 0) return 0;
	SdChanState st;
	if (hipMemcpy(&st, b->d_states + channel, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) { fail("hipMemcpy state"); return 0; }
	return st.wpos;
}

extern "C" int sonde_batch_read_bits(SondeBatch *b, uint32_t channel, uint64_t from, size_t count, uint8_t *out)
{
	if (!b || channel >= b->n_channels || !out) return fail("sonde_batch_read_bits: bad argument");
	if (sonde_batch_sync(b) < 0) return -1;
	SdChanState st;
	HIPCHK(hipMemcpy(&st, b->d_states + channel, sizeof(st), hipMemcpyDeviceToHost));
	const uint64_t ring_bits = (uint64_t)b->ring_words * 32;
	if (from + count > st.wpos || st.wpos - from > ring_bits) return fail("sonde_batch_read_bits: range not in the ring");
	std::vector<uint32_t> ring(b->ring_words);
	HIPCHK(hipMemcpy(ring.data(), b->d_bitring + (size_t)channel * b->ring_words, (size_t)b->ring_words * 4, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < count; i++) {
		const uint64_t p = from + i;
		out[i] = (ring[(p >> 5) & (b->ring_words - 1)] >> (p & 31)) & 1u;
	}
	return 0;
}

extern "C" int sonde_batch_read_state(SondeBatch *b, uint32_t channel, int64_t *t_next, int32_t *period, float *bias, float *amp, float *afc_u)
{
	if (!b || channel >= b->n_channels) return fail("sonde_batch_read_state: bad argument");
	if (sonde_batch_sync(b) < 0) return -1;
	SdChanState st;
	HIPCHK(hipMemcpy(&st, b->d_states + channel, sizeof(st), hipMemcpyDeviceToHost));
	if (t_next) *t_next = st.t_next;
	if (period) *period = st.period;
	if (bias) *bias = st.bias;
	if (amp) *amp = st.amp;
	if (afc_u) *afc_u = st.afc[2];          // the newest AFC state u (SPEC 3.0b); 0 for real input
	return 0;
}

// ---- read-only streaming probe: the HBM read bandwidth this GPU actually delivers, measured in the same
// process as the bench so that kernel A's GB/s can be quoted against *achievable* as well as against the
// 8 TB/s spec peak (SURVEY.md section 8d asks for both).  Not on the product path.
// 8 independent 16-byte loads in flight per lane, grid-stride; the xor keeps the loads alive and the store
// never happens for real data.
typedef uint32_t sd_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void sd_read_probe_kernel(const sd_u32x4 *__restrict__ src, size_t n16, uint32_t *sink)
{
	const size_t stride = (size_t)gridDim.x * 256;
	size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	uint32_t acc = 0;
	for (; i + 7 * stride < n16; i += 8 * stride) {
		sd_u32x4 v[8];
#pragma unroll
		for (int k = 0; k < 8; k++) v[k] = __builtin_nontemporal_load(src + i + k * stride);
#pragma unroll
		for (int k = 0; k < 8; k++) acc ^= v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
	}
	for (; i < n16; i += stride) {
		const sd_u32x4 v = src[i];
		acc ^= v.x ^ v.y ^ v.z ^ v.w;
	}
	if (acc == 0x5EEDBEEFu) sink[0] = acc;
}

extern "C" int sonde_hbm_read_probe(const void *d_buf, size_t bytes, int reps, float *gbs_out)
{
	if (!d_buf || bytes < 16 || reps < 1 || !gbs_out) return fail("sonde_hbm_read_probe: bad argument");
	uint32_t *sink = nullptr;
	HIPCHK(hipMalloc(&sink, 4));
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0));
	HIPCHK(hipEventCreate(&e1));
	const size_t n16 = bytes / 16;
	float best = 1e30f;
	for (int grid = 256 * 4; grid <= 256 * 32; grid *= 2) {      // best over a few occupancies
		sd_read_probe_kernel<<<grid, 256>>>((const sd_u32x4 *)d_buf, n16, sink);   // warm-up
		for (int r = 0; r < reps; r++) {
			(void)hipEventRecord(e0, 0);
			sd_read_probe_kernel<<<grid, 256>>>((const sd_u32x4 *)d_buf, n16, sink);
			(void)hipEventRecord(e1, 0);
			(void)hipEventSynchronize(e1);
			float ms = 0.f;
			(void)hipEventElapsedTime(&ms, e0, e1);
			if (ms < best) best = ms;
		}
	}
	const hipError_t err = hipGetLastError();
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	(void)hipFree(sink);
	if (err != hipSuccess) return fail("sonde_hbm_read_probe", err);
	*gbs_out = (float)((double)(n16 * 16) / ((double)best * 1e-3) / 1e9);
	return 0;
}
