// batch.hip -- host engine of libsonde_mi355.so: the B0 batch API of include/sonde_abi.h.
//
// Owns the per-channel device state (demod state, ring tail, bit ring, framer state, frame slots),
// launches kernel A (demod_kernel.hip) and kernel B (framer_kernel.hip) back to back on the caller's
// HIP stream, and hands corrected frames back.  There is no CPU fallback: every entry point fails
// with an error if HIP is unavailable.
//
// This file: create / destroy, the launch plan of a submit (submit_impl) and the restart of single channels.  The object is
// batch_impl.h; the tables it uploads are sd_tables.h; frames, poll and the timing queries are batch_results.cpp.
// Its device memory, pinned list buffers, events and streams are members that release themselves (sd_devmem.h): destroy selects the
// device, waits for the batch's own work and deletes; a create that fails half-way deletes the same way.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "batch_impl.h"
#include "sd_input.h"

static uint32_t pow2ceil(uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

// what a channel's demodulator state is before its first sample: at creation, and again after sonde_batch_restart_channels (SPEC 3.12)
static __host__ __device__ inline SdChanState chan_state_init(int32_t type, int32_t period0)
{
	SdChanState st = {};
	st.type = type;
	st.period = period0;
	st.t_next = ((int64_t)SD_NTAPS << 16) + period0;
	st.amp = 0.25f;
	return st;
}

// What destroy waits for: the streams on which the batch may still have work.  last_stream is where the last submit completes and
// where a restart's kernels follow it: the caller's stream (join mode 0, or no launch units), else done_stream, which has joined
// every unit's last kernel.  In the late-joined modes the unit streams may hold a restart's ev_restart wait behind that, so they are
// waited for too.  Nothing else of the batch's can be unfinished then: what a submit leaves on the caller's stream in those modes
// (the timing start, ev_fork, join mode 1's waits for the previous submit's ev_join) precedes what the unit streams have completed.
// After the wait no member is in use, and the order in which they are released does not matter.
extern "C" void sonde_batch_destroy(SondeBatch *b)
{
	if (!b) return;
	(void)hipSetDevice(b->device);
	if (b->pending) (void)hipStreamSynchronize(b->last_stream);
	if (b->join_mode != 0) {
		for (const SondeBatch::Unit &u : b->units) (void)hipStreamSynchronize(u.st);
		if (b->done_stream) (void)hipStreamSynchronize(b->done_stream);
	}
	delete b;
}

// ---------------------------------------------------------------- create
static int upload_fec_tables(SondeBatch *b)
{
	uint8_t exp2[SD_GFEXP_BYTES];
	uint16_t log2[256];
	uint32_t swar[24 * 8];
	uint8_t g64[192];
	uint16_t m10[99 * 8];
	fec_gf256_tables(exp2, log2);
	fec_gf256_swar(swar);
	fec_gf64_tables(g64);
	fec_m10_table(m10);
	HIPCHK(b->d_gfexp.upload(exp2, sizeof(exp2)));
	HIPCHK(b->d_gflog.upload((const uint8_t *)log2, sizeof(log2)));
	HIPCHK(b->d_gfswar.upload(swar, 24 * 8));
	HIPCHK(b->d_g64.upload(g64, sizeof(g64)));
	HIPCHK(b->d_m10tab.upload(m10, 99 * 8));
	b->fec = { b->d_gfexp, b->d_gflog, b->d_gfswar, b->d_g64, b->d_m10tab };
	return 0;
}

// the sonde types whose channels run in demod class k (the AFSK types run behind the tone demodulator: in no class's launch)
static uint32_t class_types(const SondeBatch *b, int k)
{
	uint32_t m = 0;
	for (int t = 0; t < SONDE_NTYPES; t++)
		if (t != SONDE_IMET4 && t != SONDE_C50 && modem_class(b->md, t) == k) m |= 1u << t;
	return m;
}

// Everything behind the argument checks; on failure sonde_batch_create destroys what has been built so far.
static int build(SondeBatch *b, const SondeBatchConfig *cfg)
{
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
	if (prop.multiProcessorCount <= 0) return sd_fail("sonde_batch_create: the device reports no compute units");
	b->residency = 4u * (uint32_t)prop.multiProcessorCount;
	b->n_channels = cfg->n_channels;
	b->max_samples = cfg->max_samples;
	b->input_kind = cfg->input_kind;
	b->seg_force = (int)cfg->time_slices;
	b->join_mode = (cfg->flags & SONDE_FLAG_PIPELINE) ? 2 : ((cfg->flags & SONDE_FLAG_LATE_JOIN) ? 1 : 0);
	b->fuse_fec = (cfg->flags & SONDE_FLAG_SPLIT_FEC) ? 0u : 1u;
	for (const SdDivPass &p : k_div_passes) b->div_flags |= cfg->flags & p.flag;
	if (!b->fuse_fec) b->fixed_epi = 0;
	modem_table(cfg->flags, cfg->input_kind, b->md);
	const ModemDef *md = b->md;
	b->types.assign(cfg->n_channels, SONDE_RS41);
	if (cfg->types) b->types.assign(cfg->types, cfg->types + cfg->n_channels);
	for (uint32_t c = 0; c < b->n_channels; c++) {
		const int t = b->types[c];
		if (t < 0 || t >= SONDE_NTYPES) return sd_fail("sonde_batch_create: bad sonde type");
		b->chlist[t].push_back(c);
	}
	// the bit ring holds a submit of the fastest type plus a frame; frames per submit per type: submit bits / shortest frame of the
	// type, + carry-over
	static const uint32_t min_frame_bits[SONDE_NTYPES] = { 320 * 8, 560, 1152, 1648, 140, 90, 768 };
	uint64_t max_bits = 0;
	b->max_frames = 2;
	for (int t = 0; t < SONDE_NTYPES; t++) {
		if (b->chlist[t].empty()) continue;
		const uint64_t bits_t = bits_per_submit(md, t, cfg->max_samples);
		max_bits = std::max(max_bits, bits_t);
		b->type_frames[t] = (uint32_t)(bits_t / min_frame_bits[t]) + 2;
		b->max_frames = std::max(b->max_frames, b->type_frames[t]);
	}
	b->ring_words = pow2ceil((uint32_t)((max_bits + 8 * SONDE_FRAME_MAX + 1024 + 31) / 32));
	// the fixed-length framers stage the whole ring in LDS next to a few static words: keep it below the 64 KB workgroup limit
	if ((size_t)b->ring_words * 4 >= 65536) return sd_fail("sonde_batch_create: max_samples too large for the LDS-staged bit ring (< 64 KB)");

	// ---- demod classes and launch units
	const size_t C = b->n_channels;
	const size_t n_afsk = b->chlist[SONDE_IMET4].size() + b->chlist[SONDE_C50].size();      // tone-demodulated sondes
	std::vector<uint32_t> cls[4];               // index: demod-kernel class (k_cls_decim, k_cls_nt)
	for (uint32_t c = 0; c < b->n_channels; c++) {
		if (b->types[c] == SONDE_IMET4 || b->types[c] == SONDE_C50) continue;
		const int k = modem_class(md, b->types[c]);
		if (k < 0) return sd_fail("sonde_batch_create: no demodulator class for this sonde type");
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
	int one_class_units = 1;
	if (b->join_mode != 0 && n_afsk == 0 && b->n_classes == 1) {
		int n_types = 0;
		for (int t = 0; t < SONDE_NTYPES; t++) n_types += !b->chlist[t].empty();
		// two units where a single launch would end with a part-filled generation of workgroups; a channel count that fills whole
		// residencies stays ONE plain launch on the caller's stream (two units measured +1-2 % there: not worth the lagging join;
		// the headline shape, 1024 channels, and BASELINE config 5's shard, 8192, are such counts)
		one_class_units = (n_types == 1 && b->n_channels >= 512 && b->n_channels % b->residency != 0) ? 2 : 1;
		if (cfg->launch_units) one_class_units = std::max(1, std::min(16, (int)cfg->launch_units));      // (experiments: profiles/r4_units_sweep.txt)
	}
	const bool need_lists = n_afsk != 0 || b->n_classes > 1 || one_class_units > 1;
	if (n_afsk) {
		if (cfg->max_samples % (SONDE_TILE * SD_AF_DEC)) return sd_fail("sonde_batch_create: with iMet channels max_samples must be a multiple of 16384");
		b->granule = SONDE_TILE * SD_AF_DEC;
	}

	// ---- per-channel state
	std::vector<SdChanState> st(C);
	SdModem modems[SONDE_NTYPES];
	modem_fill(md, modems);
	memcpy(b->h_modems, modems, sizeof(modems));
	for (size_t c = 0; c < C; c++) st[c] = chan_state_init(b->types[c], modems[b->types[c]].period0);
	HIPCHK(b->d_states.upload(st.data(), C));
	HIPCHK(b->d_fstates.zeros(C));
	HIPCHK(b->d_hist.zeros(C * SD_HIST));
	HIPCHK(b->d_bitring.zeros(C * (size_t)b->ring_words));
	HIPCHK(b->d_prog.zeros(C + 1));
	uint32_t types_present = 0;
	for (int t = 0; t < SONDE_NTYPES; t++) types_present |= (uint32_t)!b->chlist[t].empty() << t;
	for (int k = 0; k < SD_N_PASSES; k++) {      // the rescue passes asked for that have a channel to work on: no layout, counters zero
		const SdRescuePass &p = k_rescue_passes[k];
		if ((cfg->flags & p.flag) && (types_present & p.types)) HIPCHK(b->d_pass[k].zeros(C * p.words));
	}
	if (b->d_pass[SD_PASS_MANCHESTER] && sd_batch_need_mrztab(b)) return -1;
	if (n_afsk) {
		float wtab[2 * SD_AF_PER], wc[2 * SD_C50_PER];
		make_mixer(wtab, 17, SD_AF_PER);         // iMet: 1700 Hz
		make_mixer(wc, 19, SD_C50_PER);          // C50: 3800 Hz, midway between the 2900 / 4700 Hz tones
		HIPCHK(b->d_wtab.upload(wtab, 2 * SD_AF_PER));
		HIPCHK(b->d_wtab_c50.upload(wc, 2 * SD_C50_PER));
		HIPCHK(b->d_astates.zeros(C));
		HIPCHK(b->d_afq.alloc(n_afsk * (size_t)(cfg->max_samples / SD_AF_DEC)));
	}

	// ---- tables and channel lists
	std::vector<float> taps((size_t)SONDE_NTYPES * SD_NPHASE * SD_NTAPS);
	for (int t = 0; t < SONDE_NTYPES; t++) make_taps(md, t, &taps[(size_t)t * SD_NPHASE * SD_NTAPS]);
	HIPCHK(b->d_taps.upload(taps.data(), taps.size()));
	HIPCHK(b->d_modems.upload(modems, SONDE_NTYPES));
	if (upload_fec_tables(b)) return -1;
	HIPCHK(b->d_descs.alloc(C * (size_t)b->max_frames * SD_DESC_BYTES));
	for (int t = 0; t < SONDE_NTYPES; t++)
		if (!b->chlist[t].empty()) HIPCHK(b->d_chlist[t].upload(b->chlist[t].data(), b->chlist[t].size()));

	// ---- the two slot sets
	for (SondeBatch::Slot &s : b->slot) {
		HIPCHK(s.d_frames.alloc(C * (size_t)b->max_frames));
		HIPCHK(s.d_counts.zeros(C));
		s.h_fo = { b->d_fstates, b->d_descs, s.d_counts, b->max_frames, b->fuse_fec, /* loop_fec_max_wg = */ b->residency, b->fec.gfexp, b->fec.gflog, b->fec.gfswar,
		           b->fec.g64, s.d_frames, b->fec.m10tab, b->fixed_epi };
		HIPCHK(s.d_fo.upload(&s.h_fo, 1));
		HIPCHK(s.ev_done.create(hipEventDisableTiming));
		s.h_counts.assign(C, 0);
	}
	HIPCHK(b->ev_xs.create(SD_EV_ORDER));
	HIPCHK(b->ev_restart.create(SD_EV_ORDER));
	b->timing.submit.resize(SdTiming::kSlots);
	for (SdTiming::Submit &s : b->timing.submit) for (DevEvent &e : s.ev) HIPCHK(e.create(SD_EV_TIMING));
	if (!need_lists) return 0;

	// ---- launch units
	HIPCHK(b->ev_fork.create(SD_EV_ORDER));
	if (b->join_mode != 0) {
		// per type; pieces per type: one (2-8 pieces of every type of a mixed batch measured 6-70 % slower, profiles/r3_notes.md); a one-type batch: two
		const int R = one_class_units;
		b->n_chunks = R;
		static const int order[] = { SONDE_M10, SONDE_RS41, SONDE_DFM09, SONDE_IMS100, SONDE_MRZN1 };
		for (int j = 0; j < R; j++)
			for (int t : order) {
				const size_t nt = b->chlist[t].size();
				const size_t lo = nt * (size_t)j / (size_t)R, hi = nt * (size_t)(j + 1) / (size_t)R;
				if (hi > lo) b->units.push_back({ t, modem_class(md, t), (uint32_t)lo, (uint32_t)(hi - lo), 0, 1u << t });
			}
	} else {
		// per class; class order: the class with the longest-running workgroups (M10: twice the symbols per tile) first, then the 4:1
		// class (whose RS41 workgroups end with the FEC epilogue): best of all orders in round 2 (profiles/r2_notes.md)
		for (int k : { 3, 0, 2, 1 }) {
			if (!b->n_cls[k]) continue;
			HIPCHK(b->d_cls[k].upload(cls[k].data(), cls[k].size()));
			b->units.push_back({ -1, k, 0, b->n_cls[k], 0, class_types(b, k) });
		}
	}
	size_t row0 = 0;
	for (int t : { SONDE_IMET4, SONDE_C50 }) {       // AFSK chains: tone demodulator -> 6 kS/s rows -> demod -> framer, one unit per type
		if (b->chlist[t].empty()) continue;
		b->units.push_back({ t, 0, 0, (uint32_t)b->chlist[t].size(), row0, 1u << t });
		row0 += b->chlist[t].size();
	}
	if (b->join_mode == 0 && n_afsk == 0 && b->n_classes == 2 && b->n_cls[2] && b->n_cls[3] && b->fuse_fec && b->fixed_epi) {
		b->mixed_one = true;
		b->units.clear();              // (d_cls[2], d_cls[3] stay: the kernel's two channel lists)
	}
	for (auto &u : b->units) {
		HIPCHK(u.st.create());
		for (DevEvent &e : u.ev_join) HIPCHK(e.create(SD_EV_ORDER));
	}
	b->timing.unit.resize(2 * b->units.size() * SdTiming::kSlots);
	for (DevEvent &e : b->timing.unit) HIPCHK(e.create(SD_EV_TIMING));
	if (b->join_mode != 0) HIPCHK(b->done_stream.create());
	return 0;
}

extern "C" int sonde_batch_create(const SondeBatchConfig *cfg, SondeBatch **out)
{
	if (!cfg || !out) return sd_fail("sonde_batch_create: null argument");
	*out = nullptr;
	//  a caller compiled against an older, shorter SondeBatchConfig, or one that did not zero the struct, must not hand
	// over garbage in the members it does not know about: the size it was compiled with is part of the struct
	if (cfg->struct_size != sizeof(SondeBatchConfig))
		return sd_fail("sonde_batch_create: SondeBatchConfig.struct_size != sizeof(SondeBatchConfig) -- initialise with SONDE_BATCH_CONFIG_INIT (a host built against an older sonde_abi.h must be recompiled)");
	if (cfg->launch_units > 16) return sd_fail("sonde_batch_create: launch_units must be 0 (the library's choice) or 1..16");
	if (cfg->time_slices > 16) return sd_fail("sonde_batch_create: time_slices must be 0 (the library's choice) or 1..16");
	if (cfg->n_channels == 0) return sd_fail("sonde_batch_create: n_channels == 0");
	if (cfg->max_samples == 0 || cfg->max_samples % SONDE_TILE) return sd_fail("sonde_batch_create: max_samples must be a positive multiple of SONDE_TILE");
	if (!sd_input_known(cfg->input_kind)) return sd_fail("sonde_batch_create: bad input_kind");
	if (sd_select_device(cfg->device, "sonde_batch_create")) return -1;

	SondeBatch *b = new SondeBatch;
	b->device = cfg->device;
	if (build(b, cfg)) { sonde_batch_destroy(b); return -1; }       // (destroy leaves the error text alone)
	*out = b;
	return 0;
}

// ---------------------------------------------------------------- submit
static int submit_impl(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride, void *stream_, const SdBinsArgs *bins_in);

extern "C" int sonde_batch_submit(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride, void *stream_)
{
	if (!b || !samples) return sd_fail("sonde_batch_submit: null argument");
	if (n_samples == 0 || n_samples % b->granule || n_samples > b->max_samples) return sd_fail("sonde_batch_submit: n_samples must be a multiple of SONDE_TILE (16384 with iMet channels) and <= max_samples");
	if (channel_stride < n_samples) return sd_fail("sonde_batch_submit: channel_stride < n_samples");
	// the kernels read 16 bytes per lane: every channel row must start on a 16-byte boundary
	if (((uintptr_t)samples & 15u) || channel_stride % (16 / sd_sample_bytes(b->input_kind)))
		return sd_fail("sonde_batch_submit: samples must be 16-byte aligned and channel_stride a multiple of 2 (IQ) / 4 (real, 16-bit IQ) / 8 (8-bit IQ) samples");
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
	if (!b || !ba || !ba->phases || !ba->carry_rows || !ba->g_comp || !sd_batch_bins_capable(b)) return sd_fail("sd_batch_submit_bins: bad argument");
	//  the launch-unit path knows nothing of phase rows: it would read them as float rows without an error
	if (!b->units.empty()) return sd_fail("sd_batch_submit_bins: the decoder batch behind a channelizer must be one plain launch (no launch units)");
	for (int k = 0; k < SD_N_PASSES; k++)
		if (b->d_pass[k])
			return sd_fail((std::string("sd_batch_submit_bins: ") + k_rescue_passes[k].flag_name + " is not available for the decoder batch behind a channelizer").c_str());
	if (b->n_groups) return sd_fail("sd_batch_submit_bins: sonde_batch_set_diversity is not available for the decoder batch behind a channelizer");
	const size_t n_out = n_steps / 5 * 12;
	if (n_steps == 0 || n_steps % 2560 || n_out > b->max_samples || ba->row_stride < n_steps + 16)
		return sd_fail("sd_batch_submit_bins: n_steps must be a multiple of 2560 within max_samples");
	//  sd_bins_kernel reads the rows as uint4 (eight phases) and writes the carry as dwords
	if ((ba->row_stride & 7) || (ba->carry_stride & 7) || ((uintptr_t)ba->phases & 15u) || ((uintptr_t)ba->carry_rows & 15u))
		return sd_fail("sd_batch_submit_bins: phase rows and carry rows must be 16-byte aligned with strides that are multiples of 8 phases");
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
static int choose_segments(const SondeBatch *b, uint32_t total_wg, int n_tiles)
{
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

// One submit on its way through the launch plan (submit_impl)
struct SubmitCtx {
	const void *samples; size_t n_samples, channel_stride;
	const SdBinsArgs *bins;                // the rows are a channelizer's phase rows (sd_batch_submit_bins), else null
	hipStream_t stream;                    // the caller's
	hipStream_t done;                      // where the submit completes: the caller's stream, or the completion stream of the late-joined modes
	int n_tiles;
	SondeBatch::Slot *slot;                // this submit's frame slots, counts and framer descriptor
	int parity;                            // its index: Unit::ev_join[parity]
	SdTiming::Submit *timed;               // this submit's timing events; null: not timed
	uint32_t total_wg;                     // demod workgroups of all launches of this submit
	int max_seg = 1;                       // most time-slice segments any launch of it was cut into
	bool framer_launched = false;          // something ran behind the demodulators on `done`: the third timing event is worth its bubble
};

// The frame decoder of one sonde type, behind the demod launch that produced its bits, on that launch's stream
// (d_counts: zeroed at creation; every sync kernel rewrites the entry of each channel it owns on every submit).
// (off, nch: the piece of the type's channel list to work on; nch = 0: all of it)
static int launch_framers(SondeBatch *b, SubmitCtx &cx, int t, hipStream_t sk, uint32_t off, uint32_t nch)
{
	if (b->chlist[t].empty()) return 0;
	if (!nch) nch = (uint32_t)b->chlist[t].size();
	const uint32_t *list = b->d_chlist[t] + off;
	SondeFrame *const d_frames = cx.slot->d_frames;
	uint32_t *const d_counts = cx.slot->d_counts;
	if (t == SONDE_RS41) {
		if (b->fuse_fec) return 0;             // sync search and FEC ran inside the demod kernel
		sd_launch_framer_rs41(nch, sk, b->d_bitring, b->ring_words, b->fec.gfexp, b->fec.gflog, b->fec.gfswar, b->d_descs,
			d_frames, d_counts, b->max_frames, b->type_frames[SONDE_RS41], list);
	} else if (t == SONDE_C50) {
		sd_launch_framer_c50(nch, sk, b->d_states, b->d_fstates, b->d_bitring, b->ring_words, d_frames, d_counts, b->max_frames, list);
	} else if (t == SONDE_IMET4) {
		sd_launch_framer_imet(nch, sk, b->d_states, b->d_fstates, b->d_bitring, b->ring_words, d_frames, d_counts, b->max_frames, list);
	} else {
		if (b->fixed_epi && !cx.bins) return 0;      // decoded in the demod kernel's epilogue (the bins decoder behind a channelizer still takes the kernel)
		sd_launch_framer_other(t, nch, sk, b->d_states, b->d_fstates, b->d_bitring, b->ring_words,
			t == SONDE_M10 ? (const uint8_t *)b->fec.m10tab : b->fec.g64, b->d_descs, d_frames, d_counts, b->max_frames, b->type_frames[t], list,
			/* with_sync = */ !b->fuse_fec);        // default: the demod kernel has run the sync search (K4) itself
	}
	HIPCHK(hipGetLastError());
	cx.framer_launched = true;
	return 0;
}

// What follows a demod launch on its stream sk: the frame decoders of the sonde types it covered (a bit mask), each over the piece
// [off, off + nch) of its type's channel list (nch = 0: the whole list), and behind each type's decoders the rescue passes the batch
// has for that type over the same channels: directly behind the kernel that wrote the records, before anything joins that stream or
// records the submit's completion.  whole_batch: the launch covered channels 0..n-1 of an all-RS41 batch, and the pass needs no list.
static int launch_decoders(SondeBatch *b, SubmitCtx &cx, uint32_t types, hipStream_t sk, uint32_t off = 0, uint32_t nch = 0, bool whole_batch = false)
{
	for (int t = 0; t < SONDE_NTYPES; t++) {
		if (!(types >> t & 1u)) continue;
		if (launch_framers(b, cx, t, sk, off, nch)) return -1;
		const uint32_t n = nch ? nch : (uint32_t)b->chlist[t].size();
		for (int k = 0; k < SD_N_PASSES; k++) {
			if (!(k_rescue_passes[k].types >> t & 1u) || !b->d_pass[k] || !n) continue;
			k_rescue_passes[k].launch({ n, sk, b->fec, b->d_mrztab, b->d_states, b->d_bitring, b->ring_words, cx.slot->d_frames, cx.slot->d_counts,
				b->max_frames, whole_batch ? nullptr : b->d_chlist[t] + off, b->d_pass[k] });
			HIPCHK(hipGetLastError());
			cx.framer_launched = true;
		}
	}
	return 0;
}
static const uint32_t kAllTypes = (1u << SONDE_NTYPES) - 1;

// The time slices of one demod launch of n_wg workgroups (launch.h SdSlice): null = unsliced.  Every sliced launch of a submit
// shares seg_base (each channel belongs to exactly one launch).
static const SdSlice *slice_of(SondeBatch *b, SubmitCtx &cx, uint32_t n_wg, int decim, int nt, SdSlice &sl)
{
	if (!sd_slices_supported(b->input_kind, decim, nt)) return nullptr;
	// the library slices by itself only a submit that is ONE launch: the no-deadlock argument of launch.h (a segment's predecessor
	// has a lower block index of the same grid) is about one grid; several sliced grids side by side (launch units) run only when
	// SondeBatchConfig.time_slices asks for them (tests), under the poll's give-up guard
	if (!b->units.empty() && b->seg_force <= 0) return nullptr;
	const int S = choose_segments(b, cx.total_wg, cx.n_tiles);
	if (S <= 1) return nullptr;
	sl.seg_tiles = (cx.n_tiles + S - 1) / S; sl.n_wg = n_wg; sl.seg_base = b->seg_base; sl.prog = b->d_prog; sl.err_index = b->n_channels;
	sl.n_seg = (cx.n_tiles + sl.seg_tiles - 1) / sl.seg_tiles;
	cx.max_seg = std::max(cx.max_seg, (int)sl.n_seg);
	b->sliced_once = true;
	return &sl;
}

// Step 1.  Consecutive submits share the per-channel state: a submit on another stream waits for the previous one
// (late-joined batches: every unit keeps its own stream from submit to submit, which orders them)
static int order_behind_previous(SondeBatch *b, const SubmitCtx &cx)
{
	if (b->join_mode != 0 || !b->tickets || cx.stream == b->last_stream) return 0;
	HIPCHK(hipEventRecord(b->ev_xs, b->last_stream));
	HIPCHK(hipStreamWaitEvent(cx.stream, b->ev_xs, 0));
	return 0;
}

// Steps 2 and 3, the two default classes at the default completion mode: ONE launch, every frame decoder in its epilogue
static int launch_mixed(SondeBatch *b, SubmitCtx &cx)
{
	sd_launch_demod_mixed(b->input_kind, b->n_cls[2], b->d_cls[2], b->cls_type[2], b->n_cls[3], b->d_cls[3], b->cls_type[3], cx.stream, (const float *)cx.samples,
		cx.channel_stride, cx.n_tiles, b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems, cx.slot->d_fo);
	HIPCHK(hipGetLastError());
	if (cx.timed) HIPCHK(hipEventRecord(cx.timed->ev[1], cx.stream));
	return launch_decoders(b, cx, kAllTypes, cx.stream);       // (in the epilogue: what is left is the rescue pass)
}

// Steps 2 and 3, one class: one plain launch over channels 0..n-1 on the caller's stream, the decoders that are not in its epilogue behind it
static int launch_plain(SondeBatch *b, SubmitCtx &cx)
{
	const int k = b->only_class;
	if (cx.bins)      // channelizer bins: one wave per bin (bins_kernel.hip); n_tiles = 3 per block of 2560 phases
		sd_launch_bins(b->n_channels, cx.stream, cx.bins->phases, cx.bins->row_stride, cx.n_tiles / 3, cx.bins->carry_rows, cx.bins->carry_stride,
			b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->h_modems, &cx.slot->h_fo, cx.bins->g_comp, b->cls_type[k]);
	else {
		SdSlice sl;
		sd_launch_demod(b->input_kind, k_cls_decim[k], k_cls_nt[k], b->n_channels, cx.stream, (const float *)cx.samples, cx.channel_stride, cx.n_tiles,
			b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems, nullptr, false, cx.slot->d_fo, b->cls_type[k],
			slice_of(b, cx, b->n_channels, k_cls_decim[k], k_cls_nt[k], sl));
	}
	HIPCHK(hipGetLastError());
	if (cx.timed) HIPCHK(hipEventRecord(cx.timed->ev[1], cx.stream));
	return launch_decoders(b, cx, kAllTypes, cx.stream, 0, 0, /* whole_batch = */ b->chlist[SONDE_RS41].size() == b->n_channels);
}

// one launch unit's demodulator on the unit's stream
static int launch_unit_demod(SondeBatch *b, SubmitCtx &cx, const SondeBatch::Unit &u)
{
	if (u.type == SONDE_IMET4 || u.type == SONDE_C50) {
		// AFSK channels: tone demodulator into 6 kS/s scratch rows, then kernel A's real-input path over those rows
		// (one kernel-A tile = 2048 scratch samples = 16384 input samples)
		const size_t nq = cx.n_samples / SD_AF_DEC;
		float *rows = b->d_afq + u.row0 * (size_t)(b->max_samples / SD_AF_DEC);
		sd_launch_afsk(u.type, b->input_kind, u.n, u.st, (const float *)cx.samples, cx.channel_stride, cx.n_tiles,
			b->d_chlist[u.type], b->d_astates, u.type == SONDE_C50 ? b->d_wtab_c50 : b->d_wtab, rows, nq);
		sd_launch_demod(SONDE_INPUT_REAL, 1, 16, u.n, u.st, rows, nq, (int)(nq / SONDE_TILE),
			b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems, b->d_chlist[u.type], true, cx.slot->d_fo, u.type);
	} else {
		SdSlice sl;
		sd_launch_demod(b->input_kind, k_cls_decim[u.cls], k_cls_nt[u.cls], u.n, u.st, (const float *)cx.samples, cx.channel_stride, cx.n_tiles,
			b->d_states, b->d_hist, b->d_bitring, b->ring_words, b->d_taps, b->d_modems,
			u.type < 0 ? b->d_cls[u.cls] : b->d_chlist[u.type] + u.off, false, cx.slot->d_fo, u.type < 0 ? b->cls_type[u.cls] : u.type,
			slice_of(b, cx, u.n, k_cls_decim[u.cls], k_cls_nt[u.cls], sl));
	}
	HIPCHK(hipGetLastError());
	return 0;
}

// Steps 2 and 3, launch units.  Fork: the units are independent (disjoint channels), let them share the GPU; a unit's frame
// decoders follow its demod kernel on the unit's stream, so that they overlap the other units' demodulators.  Join: into the
// caller's stream (work queued there afterwards sees the submit finished), or -- late-joined -- into the library's completion
// stream only, so that the next submit's units start behind their OWN predecessors and the tail of one unit (its last workgroups
// draining, its frame decoders) overlaps the other units' next submit
static int launch_units(SondeBatch *b, SubmitCtx &cx)
{
	HIPCHK(hipEventRecord(b->ev_fork, cx.stream));
	const hipStream_t join_to = b->join_mode != 0 ? b->done_stream : cx.stream;
	for (size_t ui = 0; ui < b->units.size(); ui++) {
		const SondeBatch::Unit &u = b->units[ui];
		HIPCHK(hipStreamWaitEvent(u.st, b->ev_fork, 0));
		DevEvent *ec = cx.timed ? b->timing.unit_pair(b->units.size(), b->timing.unit_used % SdTiming::kSlots, ui) : nullptr;
		if (ec) HIPCHK(hipEventRecord(ec[0], u.st));
		if (launch_unit_demod(b, cx, u)) return -1;
		if (ec) HIPCHK(hipEventRecord(ec[1], u.st));
		// a per-type unit: its piece of the type's list; a per-class unit: the whole lists of the class's types
		if (launch_decoders(b, cx, u.types, u.st, u.type >= 0 ? u.off : 0, u.type >= 0 ? u.n : 0)) return -1;
		HIPCHK(hipEventRecord(u.ev_join[cx.parity], u.st));
		HIPCHK(hipStreamWaitEvent(join_to, u.ev_join[cx.parity], 0));
	}
	// join_mode 1: the caller's stream is joined with the PREVIOUS submit's units now (behind this submit's fork), i.e. one submit
	// late: work the caller queues on its stream after this call is ordered behind submit t - 1, and the tail of a unit's
	// submit t - 1 runs beside the other units' submit t
	if (b->join_mode == 1 && b->tickets)
		for (const SondeBatch::Unit &u : b->units) HIPCHK(hipStreamWaitEvent(cx.stream, u.ev_join[cx.parity ^ 1], 0));
	cx.done = join_to;
	if (cx.timed) {
		b->timing.unit_used++;
		HIPCHK(hipEventRecord(cx.timed->ev[1], cx.done));
	}
	cx.framer_launched = false;            // inside the fork/join region: timed with the demodulators
	return 0;
}

// Step 4
static int record_completion(SondeBatch *b, SubmitCtx &cx)
{
	if (cx.timed) {
		if (cx.framer_launched) HIPCHK(hipEventRecord(cx.timed->ev[2], cx.done));     // nothing behind the demod kernel: no third bubble
		cx.timed->has_framer = cx.framer_launched;
		b->timing.used++;
	}
	// time slices: segment s > 0 waits for the VALUE seg_base + s, which only segment s - 1 of the same launch writes; whatever a
	// channel's counter holds from earlier submits is <= seg_base (sliced or not, whichever launch it was in): never waited for
	if (cx.max_seg > 1) b->seg_base += (uint32_t)cx.max_seg;
	cx.slot->ev_valid = b->ticketing;
	if (b->ticketing) HIPCHK(hipEventRecord(cx.slot->ev_done, cx.done));
	cx.slot->have_counts = false;
	b->tickets++;
	b->last_stream = cx.done;
	b->pending = true;
	return 0;
}

// Behind every other kernel of the submit, where it completes (the launch units have joined there: set_diversity refuses the
// late-joined modes): the align step (SPEC 3.3k: it sets the offsets and lock bits the passes read, and marks duplicates), then the
// passes of k_div_passes over the groups of sonde_batch_set_diversity: each kernel takes the groups of its kinds out of the one
// table, and is launched only if there is one
static int launch_diversity(SondeBatch *b, SubmitCtx &cx)
{
	SdDivArgs a = {};
	a.n_groups = b->n_groups; a.stream = cx.done;
	a.groups = b->d_groups; a.states = b->d_divstate; a.carried = b->d_carried; a.counters = b->d_divcnt;
	a.other_kinds = (b->div_kinds & ~(1u << SONDE_RS41)) != 0;      // with RS41 groups only the kernels run as they did
	a.frames = cx.slot->d_frames; a.counts = cx.slot->d_counts; a.max_frames = b->max_frames;
	a.fec = b->fec; a.mrztab = b->d_mrztab;
	a.chan_states = b->d_states; a.bitring = b->d_bitring; a.ring_words = b->ring_words;
	if (b->div_mode) {
		sd_launch_diversity_align(a, b->div_mode);
		HIPCHK(hipGetLastError());
	}
	for (const SdDivPass &p : k_div_passes) {
		if (!(b->div_kinds & p.kinds)) continue;
		a.window = b->div_window ? b->div_window : p.window;
		a.kinds = p.kinds;
		p.launch(a);
		HIPCHK(hipGetLastError());
	}
	cx.framer_launched = true;
	return 0;
}

// The launch plan of a submit: (1) order it behind the previous one, (2) launch the demodulators -- the one-launch mixed kernel, one
// plain launch (or the bins decoder), or the launch units with their fork and join --, (3) the decoders behind each launch,
// (4) record completion.
static int submit_impl(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride, void *stream_, const SdBinsArgs *bins_in)
{
	HIPCHK(hipSetDevice(b->device));
	SdTiming &tm = b->timing;
	SubmitCtx cx = {};
	cx.samples = samples; cx.n_samples = n_samples; cx.channel_stride = channel_stride; cx.bins = bins_in;
	cx.stream = cx.done = (hipStream_t)stream_;
	cx.n_tiles = (int)(n_samples / SONDE_TILE);
	cx.parity = (int)(b->tickets & 1);
	cx.slot = &b->slot[cx.parity];
	cx.total_wg = b->n_channels;
	if (!b->units.empty()) { cx.total_wg = 0; for (const SondeBatch::Unit &u : b->units) cx.total_wg += u.n; }
	// timed: the LAST submit of every group of tm.every -- never the first one behind sonde_batch_set_timing's synchronize, where the
	// host has just been idle -- and the very first submit of the batch's life (a one-submit host still gets a figure)
	if (tm.every > 0 && (tm.n_submits % (unsigned long)tm.every == (unsigned long)tm.every - 1 || b->tickets == 0)) cx.timed = &tm.slot();
	tm.n_submits++;
	if (cx.timed) HIPCHK(hipEventRecord(cx.timed->ev[0], cx.stream));

	if (order_behind_previous(b, cx)) return -1;
	int rc;
	if (b->mixed_one && !bins_in) rc = launch_mixed(b, cx);
	else if (b->units.empty()) rc = launch_plain(b, cx);
	else rc = launch_units(b, cx);
	if (!rc && b->n_groups) rc = launch_diversity(b, cx);
	return rc ? -1 : record_completion(b, cx);
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
		const int32_t type = states[c].type;
		states[c] = chan_state_init(type, modems[type].period0);
		prog[c] = 0u;
	}
}

// The state of a rescue pass, `words` dwords per channel, back to zero for the n listed channels (every word of every listed state:
// one thread each)
__global__ __launch_bounds__(64) void sd_rescue_clear_kernel(const uint32_t *__restrict__ list, uint32_t n, uint32_t *__restrict__ states, uint32_t words)
{
	const uint32_t i = 64 * blockIdx.x + threadIdx.x;
	if (i < n * words) states[(size_t)list[i / words] * words + i % words] = 0u;
}
static void sd_launch_rescue_clear(uint32_t n, hipStream_t stream, const uint32_t *list, uint32_t *states, uint32_t words)
{
	hipLaunchKernelGGL(sd_rescue_clear_kernel, dim3((n * words + 63) / 64), dim3(64), 0, stream, list, n, states, words);
}

void sd_batch_mark_channelizer(SondeBatch *b) { if (b) b->behind_channelizer = true; }

extern "C" int sonde_batch_restart_channels(SondeBatch *b, const uint32_t *channels, size_t n)
{
	if (!b || (!channels && n)) return sd_fail("sonde_batch_restart_channels: null argument");
	if (b->behind_channelizer) return sd_fail("sonde_batch_restart_channels: the batch sits behind a channelizer (its bins carry state the batch does not own)");
	for (size_t i = 0; i < n; i++)
		if (channels[i] >= b->n_channels) return sd_fail("sonde_batch_restart_channels: no such channel");
	if (n == 0) return 0;
	if (b->n_groups) {      // SPEC 3.3j: the members of a group share a time base, so they restart together or not at all
		std::vector<uint32_t> listed(b->n_groups, 0u);
		for (size_t i = 0; i < n; i++) {
			const int32_t slot = b->div_slot[channels[i]];
			if (slot >= 0) listed[(size_t)slot / SD_DIV_MAX] |= 1u << (slot % SD_DIV_MAX);
		}
		std::vector<uint32_t> all(b->n_groups, 0u);
		for (const int32_t slot : b->div_slot)
			if (slot >= 0) all[(size_t)slot / SD_DIV_MAX] |= 1u << (slot % SD_DIV_MAX);
		for (uint32_t g = 0; g < b->n_groups; g++)
			if (listed[g] && listed[g] != all[g]) return sd_fail("sonde_batch_restart_channels: the list must hold all members of a diversity group or none of them");
	}
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
	if (!lb) return sd_fail("sonde_batch_restart_channels: no pinned memory for the channel list");
	// last_stream is where the last submit completes: the caller's stream (the launch units joined into it), or the completion
	// stream of the late-joined modes, which waits for every unit's last kernel.  The next submit follows it there (or through
	// ev_xs from another stream); launch units that are not joined keep their own streams from submit to submit, so each waits.
	hipStream_t s = b->last_stream;
	hipLaunchKernelGGL(sd_batch_restart_kernel, dim3((unsigned)n), dim3(256), 0, s, lb->list.dev(), b->d_states, b->d_fstates, b->d_hist, b->d_bitring,
		b->ring_words, b->d_astates, b->d_prog, b->d_modems);
	HIPCHK(hipGetLastError());
	for (int k = 0; k < SD_N_PASSES; k++) {     // SPEC 3.3c .. 3.3i: a restarted channel has no layout, and its counters are zero
		if (!b->d_pass[k]) continue;
		sd_launch_rescue_clear((uint32_t)n, s, lb->list.dev(), b->d_pass[k], k_rescue_passes[k].words);
		HIPCHK(hipGetLastError());
	}
	if (b->n_groups) {                         // SPEC 3.3j: a restarted group has no carried records, and its counters are zero
		sd_launch_diversity_clear((uint32_t)n, s, lb->list.dev(), b->d_divslot, b->d_carried, b->d_divcnt, b->d_groups, b->d_divstate, b->div_unlocked);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(b->restart_lists.done(lb, s));
	b->pending = true;                         // (sonde_batch_destroy, sonde_batch_submit_host: last_stream holds work again)
	if (b->join_mode != 0) {
		HIPCHK(hipEventRecord(b->ev_restart, s));
		for (const SondeBatch::Unit &u : b->units) HIPCHK(hipStreamWaitEvent(u.st, b->ev_restart, 0));
	}
	return 0;
}

// ---------------------------------------------------------------- test introspection: stream age (DESIGN "Stream age")
// The listed channels become "the same stream, begun earlier": one thread per entry adds to every ABSOLUTE position the batch carries
// for the channel and touches nothing relative.  The list below is sd_batch_restart_kernel's list of the state that exists, read for
// what counts from the stream's origin:
//   SdChanState     n0 (+ dn0 internal-rate samples), t_next (+ dn0 << 16), wpos (+ dbits); period, nstat, bias, amp, iq_last, afc: relative
//   SdFramerState   rpos, fstart (+ dbits; fstart is read only while collecting, and is then a position); collecting, inv, flen: relative
//   SdAfskState     n (+ samples; the tone mixers' phases are n mod 480 and n mod 240); iq_last, b, z: relative
//   hist, bit ring  contents only; dbits is a whole number of ring turns, so every ring index stays where it is
//   prog            a segment count of the launch plan, not a stream position
//   rescue passes   (k_rescue_passes) RS41: learned block layouts and two counters; the other four: two counters.  No position: the
//                   passes take every position from the records' bitpos and the channel's wpos
//   diversity       the carried record of the channel's slot: bitpos (+ dbits, if there is a record).  SdDivGroup.off / SdDivState.off
//                   are differences of bit counts against the group's clock: members shifted alike keep them
//   frame slots, descriptors   written anew by every submit; the records of earlier submits keep the positions they were given
// entry i of the list: 8 words { channel, 0, dn0 lo, hi, samples lo, hi, dbits lo, hi }.  Plain loads and stores.
__global__ __launch_bounds__(64) void sd_batch_shift_age_kernel(const uint32_t *__restrict__ list, uint32_t n, SdChanState *__restrict__ states,
	SdFramerState *__restrict__ fstates, SdAfskState *__restrict__ astates, const int32_t *__restrict__ divslot, SondeFrame *__restrict__ carried)
{
	const uint32_t i = 64 * blockIdx.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t *e = list + 8 * (size_t)i;
	const uint32_t c = e[0];
	const uint64_t dn0 = (uint64_t)e[2] | (uint64_t)e[3] << 32, samples = (uint64_t)e[4] | (uint64_t)e[5] << 32, dbits = (uint64_t)e[6] | (uint64_t)e[7] << 32;
	states[c].n0 += (int64_t)dn0;
	states[c].t_next += (int64_t)(dn0 << 16);
	states[c].wpos += dbits;
	fstates[c].rpos += dbits;
	fstates[c].fstart += dbits;
	const int32_t type = states[c].type;
	if (astates && (type == SONDE_IMET4 || type == SONDE_C50)) astates[c].n += samples;
	if (divslot && divslot[c] >= 0 && carried[divslot[c]].len != 0) carried[divslot[c]].bitpos += dbits;
}

#define SD_AGE_QUANTUM 30720u      // lcm(SONDE_TILE, SD_AF_PER) (and a multiple of SD_C50_PER and of every decimation): tile and mixer phases stay

extern "C" int sonde_batch_test_shift_age(SondeBatch *b, const uint32_t *channels, size_t n, const uint64_t *samples, const uint32_t *ring_turns,
	uint64_t *bits_added)
{
	if (!b || !channels || !samples || !ring_turns || !bits_added || !n) return sd_fail("sonde_batch_test_shift_age: null argument");
	if (b->behind_channelizer) return sd_fail("sonde_batch_test_shift_age: the batch sits behind a channelizer (its bins carry state the batch does not own)");
	if (b->tickets == 0) return sd_fail("sonde_batch_test_shift_age: nothing has run yet (shift after the first submit)");
	const uint64_t ring_bits = 32ull * b->ring_words;
	std::vector<int64_t> at(b->n_channels, -1);        // channel -> its entry
	for (size_t i = 0; i < n; i++) {
		if (channels[i] >= b->n_channels) return sd_fail("sonde_batch_test_shift_age: no such channel");
		if (at[channels[i]] >= 0) return sd_fail("sonde_batch_test_shift_age: a channel listed twice");
		if (samples[i] % SD_AGE_QUANTUM) return sd_fail("sonde_batch_test_shift_age: samples must be a multiple of 30720 (tile phase and both tone-mixer phases stay)");
		if (samples[i] >> 62 || (uint64_t)ring_turns[i] * ring_bits >> 62) return sd_fail("sonde_batch_test_shift_age: shift too large");
		at[channels[i]] = (int64_t)i;
	}
	if (b->n_groups) {      // SPEC 3.3j: the members of a group share the clock bitpos - offset: all of them, by one amount, or none
		std::vector<int64_t> first(b->n_groups, -1);
		std::vector<uint32_t> listed(b->n_groups, 0u), all(b->n_groups, 0u);
		for (uint32_t c = 0; c < b->n_channels; c++) {
			const int32_t slot = b->div_slot[c];
			if (slot < 0) continue;
			const size_t g = (size_t)slot / SD_DIV_MAX;
			all[g] |= 1u << (slot % SD_DIV_MAX);
			if (at[c] < 0) continue;
			listed[g] |= 1u << (slot % SD_DIV_MAX);
			if (first[g] < 0) first[g] = at[c];
			if (samples[at[c]] != samples[first[g]] || ring_turns[at[c]] != ring_turns[first[g]])
				return sd_fail("sonde_batch_test_shift_age: the members of a diversity group must be shifted by the same amount");
		}
		for (uint32_t g = 0; g < b->n_groups; g++)
			if (listed[g] && listed[g] != all[g]) return sd_fail("sonde_batch_test_shift_age: the list must hold all members of a diversity group or none of them");
	}
	std::vector<uint32_t> words(8 * n);
	for (size_t i = 0; i < n; i++) {
		const int t = b->types[channels[i]];
		const uint64_t dn0 = samples[i] / (uint64_t)modem_div(b->md, t);      // the class decimation; 8 behind the tone front-end
		bits_added[i] = (uint64_t)ring_turns[i] * ring_bits;
		const uint64_t v[4] = { channels[i], dn0, samples[i], bits_added[i] };
		for (int k = 0; k < 4; k++) { words[8 * i + 2 * k] = (uint32_t)v[k]; words[8 * i + 2 * k + 1] = (uint32_t)(v[k] >> 32); }
	}
	HIPCHK(hipSetDevice(b->device));
	SdChanLists::Buf *lb = b->restart_lists.put(words.data(), words.size());
	if (!lb) return sd_fail("sonde_batch_test_shift_age: no pinned memory for the list");
	// ordered as sonde_batch_restart_channels orders its kernel: behind the last submit where it completes, in front of the next one
	hipStream_t s = b->last_stream;
	hipLaunchKernelGGL(sd_batch_shift_age_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, lb->list.dev(), (uint32_t)n, b->d_states, b->d_fstates,
		b->d_astates, b->d_divslot, b->d_carried);
	HIPCHK(hipGetLastError());
	HIPCHK(b->restart_lists.done(lb, s));
	b->pending = true;
	if (b->join_mode != 0) {
		HIPCHK(hipEventRecord(b->ev_restart, s));
		for (const SondeBatch::Unit &u : b->units) HIPCHK(hipStreamWaitEvent(u.st, b->ev_restart, 0));
	}
	return 0;
}

// MRZ-N1's column table (SPEC 3.3f step 3), for SONDE_FLAG_MANCHESTER_RESCUE and for an MRZ-N1 diversity group (SPEC 3.3l): whoever
// needs it first uploads it
int sd_batch_need_mrztab(SondeBatch *b)
{
	if (b->d_mrztab) return 0;
	uint16_t mrz[43 * 8];
	fec_mrz_table(mrz);
	HIPCHK(b->d_mrztab.upload(mrz, 43 * 8));
	return 0;
}

// The receivers of one sonde (include/sonde_abi.h, SPEC 3.3j, 3.3k, 3.3l, 3.3m and 3.3n): the group table, the carried records, the counters and the
// align step's state.  mode 0 is sonde_batch_set_diversity.
extern "C" int sonde_batch_set_diversity(SondeBatch *b, const int32_t *group, const int64_t *offset_bits, uint32_t window_bits)
{
	return sonde_batch_set_diversity_auto(b, group, offset_bits, window_bits, 0u);
}

extern "C" int sonde_batch_set_diversity_auto(SondeBatch *b, const int32_t *group, const int64_t *offset_bits, uint32_t window_bits, uint32_t mode)
{
	if (!b || !group) return sd_fail("sonde_batch_set_diversity: null argument");
	if (mode & ~(SONDE_DIVERSITY_LEARN | SONDE_DIVERSITY_MARK_DUPLICATES)) return sd_fail("sonde_batch_set_diversity_auto: unknown mode bits");
	if (b->n_groups) return sd_fail("sonde_batch_set_diversity: called twice");
	if (b->tickets) return sd_fail("sonde_batch_set_diversity: must be called before the first submit");
	if (b->behind_channelizer) return sd_fail("sonde_batch_set_diversity: not available for the batch behind a channelizer");
	if (b->join_mode != 0)
		return sd_fail("sonde_batch_set_diversity: not available with SONDE_FLAG_LATE_JOIN / SONDE_FLAG_PIPELINE (the launch units never join into one stream)");
	if (window_bits > 1200) return sd_fail("sonde_batch_set_diversity: window_bits > 1200");
	if (b->max_frames >= 0xFFFFu) return sd_fail("sonde_batch_set_diversity: too many frames per submit");
	int32_t top = -1;
	for (uint32_t c = 0; c < b->n_channels; c++) {
		if (group[c] < -1 || (uint32_t)(group[c] + 1) > b->n_channels) return sd_fail("sonde_batch_set_diversity: bad group id");
		top = std::max(top, group[c]);
	}
	if (top < 0) return sd_fail("sonde_batch_set_diversity: no group");
	std::vector<SdDivGroup> gt((size_t)top + 1);
	std::vector<int32_t> slot(b->n_channels, -1);
	// the types a member can have: the kinds of the passes whose create flag is set; as the refusal lists them: "A, B or C"
	uint32_t kinds = 0, takes = 0;
	std::string not_one = "sonde_batch_set_diversity: a member that is not ";
	for (const SdDivPass &p : k_div_passes) {
		if ((b->div_flags & p.flag) != p.flag) continue;
		if (takes) not_one += ", ";
		not_one += p.names;
		takes |= p.kinds;
	}
	not_one.replace(not_one.rfind(", "), 2, " or ");
	for (SdDivGroup &g : gt) g = SdDivGroup{};
	for (uint32_t c = 0; c < b->n_channels; c++) {
		if (group[c] < 0) continue;
		SdDivGroup &g = gt[(size_t)group[c]];
		const uint32_t t = b->types[c];
		if (!(takes >> t & 1u)) return sd_fail(not_one.c_str());
		if (g.n && g.kind != t) return sd_fail("sonde_batch_set_diversity: members of different types in one group");
		g.kind = t;
		kinds |= 1u << t;
		if (g.n == SD_DIV_MAX) return sd_fail("sonde_batch_set_diversity: a group with more than 4 members");
		g.ch[g.n] = c;
		g.off[g.n] = offset_bits ? offset_bits[c] : 0;
		slot[c] = (int32_t)(SD_DIV_MAX * (uint32_t)group[c] + g.n);
		g.n++;
	}
	for (const SdDivGroup &g : gt)
		if (g.n < 2) return sd_fail(g.n ? "sonde_batch_set_diversity: a group with fewer than 2 members" : "sonde_batch_set_diversity: group ids with gaps");
	for (const SdDivPass &p : k_div_passes) {      // SPEC 3.3o: what a C50 group asks of the whole call
		if (!(kinds & p.kinds)) continue;
		if (p.max_window && window_bits > p.max_window)
			return sd_fail("sonde_batch_set_diversity: window_bits > 44 with a SONDE_C50 group (its packets lie 90 symbols apart)");
		if (p.given_offsets_only && mode)
			return sd_fail("sonde_batch_set_diversity_auto: a SONDE_C50 group takes given offsets only (its packets carry no identity: mode must be 0)");
	}
	HIPCHK(hipSetDevice(b->device));
	for (const SdDivPass &p : k_div_passes)
		if ((kinds & p.mrz_kinds) && sd_batch_need_mrztab(b)) return -1;      // the pass of SPEC 3.3l reads MRZ-N1's columns from it
	HIPCHK(b->d_groups.upload(gt.data(), gt.size()));
	HIPCHK(b->d_carried.zeros(gt.size() * SD_DIV_MAX));
	HIPCHK(b->d_divcnt.zeros(gt.size() * 2));
	HIPCHK(b->d_divslot.upload(slot.data(), slot.size()));
	// SPEC 3.3k: with SONDE_DIVERSITY_LEARN and no offsets nothing is known and every member starts unlocked; else all are locked
	const bool unlocked = (mode & SONDE_DIVERSITY_LEARN) && !offset_bits;
	std::vector<SdDivState> st(gt.size());
	for (size_t g = 0; g < gt.size(); g++) {
		st[g] = SdDivState{};
		for (uint32_t m = 0; m < gt[g].n; m++) st[g].off[m] = gt[g].off[m];
		st[g].locked = unlocked ? 0u : (1u << gt[g].n) - 1u;
	}
	HIPCHK(b->d_divstate.upload(st.data(), st.size()));
	b->div_kinds = kinds;
	b->div_mode = mode;
	b->div_unlocked = unlocked ? 1u : 0u;
	b->div_slot = slot;
	b->div_window = window_bits;
	b->n_groups = (uint32_t)gt.size();
	return 0;
}

// Device-side release of the last submit's sample buffer on `stream_` (include/sonde_abi.h).  Unit batches: the units' join events of
// the last submit (recorded behind each unit's last kernel: a superset of its readers); a plain launch: stream order on the submit's
// own stream, an event recorded there now for any other stream.
extern "C" int sonde_batch_wait_input(SondeBatch *b, void *stream_)
{
	if (!b) return sd_fail("sonde_batch_wait_input: null argument");
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
	if (!b) return sd_fail("sonde_batch_launch_info: null argument");
	if (n_units) *n_units = b->units.empty() ? 1u : (uint32_t)b->units.size();
	if (join_mode) *join_mode = b->join_mode;      // what the FLAGS ask for, whatever the unit count (the contract does not depend on the device)
	return 0;
}

extern "C" int sonde_batch_submit_host(SondeBatch *b, const void *samples, size_t n_samples, size_t channel_stride)
{
	if (!b || !samples) return sd_fail("sonde_batch_submit_host: null argument");
	if (n_samples == 0 || n_samples % b->granule || n_samples > b->max_samples) return sd_fail("sonde_batch_submit_host: bad n_samples");
	HIPCHK(hipSetDevice(b->device));
	const size_t elem = sonde_sample_bytes(b->input_kind);
	const size_t dstride = sonde_row_stride(n_samples, b->input_kind);            // rows on the recommended stride
	const size_t need = (size_t)b->n_channels * sonde_row_stride(b->max_samples, b->input_kind) * elem;
	if (b->stage_bytes < need) {
		b->stage_bytes = 0;
		HIPCHK(b->d_stage.alloc(need));
		b->stage_bytes = need;
	}
	if (b->pending) HIPCHK(hipStreamSynchronize(b->last_stream));
	HIPCHK(hipMemcpy2D(b->d_stage, dstride * elem, samples, channel_stride * elem, n_samples * elem, b->n_channels, hipMemcpyHostToDevice));
	return sonde_batch_submit(b, b->d_stage, n_samples, dstride, nullptr);
}
