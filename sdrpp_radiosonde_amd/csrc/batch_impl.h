// batch_impl.h -- private to the batch files (batch.hip: create / submit / restart; batch_results.cpp: frames, poll, timing queries;
// batch_probe.hip: test introspection): the SondeBatch object behind the B0 batch API of include/sonde_abi.h.
#pragma once
#include <hip/hip_runtime.h>
#include <deque>
#include <memory>
#include <type_traits>
#include <vector>
#include "sonde_dev.h"
#include "../../include/sonde_abi.h"
#include "launch.h"
#include "parse.h"
#include "sd_chanlist.h"
#include "sd_devmem.h"
#include "sd_host.h"
#include "sd_tables.h"

// Events that only order streams of this device, or time kernels on it, need no system-scope release (a cache write-back
// towards the host): hipEventDisableSystemFence.  Slot::ev_done is what the host waits on before it reads frames: it keeps the fence.
#ifndef SD_EV_FLAGS
#define SD_EV_FLAGS hipEventDisableSystemFence
#endif
#define SD_EV_TIMING (SD_EV_FLAGS)
#define SD_EV_ORDER  (hipEventDisableTiming | SD_EV_FLAGS)

#pragma GCC visibility push(hidden)       // private types: their inline members are not among the library's exported symbols
// The rescue passes (launch.h, DESIGN "what a rescue pass plugs into"), one row each: what create, submit, restart and the info
// entries need to know about a pass
struct SdRescuePass {
	uint32_t flag; const char *flag_name;  // SONDE_FLAG_*_RESCUE and its name
	uint32_t types;                        // bit t: the pass follows the frame decoders of sonde type t
	uint32_t words;                        // dwords of state per channel (the counters are the last two)
	void (*launch)(const SdRescueArgs &);
	const char *info;                      // its introspection entry, sonde_batch_*_rescue_info
	const char *article, *kind;            // "has no <kind> channel", "not <article> <kind> channel"
};
enum { SD_PASS_RS41, SD_PASS_MANCHESTER, SD_PASS_DFM, SD_PASS_IMS, SD_PASS_AFSK, SD_N_PASSES };
static const SdRescuePass k_rescue_passes[SD_N_PASSES] = {
	{ SONDE_FLAG_RS41_RESCUE, "SONDE_FLAG_RS41_RESCUE", 1u << SONDE_RS41, sizeof(SdRescueState) / 4, sd_launch_rescue_rs41,
	  "sonde_batch_rescue_info", "an", "RS41" },
	{ SONDE_FLAG_MANCHESTER_RESCUE, "SONDE_FLAG_MANCHESTER_RESCUE", 1u << SONDE_M10 | 1u << SONDE_MRZN1, 2, sd_launch_rescue_manchester,
	  "sonde_batch_manchester_rescue_info", "an", "M10 / M20 / MRZ-N1" },
	{ SONDE_FLAG_DFM_RESCUE, "SONDE_FLAG_DFM_RESCUE", 1u << SONDE_DFM09, 2, sd_launch_rescue_dfm, "sonde_batch_dfm_rescue_info", "a", "DFM" },
	{ SONDE_FLAG_IMS_RESCUE, "SONDE_FLAG_IMS_RESCUE", 1u << SONDE_IMS100, 2, sd_launch_rescue_ims, "sonde_batch_ims_rescue_info", "an", "iMS-100" },
	{ SONDE_FLAG_AFSK_RESCUE, "SONDE_FLAG_AFSK_RESCUE", 1u << SONDE_IMET4 | 1u << SONDE_C50, 2, sd_launch_rescue_afsk,
	  "sonde_batch_afsk_rescue_info", "an", "iMet or C50" },
};

// The combining passes of sonde_batch_set_diversity (launch.h, DESIGN "what a combining pass plugs into"), one row each: what
// set_diversity, submit and the unit entries need to know about a pass.  The kernels are launched in this order, each over the whole
// group table; the rows' kinds are disjoint
struct SdDivPass {
	uint32_t kinds;                        // bit t: the pass takes the groups of sonde type t
	void (*launch)(const SdDivArgs &);
	uint32_t window;                       // its window where the caller gives none: 960 bits; iMS-100 576 chips (frames lie 1152 apart)
	uint32_t flag;                         // the create flag a member needs; 0: none
	uint32_t mrz_kinds;                    // a group of one of these kinds: the pass reads d_mrztab
	const char *names;                     // its kinds as the refusal of a member of no pass lists them
	struct { uint32_t type, len, to; } frames[4];  // the frames of its kinds: (type, length) pairs, or (type, len .. to) with to != 0; ended by a length of 0
	uint32_t max_window;                   // the largest window a caller may give a table with one of its groups; 0: the call's own limit
	bool given_offsets_only;               // its frames carry no identity: no align step (sonde_batch_set_diversity_auto's mode bits are refused)
};
enum { SD_DIV_RS41, SD_DIV_CHECK, SD_DIV_DFM, SD_DIV_IMS, SD_DIV_IMET, SD_DIV_C50, SD_N_DIV_PASSES };
static const SdDivPass k_div_passes[SD_N_DIV_PASSES] = {
	{ 1u << SONDE_RS41, sd_launch_diversity, 960, 0, 0, "SONDE_RS41", { { SONDE_RS41, 320 }, { SONDE_RS41, 518 } } },
	{ 1u << SONDE_M10 | 1u << SONDE_MRZN1, sd_launch_check_diversity, 960, 0, 1u << SONDE_MRZN1, "SONDE_M10, SONDE_MRZN1",
	  { { SONDE_M10, 101 }, { SONDE_M10, 70 }, { SONDE_MRZN1, 45 } } },
	{ 1u << SONDE_DFM09, sd_launch_dfm_diversity, 960, 0, 0, "SONDE_DFM09", { { SONDE_DFM09, 33 } } },
	{ 1u << SONDE_IMS100, sd_launch_ims_diversity, 576, SONDE_FLAG_IMS_DIVERSITY, 0, "SONDE_IMS100", { { SONDE_IMS100, 51 } } },
	// SPEC 3.3o: one launcher, one row per kind -- bitpos counts on-air symbols, an iMet packet of one length comes once a second, C50
	// packets lie 90 symbols apart: 160 and 40, and no caller's window above 44 for a table with a C50 group
	{ 1u << SONDE_IMET4, sd_launch_afsk_diversity, 160, SONDE_FLAG_AFSK_DIVERSITY, 0, "SONDE_IMET4", { { SONDE_IMET4, 5, 64 } } },
	{ 1u << SONDE_C50, sd_launch_afsk_diversity, 40, SONDE_FLAG_AFSK_DIVERSITY, 0, "SONDE_C50", { { SONDE_C50, 9 } }, 44, true },
};
// a frame of one of the pass's kinds
static inline bool sd_div_is_frame(const SdDivPass &p, uint32_t type, uint32_t len)
{
	for (const auto &f : p.frames)
		if (f.len && f.type == type && len >= f.len && len <= (f.to ? f.to : f.len)) return true;
	return false;
}

// Timing events.  An event record is a bubble of a few microseconds in the command stream (three of them cost a 0.29 ms step 3 %), so
// only every `every`-th submit is timed (0: none), into the next of kSlots slots; all events are created with the batch.
struct SdTiming {
	static const int kSlots = 128;         // submits timed between two sonde_batch_kernel_ms() calls
	struct Submit { DevEvent ev[3]; bool has_framer = false; };      // start, behind the demodulators, behind the frame decoders (if any ran behind)
	std::vector<Submit> submit;            // [kSlots]
	int used = 0;
	// batches of launch units: the same for each unit's demod kernel alone, on the unit's stream (sonde_batch_class_ms)
	std::vector<DevEvent> unit;            // [kSlots][units][2]
	int unit_used = 0;
	int every = 8;
	unsigned long n_submits = 0;           // since sonde_batch_set_timing

	Submit &slot() { return submit[(size_t)(used % kSlots)]; }
	DevEvent *unit_pair(size_t n_units, int slot, size_t ui) { return &unit[2 * (n_units * (size_t)slot + ui)]; }
};

// The object owns its device memory, events and streams through the members of sd_devmem.h: sonde_batch_destroy waits for the batch's
// work and deletes, and a build() that fails half-way leaves an object that deletes the same way.  Launchers and kernels take plain
// pointers: the members convert.
struct SondeBatch {
	uint32_t n_channels = 0, max_samples = 0;
	int input_kind = 0, device = 0;
	uint32_t ring_words = 0, max_frames = 0;
	uint32_t type_frames[SONDE_NTYPES] = {};   // upper bound of complete frames per submit, per sonde type (B2 grid)
	std::vector<uint8_t> types;
	std::vector<uint32_t> chlist[SONDE_NTYPES];
	ModemDef md[SONDE_NTYPES];             // this batch's modem table (k_modems, with the configuration flags applied)

	DevBuf<SdChanState> d_states;
	DevBuf<SdFramerState> d_fstates;
	DevBuf<float> d_hist;
	DevBuf<uint32_t> d_bitring;
	// frame slots, per-channel frame counts and the demod kernel's framer descriptor exist TWICE: submit number t (1-based) uses
	// slot[(t - 1) & 1], so the frames of submit t stay readable while submit t + 1 is queued or running (sonde_batch_frames_of)
	struct Slot {
		DevBuf<SondeFrame> d_frames;
		DevBuf<uint32_t> d_counts;
		DevBuf<SdFramerOut> d_fo;          // where the demod kernel's in-kernel sync search keeps its state and lists frames (device copy)
		SdFramerOut h_fo = {};             // host copy: the bins decoder takes the descriptor by value (bins_kernel.hip)
		DevEvent ev_done;                  // recorded behind the last kernel of the submit once the host works with tickets
		bool ev_valid = false;             // (an event record is a bubble in the command stream: not paid by hosts that sync every submit)
		bool have_counts = false;          // h_counts, n_frames, n_overflow hold this submit's
		std::vector<uint32_t> h_counts;
		long n_frames = 0, n_overflow = 0;
	} slot[2];
	bool ticketing = false;
	DevEvent ev_xs;                        // orders a submit behind the previous one when the host changes streams
	uint64_t tickets = 0;                  // submits so far
	DevBuf<float> d_taps;
	DevBuf<SdModem> d_modems;
	SdModem h_modems[SONDE_NTYPES] = {};   // host copy: the bins decoder takes the table by value
	DevBuf<uint8_t> d_gfexp, d_gflog, d_g64;      // the FEC tables, and what launchers and kernels take: the view `fec` of them
	DevBuf<uint32_t> d_gfswar;
	DevBuf<uint16_t> d_m10tab;
	SdFecTables fec = {};
	uint32_t fuse_fec = 1;                 // RS41 FEC in the demod kernel's epilogue (default) or as its own kernel (SONDE_FLAG_SPLIT_FEC)
	uint32_t fixed_epi = 1;                // the fixed-length framers' frames decoded in the demod kernel's epilogue too (round 6; not behind a channelizer: bins_kernel.hip)
	DevBuf<uint8_t> d_descs;
	DevBuf<uint32_t> d_chlist[SONDE_NTYPES];
	DevBuf<uint8_t> d_stage;               // sonde_batch_submit_host's device rows
	size_t stage_bytes = 0;
	// AFSK sondes (iMet): tone-demodulator state, mixer table, 6 kS/s scratch rows; the other channels' list for kernel A
	DevBuf<SdAfskState> d_astates;
	DevBuf<float> d_wtab, d_wtab_c50, d_afq;
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
	struct Unit {
		int type, cls; uint32_t off, n; size_t row0;
		uint32_t types;                    // bit t: the frame decoders of sonde type t follow this unit's demod launch
		DevStream st; DevEvent ev_join[2];          // ev_join[submit parity]; created once the units are known (build)
	};
	std::vector<Unit> units;
	DevBuf<uint32_t> d_cls[4];             // joined batches: the channel list of each class
	int n_chunks = 1;
	DevEvent ev_fork;
	// How a submit of several launch units completes (include/sonde_abi.h): 0 (default): the unit streams are joined into the
	// caller's stream before sonde_batch_submit returns; 1 SONDE_FLAG_LATE_JOIN: one submit late -- submit t joins the units of submit
	// t - 1 into the caller's stream, so that a unit's submit t + 1 may start beside the other units' submit t; 2 SONDE_FLAG_PIPELINE:
	// never.  In modes 1 and 2 done_stream collects the unit streams for completion (sonde_batch_sync, tickets).
	int join_mode = 0;
	DevStream done_stream;
	uint32_t granule = SONDE_TILE;         // submit sizes must be a multiple of this
	// one residency of the GPU: the demod workgroups it holds at once, 4 (39.7 KB of LDS, 8 waves each) per CU.  The launch-unit
	// rule, the in-loop FEC bound (SdFramerOut.loop_fec_max_wg) and the time-slice policy all work with it.
	uint32_t residency = 0;
	// time slices (launch.h SdSlice): per-channel segment counters, the value they hold before the next sliced launch and the knob
	// (SondeBatchConfig.time_slices; 0: the library's choice)
	DevBuf<uint32_t> d_prog;
	uint32_t seg_base = 0;
	int seg_force = 0;
	bool sliced_once = false;
	// round 6: a batch of exactly the two default classes -- (4, 8): RS41 / DFM / iMS-100 / MRZ-N1 and (2, 8): M10; BASELINE config 3 --
	// at the default completion mode is ONE launch on the caller's stream (sd_demod_mixed_kernel: the classes interleaved block by
	// block), frame decoders in its epilogue: no fork, no join, no launch units
	bool mixed_one = false;

	SdTiming timing;
	hipStream_t last_stream = nullptr;     // where the last submit completes
	bool pending = false;
	std::vector<SondeFrame> h_slots;
	// sonde_batch_poll: per-channel parsers (created on first use), fragments waiting to be fetched
	std::vector<std::unique_ptr<SondeParser>> parsers;
	std::deque<std::pair<uint32_t, SondeData>> frags;
	uint64_t polled_ticket = 0;            // submits up to this one have been parsed by sonde_batch_poll
	// sonde_batch_restart_channels (SPEC 3.12): the channel lists on their way to the reset kernel, the event that orders the next
	// submit's launch units behind it, and (submits so far, channel): the channel's parser is replaced before a later submit is parsed
	SdChanLists restart_lists;
	DevEvent ev_restart;
	std::deque<std::pair<uint64_t, uint32_t>> parser_restarts;
	bool behind_channelizer = false;
	// the rescue passes (k_rescue_passes): per pass [n_channels][words] of state; null: its flag is off or the batch has no channel of its
	// types, and nothing of it is allocated or launched.  d_mrztab: MRZ-N1's column table, with the Manchester pass or with an MRZ-N1
	// diversity group (sd_batch_need_mrztab)
	DevBuf<uint32_t> d_pass[SD_N_PASSES];
	DevBuf<uint16_t> d_mrztab;
	// sonde_batch_set_diversity (SPEC 3.3j): the group table, per group SD_DIV_MAX carried records and two counters, the slot
	// (SD_DIV_MAX * group + member, or -1) of every channel on both sides; null / empty: the call was never made, and nothing of it is
	// allocated or launched
	// div_mode: sonde_batch_set_diversity_auto's mode (SPEC 3.3k; 0: no align step is launched), div_unlocked: its groups start unlocked;
	// d_divstate: per group the offsets and lock bits the combining pass reads, and the align step's counters
	// div_kinds: a bit per sonde type that has a group (SPEC 3.3l, 3.3m, 3.3n): which of the combining kernels (k_div_passes) are launched
	// div_flags: the create flags a pass may ask for (SdDivPass.flag); div_window: the caller's window, 0: each pass's default
	uint32_t n_groups = 0, div_window = 0, div_mode = 0, div_unlocked = 0, div_kinds = 0, div_flags = 0;
	DevBuf<SdDivGroup> d_groups;
	DevBuf<SdDivState> d_divstate;
	DevBuf<SondeFrame> d_carried;
	DevBuf<uint32_t> d_divcnt;
	DevBuf<int32_t> d_divslot;
	std::vector<int32_t> div_slot;
};
int sd_batch_need_mrztab(SondeBatch *b);      // uploads d_mrztab if it is not there yet (batch.hip); the device is set
static_assert(!std::is_copy_constructible<SondeBatch>::value && !std::is_copy_constructible<SondeBatch::Unit>::value, "owners of device resources");
static_assert(!std::is_copy_constructible<DevBuf<uint8_t>>::value && !std::is_copy_constructible<PinnedBuf<uint32_t>>::value &&
	!std::is_copy_constructible<DevEvent>::value && !std::is_copy_constructible<DevStream>::value, "owners of device resources");
#pragma GCC visibility pop
