// launch.h -- host-side launchers of the HIP kernels (one per kernel translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include "sonde_dev.h"
#include "../../include/sonde_abi.h"

// chlist: null = channels 0..n_channels-1 read their own row of `in`; else block i works on channel chlist[i] and reads
// row chlist[i] (compact_in = false: the caller's buffer) or row i (compact_in = true: a per-list scratch buffer)
// decim, nt: the decimation factor (1, 2, 4) and the taps per filter row (8, 16) of EVERY channel this launch works on: (4, 8), (2, 8), (2, 16), (1, 16)
// where the in-kernel sync search of the RS41 channels (sd_rs41.h) keeps its state and lists the complete frames
// and, for the FEC epilogue of the same kernel (sd_rsdec.h), the GF(2^8) tables and the frame slots
struct SdFramerOut {
	SdFramerState *fstates; void *descs; uint32_t *counts; uint32_t max_frames;
	uint32_t fuse_fec;                      // 1: the demod kernel decodes the listed frames in its epilogue; 0: sd_rsdec_rs41_kernel does
	uint32_t loop_fec_max_wg;               // launches of at most this many workgroups (= one residency of the GPU) and >= 48 tiles decode clean
	                                        // RS41 frames inside the tile loop (sd_rsdec.h sd_rs41_loop_step); 0: never
	const uint8_t *gf_exp, *gf_log; const uint32_t *gf_swar;
	const uint8_t *gf64;                    // GF(2^6) tables of the iMS-100 BCH decoder
	SondeFrame *frames;
	const uint16_t *m10tab;                 // Meteomodem checksum matrix rows [99][8] (sd_fixed.h sd_m10_decode_frame)
	uint32_t fixed_epi;                     // 1: the demod kernel also decodes the frames of the fixed-length framers (DFM / M10 / iMS-100 / MRZ-N1) in its
	                                        // epilogue, one frame per wave, like RS41's; 0: sd_dec_fixed_kernel does, one launch more per type
};
// TIME SLICES (round 6).  A demod workgroup lives for its channel's whole submit, so a launch whose workgroup count is not a multiple of
// one residency of the GPU ends with a part-filled generation running alone, and any launch ends with a ramp-down as long as a
// workgroup's life.  With n_seg > 1 a channel's submit is cut into n_seg consecutive SEGMENTS of seg_tiles tiles, each its own
// workgroup: grid = n_wg * n_seg, block b works on segment b / n_wg of list entry b % n_wg (segment-major: every channel's first
// segment is dispatched before any second one).  A segment is what a submit is to the arithmetic -- the channel's whole state is
// carried in HBM, the SPEC does not see where a submit is cut (tests: ragged submits) -- so the frames are those of the unsliced
// launch, bit for bit.  Segment s of a channel waits (one lane polls an agent-scope word, the others sit at a barrier) until segment
// s - 1 has published prog[channel] = seg_base + s; the predecessor has a lower block index, so it was dispatched earlier and is
// running or done: no deadlock as long as workgroups are dispatched in index order per XCD.  Should that ever not hold, the poll
// gives up after ~0.3 s, sets prog[err_index] and the workgroup leaves without touching the channel: the host reports it (never a hang).
struct SdSlice {
	int32_t   n_seg;        // segments per channel (1: unsliced: the fields below are not read)
	int32_t   seg_tiles;    // tiles per segment (the last one takes what is left)
	uint32_t  n_wg;         // list entries (channels) of the launch
	uint32_t  seg_base;     // prog[channel] == seg_base when the launch starts (the host advances it by n_seg per sliced launch)
	uint32_t *prog;         // [n_channels of the batch + 1]: per channel the segments completed so far; the last word: poll gave up
	uint32_t  err_index;    // = n_channels of the batch
};
// which launches have a time-sliced instantiation (the two default classes, IQ input of every kind); the host asks before it slices
bool sd_slices_supported(int in_kind, int decim, int nt);
// in_kind: what the 48 kS/s rows hold (SONDE_INPUT_*, sd_input.h)
void sd_launch_demod(int in_kind, int decim, int nt, uint32_t n_channels, hipStream_t stream,
	const float *in, size_t ch_stride, int n_tiles, SdChanState *states, float *hist,
	uint32_t *bitring, uint32_t ring_words, const float *taps_all, const SdModem *modems,
	const uint32_t *chlist, bool compact_in, const SdFramerOut *fo /* DEVICE memory: the kernel reads it on demand */,
	int utype /* >= 0: every channel of the launch is of this sonde type (taps / modem loads need not wait for the state); -1: per channel */,
	const SdSlice *slice = nullptr /* null or n_seg <= 1: one workgroup per channel for the whole submit */);
// One launch over the channels of the two default classes: list_a = the (4, 8) class's channels (RS41, DFM, iMS-100, MRZ-N1), list_b = the
// (2, 8) class's (M10); utype_x >= 0: every channel of that list is of this sonde type (demod_kernel.hip sd_demod_mixed_kernel)
void sd_launch_demod_mixed(int in_kind, uint32_t n_a, const uint32_t *list_a, int utype_a, uint32_t n_b, const uint32_t *list_b, int utype_b, hipStream_t stream,
	const float *in, size_t ch_stride, int n_tiles, SdChanState *states, float *hist, uint32_t *bitring, uint32_t ring_words,
	const float *taps_all, const SdModem *modems, const SdFramerOut *fo /* DEVICE memory */);
// The decoder behind the filter bank (bins_kernel.hip): one wave per bin; rows of 16-bit phases [16 carried | n_steps]; the last 16
// phases of the submit go to the head of carry_rows' rows (the buffer the next submit reads: the same one unless double-buffered)
struct SdBinsArgs { const int16_t *phases; size_t row_stride; int16_t *carry_rows; size_t carry_stride; const float *g_comp /* [3][SD_RS_KT_LD], device */; };
void sd_launch_bins(uint32_t n_channels, hipStream_t stream, const int16_t *phases, size_t row_stride, int n_blocks,
	int16_t *carry_rows, size_t carry_stride, SdChanState *states, float *hist, uint32_t *bitring, uint32_t ring_words,
	const float *taps_all, const SdModem *modems_host /* [SONDE_NTYPES], HOST memory: passed by value */, const SdFramerOut *fo_host /* HOST copy: by value */,
	const float *g_comp, int utype /* >= 0: every bin is of this sonde type; -1: per bin */);
// the batch object behind a channelizer takes its input as phase rows (channelizer.hip): 3 tiles per 2560 phase samples
int sd_batch_submit_bins(SondeBatch *b, const SdBinsArgs *ba, size_t n_steps, void *stream);
void sd_batch_mark_channelizer(SondeBatch *b);      // sonde_batch_restart_channels refuses such a batch (the bins' carried phases are the channelizer's)
int sd_batch_bins_capable(const SondeBatch *b);      // 1: every channel's class has a bins instantiation (no AFSK sonde, no class without one)

void sd_launch_afsk(int type /* SONDE_IMET4 or SONDE_C50 */, int kind /* SONDE_INPUT_* */, uint32_t n_list, hipStream_t stream, const float *in, size_t ch_stride, int n_tiles,
	const uint32_t *chlist, SdAfskState *astates, const float *wtab, float *out, size_t out_stride);
void sd_launch_framer_imet(uint32_t n_list, hipStream_t stream, const SdChanState *states, SdFramerState *fstates,
	const uint32_t *bitring, uint32_t ring_words, SondeFrame *frames, uint32_t *counts, uint32_t max_frames, const uint32_t *chlist);
void sd_launch_framer_c50(uint32_t n_list, hipStream_t stream, const SdChanState *states, SdFramerState *fstates,
	const uint32_t *bitring, uint32_t ring_words, SondeFrame *frames, uint32_t *counts, uint32_t max_frames, const uint32_t *chlist);

#define SD_DESC_BYTES 16   // sizeof(SdFrameDesc)
void sd_launch_framer_rs41(uint32_t n_list, hipStream_t stream, const uint32_t *bitring, uint32_t ring_words,
	const uint8_t *gf_exp, const uint8_t *gf_log, const uint32_t *gf_swar, const void *descs,
	SondeFrame *frames, const uint32_t *counts, uint32_t max_frames, uint32_t grid_frames, const uint32_t *chlist);

void sd_launch_framer_other(int type, uint32_t n_list, hipStream_t stream,
	const SdChanState *states, SdFramerState *fstates, const uint32_t *bitring, uint32_t ring_words,
	const uint8_t *g64, void *descs, SondeFrame *frames, uint32_t *counts, uint32_t max_frames, uint32_t grid_frames, const uint32_t *chlist,
	bool with_sync /* false: the demod kernel has listed the frames already */);

// parity-test introspection: the RS(255,231) corrector on caller-supplied codeword pairs ([n_pairs][2][256] bytes, device memory)
void sd_launch_rs255_unit(uint8_t *cw_io, uint32_t n_pairs, int n, int32_t *status, const uint8_t *gf_exp, const uint8_t *gf_log,
	const uint32_t *gf_swar, hipStream_t stream);

// The FEC tables of the frame decoders (sd_tables.h), each its own allocation
struct SdFecTables {
	uint8_t *gfexp;                        // zero-absorbing antilog table of the RS decoder (GF_EXP2 in framer_kernel.hip)
	uint8_t *gflog;                        // 256 x u16 logarithms, log 0 = 768
	uint32_t *gfswar;                      // byte-slice tables of the 24 syndrome multipliers alpha^(4j), framer_kernel.hip
	uint8_t *g64;                          // GF(2^6): iMS-100's BCH(63,51); exp[128], log[64]
	uint16_t *m10tab;                      // Meteomodem checksum as a GF(2) matrix product: rows A^k B, sd_fixed.h
};

// THE RESCUE PASSES (DESIGN "what a rescue pass plugs into"): opt-in second passes over a submit's frame records, each behind the
// frame decoders of its sonde types on their stream.  Every pass carries per channel two counters from submit to submit -- records
// that reached its decoder, records rescued -- as the LAST two words of its state; RS41's state has its learned block layouts of the
// two frame lengths (320, 518) in front of them, the other four have nothing else.
struct SdRescueCounters { uint32_t tried, rescued; };
struct SdRescueState { SondeRs41Layout lay[2]; uint32_t tried, rescued; };
// what a pass launcher may need; each picks what its kernel takes
struct SdRescueArgs {
	uint32_t n_list; hipStream_t stream;
	SdFecTables fec;
	const uint16_t *mrztab;                // MRZ-N1's column table (SONDE_FLAG_MANCHESTER_RESCUE only, else null)
	const SdChanState *chan_states; const uint32_t *bitring; uint32_t ring_words;
	SondeFrame *frames; const uint32_t *counts; uint32_t max_frames;
	const uint32_t *chlist;                // null (RS41 only): channels 0..n_list-1
	void *states;                          // [n_channels] of the pass's state
};
void sd_launch_rescue_rs41(const SdRescueArgs &a);            // SONDE_FLAG_RS41_RESCUE (rescue_kernel.hip, DESIGN SPEC 3.3c)
void sd_launch_rescue_manchester(const SdRescueArgs &a);      // SONDE_FLAG_MANCHESTER_RESCUE (check_rescue_kernel.hip, 3.3f): M10 / M20 / MRZ-N1
void sd_launch_rescue_dfm(const SdRescueArgs &a);             // SONDE_FLAG_DFM_RESCUE (dfm_rescue_kernel.hip, 3.3g)
void sd_launch_rescue_ims(const SdRescueArgs &a);             // SONDE_FLAG_IMS_RESCUE (ims_rescue_kernel.hip, 3.3h)
void sd_launch_rescue_afsk(const SdRescueArgs &a);            // SONDE_FLAG_AFSK_RESCUE (afsk_rescue_kernel.hip, 3.3i): iMet / C50
// test introspection, each a step of its pass alone over caller-made cases (device memory), in place:
// the errors-and-erasures corrector of 3.3c on codeword pairs
void sd_launch_rsee_unit(uint8_t *cw_io, const uint8_t *erased, uint32_t n_pairs, int n, int32_t *status, const uint8_t *gf_exp, const uint8_t *gf_log,
	const uint32_t *gf_swar, hipStream_t stream);
// step 4 of 3.3g: n words and their erasure masks; status = bits changed, -1 = no decode
void sd_launch_hamming84_unit(uint8_t *words, const uint8_t *erased, uint32_t n, int32_t *status, hipStream_t stream);
// step 3 of 3.3h: n blocks and the masks of their violated boundaries; status = bits flipped, -1 = no decode
void sd_launch_ims_block_unit(const uint8_t *g64, uint64_t *blocks, const uint64_t *viols, uint32_t n, int32_t *status, hipStream_t stream);
// steps 1..5 of 3.3i: n records; status = 0 untouched, 1 rescued, 2 several patterns fit
void sd_launch_afsk_repair_unit(SondeFrame *records, uint32_t n, int32_t *status, hipStream_t stream);

// sonde_batch_set_diversity (DESIGN SPEC 3.3j, 3.3l, 3.3m, 3.3n, 3.3o): a group = 2..4 channels of one type that hear the same sonde; ch[m] and
// off[m] (offset_bits) per member, kind = the members' type: SONDE_RS41 (0: diversity_kernel.hip), SONDE_M10 or SONDE_MRZN1
// (check_diversity_kernel.hip), SONDE_DFM09 (dfm_diversity_kernel.hip), SONDE_IMS100 (ims_diversity_kernel.hip; SONDE_FLAG_IMS_DIVERSITY), SONDE_IMET4 or SONDE_C50 (afsk_diversity_kernel.hip; SONDE_FLAG_AFSK_DIVERSITY).  Each combining kernel (one row of k_div_passes, batch_impl.h) is launched over the whole table and takes the groups of its kinds; the align
// step, the carried records, the counters and the state are one space for all kinds.  carried: [n_groups][SD_DIV_MAX] records
// (len = 0: none), counters: [n_groups][2] (tried, combined); both carried from submit to submit.  The launches stand behind every
// other kernel of the submit.
#define SD_DIV_MAX 4
struct SdDivGroup { uint32_t n; uint32_t ch[SD_DIV_MAX]; uint32_t kind; int64_t off[SD_DIV_MAX]; };
// What the align step (diversity_align_kernel.hip, DESIGN SPEC 3.3k) carries per group from submit to submit and the combining pass
// reads: off[m] = where member m's bit count stands on the group's clock (SdDivGroup.off is its initial value), locked = a bit per
// member (an unlocked member is to the combining pass a member without records), learned / duplicates = the step's counters.  Without
// the step (mode 0) off is the host's and every member is locked, for good.
struct SdDivState { int64_t off[SD_DIV_MAX]; uint32_t locked, learned, duplicates, pad; };
// THE COMBINING PASSES (DESIGN "what a combining pass plugs into"; batch_impl.h k_div_passes): what a launcher may need; each picks
// what its kernel takes
struct SdDivArgs {
	uint32_t n_groups; hipStream_t stream;
	const SdDivGroup *groups; SdDivState *states; SondeFrame *carried; uint32_t *counters;
	uint32_t window;                       // of the pass that is launched: the caller's, or the pass's default
	uint32_t kinds;                        // of the pass that is launched (SdDivPass.kinds): a launcher of several rows tells them apart by it
	uint32_t other_kinds;                  // the table has groups that are not RS41: the RS41 kernels read the kind word
	SondeFrame *frames; const uint32_t *counts; uint32_t max_frames;
	SdFecTables fec;
	const uint16_t *mrztab;                // MRZ-N1's column table (null: the table has no MRZ-N1 group)
	const SdChanState *chan_states; const uint32_t *bitring; uint32_t ring_words;      // iMS-100 reads the copies' blocks from the chips
};
void sd_launch_diversity(const SdDivArgs &a);                 // RS41 (diversity_kernel.hip, DESIGN SPEC 3.3j)
void sd_launch_check_diversity(const SdDivArgs &a);           // M10 / M20 / MRZ-N1 (check_diversity_kernel.hip, 3.3l)
void sd_launch_dfm_diversity(const SdDivArgs &a);             // DFM (dfm_diversity_kernel.hip, 3.3m)
void sd_launch_ims_diversity(const SdDivArgs &a);             // iMS-100, SONDE_FLAG_IMS_DIVERSITY (ims_diversity_kernel.hip, 3.3n)
void sd_launch_afsk_diversity(const SdDivArgs &a);            // iMet or C50 (a.kinds), SONDE_FLAG_AFSK_DIVERSITY (afsk_diversity_kernel.hip, 3.3o)
// the align step, one launch in front of the passes when mode != 0 (SONDE_DIVERSITY_LEARN | SONDE_DIVERSITY_MARK_DUPLICATES)
void sd_launch_diversity_align(const SdDivArgs &a, uint32_t mode);
// the groups of the listed channels back to "no carried record, counters zero, offsets and locks as set_diversity left them"
// (unlocked_start: the members of a group start unlocked); slot_of[channel] = SD_DIV_MAX * group + member or -1
void sd_launch_diversity_clear(uint32_t n, hipStream_t stream, const uint32_t *list, const int32_t *slot_of, SondeFrame *carried, uint32_t *counters,
	const SdDivGroup *groups, SdDivState *states, uint32_t unlocked_start);
// the align step alone: n cases of SD_DIV_MAX members with max_rec record slots each (records[(4 k + m) * max_rec + i], counts[4 k + m]
// in use, n_members[k] = 2..4), carried[4 k + m] (len 0: none), states[k] in and out, modes[k]; all device memory.  kind: the sonde type
// whose predicates the step uses (SdDivGroup.kind)
void sd_launch_diversity_align_unit(uint32_t n, hipStream_t stream, SondeFrame *records, const uint32_t *counts, uint32_t max_rec,
	const uint32_t *n_members, const SondeFrame *carried, SdDivState *states, const uint32_t *modes, uint32_t kind);
// A pass's rule alone (the steps behind 1 and 2): n cases of SD_DIV_MAX copies each (device memory; n_copies[i] of them in use, copy 0
// the record to rewrite); out[i] = copy 0, rewritten or not; status[i] = copies used, or what the rule answers: RS41 -1 too many
// erasures, -2 no decode, -3 rejected; check and AFSK -1 not attempted, -2 none fits, -3 several fit; DFM and iMS-100 -1 the pairing guard
// refuses, -2 a word / block has no solution, -3 one has several.  iMS-100: copies = n records (copy 0's alone), blocks = the copies'
// received blocks [n][SD_DIV_MAX][12]; status 0 = the record's nerr[1] is not what copy 0's blocks say
struct SdDivUnitArgs {
	const SondeFrame *copies; const uint32_t *n_copies; uint32_t n; SondeFrame *out; int32_t *status;
	SdFecTables fec; const uint16_t *mrztab; const uint64_t *blocks; hipStream_t stream;
};
void sd_launch_diversity_unit(const SdDivUnitArgs &a);
void sd_launch_check_diversity_unit(const SdDivUnitArgs &a);
void sd_launch_dfm_diversity_unit(const SdDivUnitArgs &a);
void sd_launch_ims_diversity_unit(const SdDivUnitArgs &a);
void sd_launch_afsk_diversity_unit(const SdDivUnitArgs &a);

// sets the text sonde_last_error() returns; returns -1 (sd_host.cpp)
int sd_fail(const char *what, hipError_t e = hipSuccess);
