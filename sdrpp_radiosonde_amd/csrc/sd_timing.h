// sd_timing.h -- the symbol-timing loop of SPEC 3.2 / 3.2b, written once for the two kernels that run it: demod_kernel.hip (one
// workgroup per channel: four round waves evaluate the symbols, the lead wave closes the loop, round wave 1 appends the bits) and
// bins_kernel.hip (one wave per channelizer bin, everything in program order).  Here is the ARITHMETIC both must produce to the bit,
// and the sync search's dispatch by sonde type; who evaluates which symbol, where the partial sums meet and how the words are stored
// stays with each kernel: no function knows either kernel's LDS.  Bit-exactness contract: -ffp-contract=off,
// every fused op an explicit __builtin_fmaf, every cross-lane reduction an integer sum: do not re-associate the expressions below.
#pragma once
#include "sd_wave.h"
#include "sd_fixed.h"

// The symbols of the tile that ends at sample n0 (exclusive): those whose on-time instant leaves the filter (nt taps) and the
// look-ahead slack of SPEC 3.2 inside the samples that have arrived.
__device__ __forceinline__ int sd_tile_symbols(int64_t n0, int nt, int64_t t_next, int period)
{
	const int64_t limit = (((n0 - 1 - nt / 2 - SD_MARGIN) << 16) | 0xFFFF);
	return (t_next <= limit) ? (int)((uint32_t)(limit - t_next) / (uint32_t)period) + 1 : 0;
}

// One symbol's term of the Gardner timing-error detector: y, m = the filter at the on-time and the mid-symbol instant, yprev = y of
// the symbol before.  The caller adds __float2int_rn of it for every active symbol but the first of its 64-group (lane 0 in either
// symbol mapping), which has no predecessor in the wave and carries no term (SPEC 3.2).  (The rounding stays in the caller's
// conditional: done in here, masked or not, the bins kernel's register allocation spills -- profiles/timing_loop_notes.md.)
__device__ __forceinline__ float sd_gardner_term(float y, float m, float yprev, float bias)
{
	const float e = (yprev - y) * (m - bias);
	return sd_clamp(e * 1024.0f, -1.0e6f, 1.0e6f);
}

// One symbol's level as an integer, for the sum of the ones (S1) or of the zeros (S0); decision and sums stay with the caller, as above
__device__ __forceinline__ int sd_level_term(float y) { return __float2int_rn(sd_clamp(y, -8.0f, 8.0f) * 4096.0f); }

// The bit ring's words that a round of K > 0 symbols, appended at bit wpos, writes: lane l takes word (wpos >> 5) + l, if the round
// reaches it (touched); the word sits at `index` of the ring; the lane whose word the next round starts in keeps it as that round's
// `partial`, the bits already in the word wpos points into.  The stores are the caller's.
__device__ __forceinline__ bool sd_ring_touched(int lane, uint64_t wpos, int K) { return (uint32_t)(32 * lane) < ((uint32_t)wpos & 31u) + (uint32_t)K; }
__device__ __forceinline__ uint32_t sd_ring_index(int lane, uint64_t wpos, uint32_t ring_mask) { return ((uint32_t)(wpos >> 5) + (uint32_t)lane) & ring_mask; }
__device__ __forceinline__ uint32_t sd_ring_next_owner(uint64_t wpos, int K) { return (((uint32_t)wpos & 31u) + (uint32_t)K) >> 5; }
// a touched lane's word.  chunk: the round's bits in symbol order, chunk[0] = 0, chunk[1 ..] the ballots, zero-padded; *partial is
// read by lane 0 alone, and only when wpos is not at a word's start (by address: through a reference the compiler reads it -- in
// kernel A an LDS word -- in every lane and masks it afterwards).
__device__ __forceinline__ uint32_t sd_ring_word(const uint32_t *chunk, int lane, uint64_t wpos, const uint32_t *partial)
{
	const uint32_t sh = (uint32_t)wpos & 31u;
	const uint32_t lo = chunk[lane + 1], pvw = chunk[lane];
	uint32_t vv = sh ? ((lo << sh) | (pvw >> (32u - sh))) : lo;
	if (lane == 0 && sh) vv |= *partial & ((1u << sh) - 1u);
	return vv;
}

// The loop update of a round of K > 0 symbols: slicer levels (bias, amp), then the PI loop filter (t_next, period).  E: the detector's
// sum over the n_det <= K symbols that fed it; S1, S0: the level sums of the C1 ones and K - C1 zeros; acquiring: SPEC 3.2b holds for
// this round; half_jump: SPEC 3.6b, the caller saw the eye open at the mid-symbol instants.
__device__ __forceinline__ void sd_loop_update(SdChanState &st, const SdModem &md, int K, int n_det, int E, int S1, int S0, int C1,
	bool acquiring, bool half_jump)
{
	const int C0 = K - C1;
	if (C1 > 0 && C0 > 0) {
		const f32x2 cnt = {(float)C1, (float)C0}, rc = sd_recip2(cnt);
		const float hi = ((float)S1 * rc.x) * (1.0f / 4096.0f);
		const float lo = ((float)S0 * rc.y) * (1.0f / 4096.0f);
		const float c = 0.5f * (hi + lo), a = 0.5f * (hi - lo);
		if (st.nstat == 0) { st.bias = c; st.amp = a; }
		else { st.bias = st.bias + 0.5f * (c - st.bias); st.amp = st.amp + 0.5f * (a - st.amp); }
		if (!(st.amp >= 1.0e-3f)) st.amp = 1.0e-3f;
		st.nstat = 1;
	} else {
		// one-sided round (carrier offset larger than the deviation): no level estimate; move the threshold to the mean of the round
		// so that the next one sees both levels (SPEC 3.2)
		st.bias = ((float)(S1 + S0) * sd_recip((float)K)) * (1.0f / 4096.0f);
	}
	// SPEC 3.2b, acquisition: during a stream's first three tiles the threshold is the mean of the round (the level estimate
	// above is built from the slicer's own decisions: with the carrier 2 kHz off it needs several tiles to find the offset)
	if (acquiring) st.bias = ((float)(S1 + S0) * sd_recip((float)K)) * (1.0f / 4096.0f);
	const f32x2 den = {(float)n_det, st.amp * st.amp}, rd = sd_recip2(den);
	float err = ((float)E * rd.x) * (1.0f / 1024.0f);
	err = sd_clamp(err * rd.y, -1.0f, 1.0f);
	const int dphase = __float2int_rn(err * md.kp), dper = __float2int_rn(err * md.ki);
	st.t_next += (int64_t)K * st.period + dphase;
	// SPEC 3.6b, acquisition aid of the AFSK streams: half a symbol off, the Gardner detector sits on its unstable zero and a loop
	// closed 3-6 times a second takes seconds to leave it; there the mid-symbol samples show the open eye.  Jump half a symbol.
	if (half_jump && st.nstat) st.t_next += st.period >> 1;
	st.period += dper;
	if (st.period < md.pmin) st.period = md.pmin;
	if (st.period > md.pmax) st.period = md.pmax;
}

// K4: one step of a framed channel's sync-search state machine over the bits [.., wp), by sonde type (wave-uniform flags, tested in this
// order: who has ruled the others out passes true for the last, whose class cannot meet a type a constant false).  REG, list: as sd_rs41_sync_step.
template <bool REG>
__device__ __forceinline__ void sd_sync_step_of(bool is_rs41, bool is_dfm, bool is_m10, bool is_ims, bool is_mrz, SdSyncRun &state,
	uint64_t wp, const uint32_t *mirror, int lane, SdFrameDesc *__restrict__ descs_ch, uint32_t max_frames, SdFrameDesc *list = nullptr)
{
	if (is_rs41) sd_rs41_sync_step<REG>(state, wp, mirror, lane, descs_ch, max_frames, list);
	else if (is_dfm) sd_fixed_sync_step<SONDE_DFM09, REG>(state, wp, mirror, lane, descs_ch, max_frames, list);
	else if (is_m10) sd_fixed_sync_step<SONDE_M10, REG>(state, wp, mirror, lane, descs_ch, max_frames, list);
	else if (is_ims) sd_fixed_sync_step<SONDE_IMS100, REG>(state, wp, mirror, lane, descs_ch, max_frames, list);
	else if (is_mrz) sd_fixed_sync_step<SONDE_MRZN1, REG>(state, wp, mirror, lane, descs_ch, max_frames, list);
}
