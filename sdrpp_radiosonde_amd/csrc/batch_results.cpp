// batch_results.cpp -- what a host reads back from a SondeBatch (batch_impl.h): completion and tickets, frames, parsed fragments
// (sonde_batch_poll) and the kernel timings.  No kernel is launched here.
#include <string.h>
#include <algorithm>
#include "batch_impl.h"

// wait for submit number `ticket` (1-based) and read its per-channel frame counts; -1 if its slot set has been reused
static long sync_ticket(SondeBatch *b, uint64_t ticket)
{
	if (ticket == 0 || ticket > b->tickets) return sd_fail("sonde_batch: no such submit");
	if (b->tickets - ticket >= 2) return sd_fail("sonde_batch: the frames of that submit have been overwritten (two newer submits)");
	if (hipSetDevice(b->device) != hipSuccess) return sd_fail("hipSetDevice");
	SondeBatch::Slot &s = b->slot[(ticket - 1) & 1];
	if (!s.have_counts) {
		// with an event: wait for that submit only; without (the host did not ask for tickets before it): for the stream
		hipError_t e = s.ev_valid ? hipEventSynchronize(s.ev_done) : hipStreamSynchronize(b->last_stream);
		if (e != hipSuccess) return sd_fail("hipEventSynchronize", e);
		if (ticket == b->tickets || !s.ev_valid) b->pending = false;
		e = hipMemcpy(s.h_counts.data(), s.d_counts, b->n_channels * sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return sd_fail("hipMemcpy counts", e);
		if (b->sliced_once) {      // time slices: a workgroup whose predecessor never published gave up instead of hanging (launch.h SdSlice)
			uint32_t gave_up = 0;
			e = hipMemcpy(&gave_up, b->d_prog + b->n_channels, sizeof(uint32_t), hipMemcpyDeviceToHost);
			if (e != hipSuccess) return sd_fail("hipMemcpy prog", e);
			if (gave_up) return sd_fail("sonde_batch: a time-sliced demod launch found a segment whose predecessor never finished (workgroup dispatch out of order?); the batch's state is undefined -- recreate it");
		}
		long n = 0, over = 0;
		for (uint32_t c = 0; c < b->n_channels; c++) {
			n += std::min(s.h_counts[c], b->max_frames);
			if (s.h_counts[c] > b->max_frames) over += s.h_counts[c] - b->max_frames;
		}
		s.n_frames = n;
		s.n_overflow = over;
		s.have_counts = true;
	}
	return s.n_frames;
}

extern "C" long sonde_batch_sync(SondeBatch *b)
{
	if (!b) return sd_fail("sonde_batch_sync: null argument");
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
	if (!b) return sd_fail("sonde_batch_overflow: null argument");
	if (b->tickets == 0) return 0;
	if (sync_ticket(b, b->tickets) < 0) return -1;
	return b->slot[(b->tickets - 1) & 1].n_overflow;
}

extern "C" long sonde_batch_frames_of(SondeBatch *b, uint64_t ticket, SondeFrame *out, size_t cap)
{
	if (!b) return sd_fail("sonde_batch_frames_of: null argument");
	const long n = sync_ticket(b, ticket);
	if (n < 0) return n;
	if (!out || cap == 0) return n;          // count only: size the buffer from it
	if (n == 0) return 0;
	const SondeBatch::Slot &s = b->slot[(ticket - 1) & 1];
	// frames sit in per-channel slot groups (ordered by channel, then time): one bulk copy of the slot
	// array when it is small, else one copy per channel that has frames
	size_t k = 0;
	const size_t all = (size_t)b->n_channels * b->max_frames;
	if (all * sizeof(SondeFrame) <= (64u << 20)) {
		b->h_slots.resize(all);
		hipError_t e = hipMemcpy(b->h_slots.data(), s.d_frames, all * sizeof(SondeFrame), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return sd_fail("hipMemcpy frames", e);
		for (uint32_t c = 0; c < b->n_channels && k < cap; c++) {
			const uint32_t cnt = std::min(s.h_counts[c], b->max_frames);
			const size_t take = std::min((size_t)cnt, cap - k);
			if (take) memcpy(out + k, b->h_slots.data() + (size_t)c * b->max_frames, take * sizeof(SondeFrame));
			k += take;
		}
		return (long)k;
	}
	for (uint32_t c = 0; c < b->n_channels && k < cap; c++) {
		const uint32_t cnt = std::min(s.h_counts[c], b->max_frames);
		if (!cnt) continue;
		const size_t take = std::min((size_t)cnt, cap - k);
		hipError_t e = hipMemcpy(out + k, s.d_frames + (size_t)c * b->max_frames, take * sizeof(SondeFrame), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return sd_fail("hipMemcpy frames", e);
		k += take;
	}
	return (long)k;
}

extern "C" long sonde_batch_frames(SondeBatch *b, SondeFrame *out, size_t cap)
{
	if (!b) return sd_fail("sonde_batch_frames: null argument");
	if (b->tickets == 0) return 0;
	return sonde_batch_frames_of(b, b->tickets, out, cap);
}

extern "C" long sonde_batch_poll(SondeBatch *b, SondeData *out, uint32_t *channel, size_t cap)
{
	if (!b || !out || !channel) return sd_fail("sonde_batch_poll: null argument");
	// every submit since the last poll that is still resident (frame slots exist twice): a pipelined host may have queued
	// submit t + 1 before it polls; the per-channel parsers are stateful (RS41 calibration, DFM date, C50 position), so a
	// skipped submit would not only lose its own fragments
	while (b->polled_ticket < b->tickets) {
		const uint64_t t = b->polled_ticket + 1;
		if (b->tickets - t >= 2) {
			b->polled_ticket = b->tickets - 2;     // resume with what is left, but say so
			return sd_fail("sonde_batch_poll: the frames of an unpolled submit have been overwritten (poll at least every second submit)");
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
			b->parsers[c]->feed(fr[(size_t)i], v);      // a duplicate too: the parser's calibration state keeps learning
			if (fr[(size_t)i].flags & SONDE_FRAME_DUPLICATE) continue;      // SPEC 3.3k: another receiver of the group has delivered this frame
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

// ---------------------------------------------------------------- timing (SdTiming)
extern "C" int sonde_batch_kernel_ms(SondeBatch *b, float *demod_ms, float *framer_ms)
{
	if (!b) return sd_fail("sonde_batch_kernel_ms: null argument");
	if (sonde_batch_sync(b) < 0) return -1;
	SdTiming &tm = b->timing;
	float a = 0.0f, c = 0.0f;
	const int n = std::min(tm.used, (int)SdTiming::kSlots);
	if (n == 0) return sd_fail("sonde_batch_kernel_ms: no timed submit since the last query (sonde_batch_set_timing)");
	for (int i = 0; i < n; i++) {
		const SdTiming::Submit &s = tm.submit[(size_t)i];
		float x = 0.0f, y = 0.0f;
		HIPCHK(hipEventElapsedTime(&x, s.ev[0], s.ev[1]));
		if (s.has_framer) HIPCHK(hipEventElapsedTime(&y, s.ev[1], s.ev[2]));
		a += x; c += y;
	}
	a /= (float)n; c /= (float)n;
	tm.used = 0;
	if (demod_ms) *demod_ms = a;
	if (framer_ms) *framer_ms = c;
	return 0;
}

extern "C" int sonde_batch_set_timing(SondeBatch *b, int every_n)
{
	if (!b || every_n < 0) return sd_fail("sonde_batch_set_timing: bad argument");
	if (sonde_batch_sync(b) < 0) return -1;
	b->timing.every = every_n;
	b->timing.n_submits = 0;
	b->timing.used = 0;
	b->timing.unit_used = 0;
	return 0;
}

// Mixed batches: average device time (ms) of each demodulator class's kernel alone over the timed submits since the last
// call / sonde_batch_set_timing; class index: 0 (decimation 1, 16 taps), 1 (2, 16), 2 (4, 8), 3 (2, 8); -1: class not in the
// batch.  Returns the number of timed submits averaged (0: the batch is one launch -- use sonde_batch_kernel_ms).
extern "C" int sonde_batch_class_ms(SondeBatch *b, float out[4])
{
	if (!b || !out) return sd_fail("sonde_batch_class_ms: null argument");
	for (int k = 0; k < 4; k++) out[k] = -1.0f;
	if (b->units.empty()) return 0;
	if (sonde_batch_sync(b) < 0) return -1;
	SdTiming &tm = b->timing;
	const int n = std::min(tm.unit_used, (int)SdTiming::kSlots);
	const size_t nu = b->units.size();
	for (int k = 0; k < 4 && n > 0; k++) {
		float acc = 0.0f;
		int cnt = 0;
		for (size_t ui = 0; ui < nu; ui++) {
			const SondeBatch::Unit &u = b->units[ui];
			if (u.type == SONDE_IMET4 || u.type == SONDE_C50 || u.cls != k) continue;
			for (int i = 0; i < n; i++) {
				const DevEvent *ec = tm.unit_pair(nu, i, ui);
				float x = 0.0f;
				HIPCHK(hipEventElapsedTime(&x, ec[0], ec[1]));
				acc += x;
				cnt++;
			}
		}
		if (cnt) out[k] = acc / (float)cnt;
	}
	tm.unit_used = 0;
	return n;
}
