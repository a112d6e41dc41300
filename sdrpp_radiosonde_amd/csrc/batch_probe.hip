// batch_probe.hip -- introspection for the staged parity tests and the bench: the RS correctors alone, a channel's state and bits,
// what the rescue pass has learned, a combining pass's rule alone (test_combine), and the HBM read probe.  Not on the product path.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "batch_impl.h"

// What every unit entry below does around its launch, on the device the caller has selected: the cases `in` (n_io elements; null: a
// buffer for results only) and a status of n_st words in device memory, launch(cases, status), the launch's error, and cases and
// status back into out and status.  A HIP call that fails here is reported under the entry's name.
template <typename T, typename Launch>
static int probe_unit(const char *who, const T *in, T *out, size_t n_io, int32_t *status, size_t n_st, Launch launch)
{
	DevBuf<T> d_io;
	DevBuf<int32_t> d_st;
	hipError_t e = in ? d_io.upload(in, n_io) : d_io.alloc(n_io);
	if (e == hipSuccess) e = d_st.alloc(n_st);
	if (e == hipSuccess) { launch((T *)d_io, (int32_t *)d_st); e = hipGetLastError(); }
	if (e == hipSuccess) e = hipMemcpy(out, d_io, n_io * sizeof(T), hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(status, d_st, n_st * sizeof(int32_t), hipMemcpyDeviceToHost);
	return e == hipSuccess ? 0 : sd_fail(who, e);
}

// The RS(255,231) corrector alone: n_pairs codeword pairs of [2][256] bytes (positions >= n zero), corrected in place;
// status[2 * i + c]: 0 clean, > 0 corrected byte errors, -1 uncorrectable (word left as received).
// erased = null: errors only (sd_rsdec.h); else the errors-and-erasures corrector of SONDE_FLAG_RS41_RESCUE (sd_rsee.h), with
// erased[i][c][k] != 0 marking position k.
static int test_rs255(const char *who, SondeBatch *b, uint8_t *cw_pairs, size_t n_pairs, int n, const uint8_t *erased, int32_t *status)
{
	HIPCHK(hipSetDevice(b->device));
	DevBuf<uint8_t> d_er;
	const hipError_t e = erased ? d_er.upload(erased, n_pairs * 512) : hipSuccess;
	if (e != hipSuccess) return sd_fail(who, e);
	return probe_unit(who, cw_pairs, cw_pairs, n_pairs * 512, status, n_pairs * 2, [&](uint8_t *d_cw, int32_t *d_st) {
		if (erased) sd_launch_rsee_unit(d_cw, d_er, (uint32_t)n_pairs, n, d_st, b->fec.gfexp, b->fec.gflog, b->fec.gfswar, nullptr);
		else sd_launch_rs255_unit(d_cw, (uint32_t)n_pairs, n, d_st, b->fec.gfexp, b->fec.gflog, b->fec.gfswar, nullptr);
	});
}

extern "C" int sonde_batch_test_rs255(SondeBatch *b, uint8_t *cw_pairs, size_t n_pairs, int n, int32_t *status)
{
	if (!b || !cw_pairs || !status || !n_pairs || n < 25 || n > 255) return sd_fail("sonde_batch_test_rs255: bad argument");
	return test_rs255("sonde_batch_test_rs255", b, cw_pairs, n_pairs, n, nullptr, status);
}

extern "C" int sonde_batch_test_rs255_erasures(SondeBatch *b, uint8_t *cw_pairs, size_t n_pairs, int n, const uint8_t *erased, int32_t *status)
{
	if (!b || !cw_pairs || !erased || !status || !n_pairs || n < 25 || n > 255) return sd_fail("sonde_batch_test_rs255_erasures: bad argument");
	return test_rs255("sonde_batch_test_rs255_erasures", b, cw_pairs, n_pairs, n, erased, status);
}

// What a rescue pass (k_rescue_passes) has counted on a channel: the last two words of the channel's state
static int rescue_info(SondeBatch *b, int pass, uint32_t channel, uint32_t *tried, uint32_t *rescued)
{
	const SdRescuePass &p = k_rescue_passes[pass];
	const std::string who = std::string(p.info) + ": ";
	if (!b || channel >= b->n_channels) return sd_fail((who + "bad argument").c_str());
	if (b->behind_channelizer) return sd_fail((who + p.flag_name + " is not available for the batch behind a channelizer").c_str());
	if (!b->d_pass[pass]) return sd_fail((who + "the batch was created without " + p.flag_name + " (or has no " + p.kind + " channel)").c_str());
	if (!(p.types >> b->types[channel] & 1u)) return sd_fail((who + "not " + p.article + " " + p.kind + " channel").c_str());
	if (sonde_batch_sync(b) < 0) return -1;
	SdRescueCounters cnt;
	HIPCHK(hipMemcpy(&cnt, b->d_pass[pass] + ((size_t)channel + 1) * p.words - 2, sizeof(cnt), hipMemcpyDeviceToHost));
	if (tried) *tried = cnt.tried;
	if (rescued) *rescued = cnt.rescued;
	return 0;
}

extern "C" int sonde_batch_rescue_info(SondeBatch *b, uint32_t channel, SondeRs41Layout out[2], uint32_t *tried, uint32_t *rescued)
{
	if (rescue_info(b, SD_PASS_RS41, channel, tried, rescued)) return -1;
	const SdRescueState *st = (const SdRescueState *)(uint32_t *)b->d_pass[SD_PASS_RS41] + channel;
	if (out) HIPCHK(hipMemcpy(out, st->lay, sizeof(st->lay), hipMemcpyDeviceToHost));
	return 0;
}
extern "C" int sonde_batch_manchester_rescue_info(SondeBatch *b, uint32_t channel, uint32_t *tried, uint32_t *rescued)
{
	return rescue_info(b, SD_PASS_MANCHESTER, channel, tried, rescued);
}
extern "C" int sonde_batch_dfm_rescue_info(SondeBatch *b, uint32_t channel, uint32_t *tried, uint32_t *rescued)
{
	return rescue_info(b, SD_PASS_DFM, channel, tried, rescued);
}
extern "C" int sonde_batch_ims_rescue_info(SondeBatch *b, uint32_t channel, uint32_t *tried, uint32_t *rescued)
{
	return rescue_info(b, SD_PASS_IMS, channel, tried, rescued);
}
extern "C" int sonde_batch_afsk_rescue_info(SondeBatch *b, uint32_t channel, uint32_t *tried, uint32_t *rescued)
{
	return rescue_info(b, SD_PASS_AFSK, channel, tried, rescued);
}

// Step 4 of SPEC 3.3g alone, through the kernel's own device function: n words and their erasure masks, decoded in place;
// status[i] = bits changed, -1 = no decode (word untouched).
extern "C" int sonde_batch_test_hamming84_erasures(SondeBatch *b, uint8_t *words, const uint8_t *erased, size_t n, int32_t *status)
{
	if (!b || !words || !erased || !status || !n || n > (1u << 24)) return sd_fail("sonde_batch_test_hamming84_erasures: bad argument");
	HIPCHK(hipSetDevice(b->device));
	DevBuf<uint8_t> d_e;
	HIPCHK(d_e.upload(erased, n));
	return probe_unit("sonde_batch_test_hamming84_erasures", words, words, n, status, n,
		[&](uint8_t *d_w, int32_t *d_st) { sd_launch_hamming84_unit(d_w, d_e, (uint32_t)n, d_st, nullptr); });
}

// Step 3 of SPEC 3.3h alone, through the kernel's own device function: n blocks (bit b of the block = bit 45 - b) and the masks of
// their violated boundaries (bit k = boundary k, 0..46), decoded in place; status[i] = bits flipped, -1 = no decode (block untouched).
extern "C" int sonde_batch_test_ims_block(SondeBatch *b, size_t n, uint64_t *blocks, const uint64_t *viol, int32_t *status)
{
	if (!b || !blocks || !viol || !status || !n || n > (1u << 24)) return sd_fail("sonde_batch_test_ims_block: bad argument");
	HIPCHK(hipSetDevice(b->device));
	DevBuf<uint64_t> d_v;
	HIPCHK(d_v.upload(viol, n));
	return probe_unit("sonde_batch_test_ims_block", blocks, blocks, n, status, n,
		[&](uint64_t *d_b, int32_t *d_st) { sd_launch_ims_block_unit(b->fec.g64, d_b, d_v, (uint32_t)n, d_st, nullptr); });
}

// Steps 1..5 of SPEC 3.3i alone, through the kernel's own device function: n caller-made records, rewritten in place where rescued;
// status[i] = 0 untouched (not eligible, or no pattern fits), 1 rescued, 2 several patterns fit (untouched).
extern "C" int sonde_batch_test_afsk_repair(SondeBatch *b, SondeFrame *records, size_t n, int32_t *status)
{
	if (!b || !records || !status || !n || n > (1u << 20)) return sd_fail("sonde_batch_test_afsk_repair: bad argument");
	HIPCHK(hipSetDevice(b->device));
	return probe_unit("sonde_batch_test_afsk_repair", records, records, n, status, n,
		[&](SondeFrame *d_r, int32_t *d_st) { sd_launch_afsk_repair_unit(d_r, (uint32_t)n, d_st, nullptr); });
}

extern "C" int sonde_batch_diversity_info(SondeBatch *b, uint32_t group, uint32_t *tried, uint32_t *combined)
{
	if (!b) return sd_fail("sonde_batch_diversity_info: bad argument");
	if (!b->n_groups) return sd_fail("sonde_batch_diversity_info: sonde_batch_set_diversity was not called");
	if (group >= b->n_groups) return sd_fail("sonde_batch_diversity_info: no such group");
	if (sonde_batch_sync(b) < 0) return -1;
	uint32_t cnt[2];
	HIPCHK(hipMemcpy(cnt, b->d_divcnt + 2 * (size_t)group, sizeof(cnt), hipMemcpyDeviceToHost));
	if (tried) *tried = cnt[0];
	if (combined) *combined = cnt[1];
	return 0;
}

// What the four combine entries below do around their pass's unit kernel (launch.h SdDivUnitArgs), each through the kernel's own device
// function.  An entry: its name, its launcher, the records per case (SD_DIV_MAX copies, copy 0 the record to rewrite; iMS-100: copy
// 0's record alone), the received blocks per case (iMS-100; else 0), and whether the kernel reads MRZ-N1's column table -- one of the
// call's own: the batch stays as it is.  The cases, as the caller gave them: n of them, n_copies[i] = 2..4 copies in use; out[i] =
// copy 0, rewritten or not, status[i] = what the rule answers.  why(c, k) = null, or why the case of the k copies c is refused
struct CombineEntry { const char *who; void (*launch)(const SdDivUnitArgs &); size_t per, per_blocks; bool mrz; };
struct CombineCases { size_t n; const SondeFrame *copies; const uint32_t *n_copies; const uint64_t *blocks; SondeFrame *out; int32_t *status; };
template <typename Why> static int test_combine(const CombineEntry &e, SondeBatch *b, const CombineCases &c, Why why)
{
	const auto fail = [&e](const char *w) { std::string m(e.who); m += ": "; m += w; return sd_fail(m.c_str()); };
	if (!b || !c.copies || !c.n_copies || (e.per_blocks && !c.blocks) || !c.out || !c.status || !c.n || c.n > (1u << 16)) return fail("bad argument");
	for (size_t i = 0; i < c.n; i++) {
		if (c.n_copies[i] < 2 || c.n_copies[i] > SD_DIV_MAX) return fail("n_copies must be 2..4");
		if (const char *w = why(c.copies + e.per * i, c.n_copies[i])) return fail(w);
	}
	HIPCHK(hipSetDevice(b->device));
	DevBuf<SondeFrame> d_c;
	DevBuf<uint32_t> d_n;
	DevBuf<uint64_t> d_b;
	DevBuf<uint16_t> d_mrz;
	if (e.mrz) {
		uint16_t tab[43 * 8];
		fec_mrz_table(tab);
		HIPCHK(d_mrz.upload(tab, 43 * 8));
	}
	HIPCHK(d_c.upload(c.copies, e.per * c.n));
	HIPCHK(d_n.upload(c.n_copies, c.n));
	if (e.per_blocks) HIPCHK(d_b.upload(c.blocks, e.per_blocks * c.n));
	return probe_unit(e.who, (const SondeFrame *)nullptr, c.out, c.n, c.status, c.n, [&](SondeFrame *d_o, int32_t *d_st) {
		e.launch({ d_c, d_n, (uint32_t)c.n, d_o, d_st, b->fec, d_mrz, d_b, nullptr });
	});
}

// Steps 3 to 7 of SPEC 3.3j alone: status[i] = copies used, -1 too many erasures, -2 no decode, -3 rejected.
extern "C" int sonde_batch_test_rs41_combine(SondeBatch *b, size_t n, const SondeFrame *copies, const uint32_t *n_copies, SondeFrame *out, int32_t *status)
{
	return test_combine({ "sonde_batch_test_rs41_combine", sd_launch_diversity_unit, SD_DIV_MAX, 0, false }, b, { n, copies, n_copies, nullptr, out, status },
		[](const SondeFrame *c, uint32_t k) -> const char * {
			if (!sd_div_is_frame(k_div_passes[SD_DIV_RS41], SONDE_RS41, c[0].len) || (c[0].nerr[0] >= 0 && c[0].nerr[1] >= 0))
				return "copy 0 must be a 320- or 518-byte record with a failed codeword";
			for (uint32_t j = 1; j < k; j++)
				if (c[j].len != c[0].len) return "the copies of a case must have one length";
			return nullptr;
		});
}

// Steps 3 to 6 of SPEC 3.3l alone: status[i] = copies used, -1 not attempted, -2 no subset fits, -3 several fit.
extern "C" int sonde_batch_test_check_combine(SondeBatch *b, size_t n, const SondeFrame *copies, const uint32_t *n_copies, SondeFrame *out, int32_t *status)
{
	return test_combine({ "sonde_batch_test_check_combine", sd_launch_check_diversity_unit, SD_DIV_MAX, 0, true }, b, { n, copies, n_copies, nullptr, out, status },
		[](const SondeFrame *c, uint32_t k) -> const char * {
			if (!sd_div_is_frame(k_div_passes[SD_DIV_CHECK], c[0].type, c[0].len) || c[0].nerr[0] >= 0)
				return "copy 0 must be a failed SONDE_M10 record of 101 or 70 bytes or a failed SONDE_MRZN1 record of 45";
			for (uint32_t j = 1; j < k; j++)
				if (c[j].len != c[0].len || c[j].type != c[0].type) return "the copies of a case must have one type and one length";
			return nullptr;
		});
}

// Steps 3 to 6 of SPEC 3.3m alone: status[i] = copies used, -1 the pairing guard refuses, -2 a word has no solution, -3 a word has several.
extern "C" int sonde_batch_test_dfm_combine(SondeBatch *b, size_t n, const SondeFrame *copies, const uint32_t *n_copies, SondeFrame *out, int32_t *status)
{
	return test_combine({ "sonde_batch_test_dfm_combine", sd_launch_dfm_diversity_unit, SD_DIV_MAX, 0, false }, b, { n, copies, n_copies, nullptr, out, status },
		[](const SondeFrame *c, uint32_t k) -> const char * {
			if (c[0].nerr[1] <= 0) return "copy 0 must be a failed record (nerr[1] > 0)";
			for (uint32_t j = 0; j < k; j++)
				if (!sd_div_is_frame(k_div_passes[SD_DIV_DFM], c[j].type, c[j].len)) return "every copy must be a SONDE_DFM09 record of 33 bytes";
			return nullptr;
		});
}

// Steps 4 to 7 of SPEC 3.3n alone: per case copy 0's record and the received blocks of the copies, [SD_DIV_MAX][12]; status[i] = copies
// used, 0 the record's nerr[1] is not what copy 0's blocks say, -1 the pairing guard refuses, -2 a block has no solution, -3 a block
// has several.
extern "C" int sonde_batch_test_ims_combine(SondeBatch *b, size_t n, const SondeFrame *records, const uint32_t *n_copies, const uint64_t *blocks,
	SondeFrame *out, int32_t *status)
{
	return test_combine({ "sonde_batch_test_ims_combine", sd_launch_ims_diversity_unit, 1, SD_DIV_MAX * 12, false }, b, { n, records, n_copies, blocks, out, status },
		[](const SondeFrame *r, uint32_t) -> const char * {
			if (!sd_div_is_frame(k_div_passes[SD_DIV_IMS], r->type, r->len)) return "copy 0 must be a SONDE_IMS100 record of 51 bytes";
			return r->nerr[1] <= 0 ? "copy 0 must be a failed record (nerr[1] > 0)" : nullptr;
		});
}

// Steps 3 to 6 of SPEC 3.3o alone: status[i] = copies used, -1 not attempted, -2 no subset fits, -3 several fit.
extern "C" int sonde_batch_test_afsk_combine(SondeBatch *b, size_t n, const SondeFrame *copies, const uint32_t *n_copies, SondeFrame *out, int32_t *status)
{
	return test_combine({ "sonde_batch_test_afsk_combine", sd_launch_afsk_diversity_unit, SD_DIV_MAX, 0, false }, b, { n, copies, n_copies, nullptr, out, status },
		[](const SondeFrame *c, uint32_t k) -> const char * {
			if ((!sd_div_is_frame(k_div_passes[SD_DIV_IMET], c[0].type, c[0].len) && !sd_div_is_frame(k_div_passes[SD_DIV_C50], c[0].type, c[0].len)) ||
				c[0].nerr[0] >= 0)
				return "copy 0 must be a failed SONDE_IMET4 record of 5 to 64 bytes or a failed SONDE_C50 record of 9";
			for (uint32_t j = 1; j < k; j++)
				if (c[j].len != c[0].len || c[j].type != c[0].type) return "the copies of a case must have one type and one length";
			return nullptr;
		});
}

extern "C" int sonde_batch_diversity_offsets(SondeBatch *b, uint32_t group, int64_t off[4], uint32_t *locked_mask, uint32_t *learned, uint32_t *duplicates)
{
	if (!b) return sd_fail("sonde_batch_diversity_offsets: bad argument");
	if (!b->n_groups) return sd_fail("sonde_batch_diversity_offsets: sonde_batch_set_diversity was not called");
	if (group >= b->n_groups) return sd_fail("sonde_batch_diversity_offsets: no such group");
	if (sonde_batch_sync(b) < 0) return -1;
	if (b->tickets) HIPCHK(hipStreamSynchronize(b->last_stream));      // a restart queued behind the last submit has written the state too
	SdDivState st;
	HIPCHK(hipMemcpy(&st, b->d_divstate + (size_t)group, sizeof(st), hipMemcpyDeviceToHost));
	for (int m = 0; off && m < SD_DIV_MAX; m++) off[m] = st.off[m];
	if (locked_mask) *locked_mask = st.locked;
	if (learned) *learned = st.learned;
	if (duplicates) *duplicates = st.duplicates;
	return 0;
}

// The align step of SPEC 3.3k alone, through the kernel's own device function (include/sonde_abi.h), with the predicates of `kind`
static int test_diversity_align(uint32_t kind, SondeBatch *b, size_t n, size_t max_rec, const uint32_t *n_members, SondeFrame *records, const uint32_t *counts,
	const SondeFrame *carried, int64_t *off, uint32_t *locked, const uint32_t *mode, uint32_t *learned, uint32_t *duplicates)
{
	if (!b || !n_members || !records || !counts || !carried || !off || !locked || !mode || !learned || !duplicates || !n || n > (1u << 12) || !max_rec ||
		max_rec > 1024)
		return sd_fail("sonde_batch_test_diversity_align: bad argument");
	std::vector<SdDivState> st(n);
	for (size_t k = 0; k < n; k++) {
		if (n_members[k] < 2 || n_members[k] > SD_DIV_MAX) return sd_fail("sonde_batch_test_diversity_align: n_members must be 2..4");
		if (mode[k] & ~(SONDE_DIVERSITY_LEARN | SONDE_DIVERSITY_MARK_DUPLICATES)) return sd_fail("sonde_batch_test_diversity_align: unknown mode bits");
		if (locked[k] >> n_members[k]) return sd_fail("sonde_batch_test_diversity_align: a lock bit of a member the case does not have");
		st[k] = SdDivState{};
		for (uint32_t m = 0; m < SD_DIV_MAX; m++) {
			if (counts[SD_DIV_MAX * k + m] > max_rec) return sd_fail("sonde_batch_test_diversity_align: counts > max_rec");
			st[k].off[m] = off[SD_DIV_MAX * k + m];
		}
		st[k].locked = locked[k];
	}
	HIPCHK(hipSetDevice(b->device));
	DevBuf<SondeFrame> d_r, d_c;
	DevBuf<uint32_t> d_cnt, d_nm, d_mode;
	DevBuf<SdDivState> d_st;
	HIPCHK(d_r.upload(records, SD_DIV_MAX * n * max_rec));
	HIPCHK(d_c.upload(carried, SD_DIV_MAX * n));
	HIPCHK(d_cnt.upload(counts, SD_DIV_MAX * n));
	HIPCHK(d_nm.upload(n_members, n));
	HIPCHK(d_mode.upload(mode, n));
	HIPCHK(d_st.upload(st.data(), n));
	sd_launch_diversity_align_unit((uint32_t)n, nullptr, d_r, d_cnt, (uint32_t)max_rec, d_nm, d_c, d_st, d_mode, kind);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(records, d_r, SD_DIV_MAX * n * max_rec * sizeof(SondeFrame), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(st.data(), d_st, n * sizeof(SdDivState), hipMemcpyDeviceToHost));
	for (size_t k = 0; k < n; k++) {
		for (uint32_t m = 0; m < SD_DIV_MAX; m++) off[SD_DIV_MAX * k + m] = st[k].off[m];
		locked[k] = st[k].locked;
		learned[k] = st[k].learned;
		duplicates[k] = st[k].duplicates;
	}
	return 0;
}

extern "C" int sonde_batch_test_diversity_align(SondeBatch *b, size_t n, size_t max_rec, const uint32_t *n_members, SondeFrame *records, const uint32_t *counts,
	const SondeFrame *carried, int64_t *off, uint32_t *locked, const uint32_t *mode, uint32_t *learned, uint32_t *duplicates)
{
	return test_diversity_align(SONDE_RS41, b, n, max_rec, n_members, records, counts, carried, off, locked, mode, learned, duplicates);
}

extern "C" int sonde_batch_test_diversity_align_kind(SondeBatch *b, uint32_t kind, size_t n, size_t max_rec, const uint32_t *n_members, SondeFrame *records,
	const uint32_t *counts, const SondeFrame *carried, int64_t *off, uint32_t *locked, const uint32_t *mode, uint32_t *learned, uint32_t *duplicates)
{
	if (kind != SONDE_RS41 && kind != SONDE_M10 && kind != SONDE_MRZN1 && kind != SONDE_DFM09 && kind != SONDE_IMS100)
		return sd_fail("sonde_batch_test_diversity_align_kind: a kind this entry does not take (iMet groups are tested on scenes, C50 has no align step)");
	return test_diversity_align(kind, b, n, max_rec, n_members, records, counts, carried, off, locked, mode, learned, duplicates);
}

// wait for the last submit and fetch the channel's demodulator state
static int fetch_state(SondeBatch *b, uint32_t channel, SdChanState *st)
{
	if (sonde_batch_sync(b) < 0) return -1;
	HIPCHK(hipMemcpy(st, b->d_states + channel, sizeof(*st), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" uint64_t sonde_batch_nbits(SondeBatch *b, uint32_t channel)
{
	if (!b || channel >= b->n_channels) { sd_fail("sonde_batch_nbits: bad argument"); return 0; }
	SdChanState st;
	return fetch_state(b, channel, &st) ? 0 : st.wpos;
}

extern "C" int sonde_batch_read_bits(SondeBatch *b, uint32_t channel, uint64_t from, size_t count, uint8_t *out)
{
	if (!b || channel >= b->n_channels || !out) return sd_fail("sonde_batch_read_bits: bad argument");
	SdChanState st;
	if (fetch_state(b, channel, &st)) return -1;
	const uint64_t ring_bits = (uint64_t)b->ring_words * 32;
	if (from + count > st.wpos || st.wpos - from > ring_bits) return sd_fail("sonde_batch_read_bits: range not in the ring");
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
	if (!b || channel >= b->n_channels) return sd_fail("sonde_batch_read_state: bad argument");
	SdChanState st;
	if (fetch_state(b, channel, &st)) return -1;
	if (t_next) *t_next = st.t_next;
	if (period) *period = st.period;
	if (bias) *bias = st.bias;
	if (amp) *amp = st.amp;
	if (afc_u) *afc_u = st.afc[2];          // the newest AFC state u (SPEC 3.0b); 0 for real input
	return 0;
}

// ---- read-only streaming probe: the HBM read bandwidth this GPU actually delivers, measured in the same
// process as the bench so that kernel A's GB/s can be quoted against *achievable* as well as against the
// 8 TB/s spec peak (SURVEY.md section 8d asks for both).
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
	if (!d_buf || bytes < 16 || reps < 1 || !gbs_out) return sd_fail("sonde_hbm_read_probe: bad argument");
	DevBuf<uint32_t> sink;
	DevEvent e0, e1;
	HIPCHK(sink.alloc(1));
	HIPCHK(e0.create(hipEventDefault));
	HIPCHK(e1.create(hipEventDefault));
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
	if (err != hipSuccess) return sd_fail("sonde_hbm_read_probe", err);
	*gbs_out = (float)((double)(n16 * 16) / ((double)best * 1e-3) / 1e9);
	return 0;
}
