// sd_tables.cpp -- the modem table, tap / mixer generators and FEC tables of sd_tables.h, and the entry points that hand them out.
#include <math.h>
#include <string.h>
#include <algorithm>
#include "sd_tables.h"
#include "sd_host.h"
#include "sd_input.h"      // sd_sample_bytes: the one definition of the sample sizes

// ---------------------------------------------------------------- modem table (SPEC)
// Symbol (chip) rates: SURVEY.md Appendix B; the VFO bandwidths of /root/reference/src/main.hpp:44-52
// bound them from above.
const ModemDef k_modems[SONDE_NTYPES] = {
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

void modem_table(uint32_t flags, int input_kind, ModemDef out[SONDE_NTYPES])
{
	for (int t = 0; t < SONDE_NTYPES; t++) out[t] = k_modems[t];
	if (!(flags & (SONDE_FLAG_WIDE | SONDE_FLAG_WIDE_AUTO)) || input_kind == SONDE_INPUT_REAL) return;
	for (int t = 0; t < SONDE_NTYPES; t++) {
		// SONDE_FLAG_WIDE: every GFSK sonde; SONDE_FLAG_WIDE_AUTO: the types whose channel is 20 kHz or wider in the reference
		// (iMS-100 / RS-11G, MRZ-N1: 20 kHz, M10 / M20: 50 kHz, /root/reference/src/main.hpp:47-51) -- per type, for mixed batches
		const bool wide_type = (flags & SONDE_FLAG_WIDE) || t == SONDE_IMS100 || t == SONDE_MRZN1 || t == SONDE_M10;
		if (out[t].pre == 1 && wide_type) out[t].decim /= 2;       // one decimation step less (SPEC 3.0)
	}
}

int modem_div(const ModemDef *md, int type) { return md[type].decim * md[type].pre; }
int32_t modem_period0(const ModemDef *md, int type) { return (int32_t)llrint(65536.0 * ((double)SD_FS / modem_div(md, type)) / md[type].baud); }
int modem_nt(const ModemDef *md, int type) { return SD_NT_OF(modem_period0(md, type), md[type].pre); }
const int k_cls_decim[4] = { 1, 2, 4, 2 }, k_cls_nt[4] = { 16, 16, 8, 8 };
int modem_class(const ModemDef *md, int type)
{
	const int d = md[type].decim, nt = modem_nt(md, type);
	for (int k = 0; k < 4; k++) if (k_cls_decim[k] == d && k_cls_nt[k] == nt) return k;
	return -1;
}

uint64_t bits_per_submit(const ModemDef *md, int type, uint32_t max_samples)
{
	const int32_t p = modem_period0(md, type) - (modem_period0(md, type) >> 8);      // fastest symbol clock the loop allows
	return ((uint64_t)(max_samples / modem_div(md, type)) << 16) / (uint64_t)p + 2;
}

void modem_fill(const ModemDef *md, SdModem out[SONDE_NTYPES])
{
	for (int t = 0; t < SONDE_NTYPES; t++) {
		const int32_t p0 = modem_period0(md, t);
		out[t].period0 = p0;
		out[t].kp = (float)p0 * 0.159154943f;       // half of 1/pi symbol per unit error
		out[t].ki = out[t].kp * (1.0f / 4096.0f);
		out[t].pmin = p0 - (p0 >> 8);
		out[t].pmax = p0 + (p0 >> 8);
		out[t].decim = md[t].decim;
		out[t].itile = SD_TILE / md[t].decim;      // AFSK: kernel A sees the 6 kS/s stream as plain real input
		out[t].nt = modem_nt(md, t);
		const int rmax = SD_ROUND_MAX * SD_ROUND_SPL(out[t].decim, out[t].nt);
		out[t].rounds = (int32_t)(((((int64_t)out[t].itile << 16) / out[t].pmin) + 2 + rmax - 1) / rmax);   // 1; 2: C50
	}
}

void make_taps(const ModemDef *md, int type, float *out /* [32][32] */)
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
	if (!out) return sd_fail_msg("sonde_get_afsk_table: null argument");
	make_mixer(out, 17, SD_AF_PER);         // iMet: 1700 Hz
	return 0;
}

extern "C" int sonde_get_taps(int type, float *out)
{
	if (type < 0 || type >= SONDE_NTYPES || !out) return sd_fail_msg("sonde_get_taps: bad argument");
	make_taps(k_modems, type, out);
	return 0;
}

// ---------------------------------------------------------------- FEC tables
// GF(2^8), primitive polynomial 0x11D: antilog (twice the period, so that a sum of two logs needs no reduction) and log
static void gf256(uint8_t gexp[512], uint8_t glog[256])
{
	int x = 1;
	memset(glog, 0, 256);
	for (int i = 0; i < 255; i++) { gexp[i] = (uint8_t)x; glog[x] = (uint8_t)i; x <<= 1; if (x & 0x100) x ^= 0x11D; }
	for (int i = 255; i < 512; i++) gexp[i] = gexp[i - 255];
}

void fec_gf256_tables(uint8_t exp2[SD_GFEXP_BYTES], uint16_t log2[256])
{
	uint8_t gexp[512], glog[256];
	gf256(gexp, glog);
	memset(exp2, 0, SD_GFEXP_BYTES);
	for (int i = 0; i < 768; i++) exp2[i] = gexp[i % 255];
	for (int v = 0; v < 256; v++) log2[v] = v ? (uint16_t)glog[v] : (uint16_t)768;
}

void fec_gf256_swar(uint32_t sw[24 * 8])
{
	uint8_t gexp[512], glog[256];
	gf256(gexp, glog);
	memset(sw, 0, 24 * 8 * sizeof(uint32_t));
	auto mul = [&](int c, int v) -> uint32_t { return (c && v) ? gexp[glog[c] + glog[v]] : 0u; };
	for (int j = 0; j < 24; j++) {
		const int c = gexp[(4 * j) % 255];
		for (int x = 0; x < 8; x++) {
			sw[8 * j + 0 + x / 4] |= mul(c, x) << (8 * (x % 4));
			sw[8 * j + 2 + x / 4] |= mul(c, x << 3) << (8 * (x % 4));
			if (x < 4) sw[8 * j + 4] |= mul(c, x << 6) << (8 * x);
		}
	}
}

void fec_gf64_tables(uint8_t g64[192])
{
	memset(g64, 0, 192);
	int x = 1;
	for (int i = 0; i < 63; i++) { g64[i] = (uint8_t)x; g64[128 + x] = (uint8_t)i; x <<= 1; if (x & 0x40) x ^= 0x43; }
	for (int i = 63; i < 128; i++) g64[i] = g64[i - 63];
}

void fec_m10_table(uint16_t tab[99 * 8])
{
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
	for (int j = 0; j < 8; j++) {
		unsigned c = step(0, 1u << j);
		for (int k = 0; k < 99; k++) { tab[8 * k + j] = (uint16_t)c; c = step(c, 0); }
	}
}

void fec_mrz_table(uint16_t tab[43 * 8])
{
	auto step = [](unsigned c, unsigned b) {
		c ^= b;
		for (int k = 0; k < 8; k++) c = (c & 1u) ? ((c >> 1) ^ 0xA001u) : (c >> 1);
		return c;
	};
	for (int j = 0; j < 8; j++) {
		unsigned c = step(0, 1u << j);
		for (int k = 0; k < 43; k++) { tab[8 * k + j] = (uint16_t)c; c = step(c, 0); }
	}
}

// ---------------------------------------------------------------- row layout
extern "C" size_t sonde_sample_bytes(int input_kind)
{
	return sd_sample_bytes(input_kind);
}

// Channel stride (in elements) this library recommends for rows of n_samples: the next power of two in BYTES from 64 KiB up.
// Measured (profiles/r3_stride_sweep.txt, three boxes): 1024 rows of 1.5 MiB streamed side by side run 2.3-5.5 % faster 2 MiB
// apart than back to back (rows 384 KiB -> 512 KiB: +0.8 %); strides a little off a power of two (2064 KiB) can be 7 % SLOWER
// than the contiguous layout: how the rows that are in flight together spread over the HBM channels.
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
