// sd_tables.h -- everything the host computes once and the kernels only read: the modem table (SPEC), the
// polyphase taps, the AFSK mixer tables and the FEC tables.  Pure host code (sd_tables.cpp): no HIP, no batch object.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sonde_dev.h"
#include "../../include/sonde_abi.h"

// SPEC 3.6's mixer table: out[2k], out[2k + 1] = (cos, -sin)(2 pi cycles k / per) as float32
void make_mixer(float *out, int cycles, int per);

#pragma GCC visibility push(hidden)       // what follows is shared by the library's own sources only: not among its exported symbols
struct ModemDef { double baud; float cutoff; int decim; int pre; };   // pre = 8: AFSK tone demodulator in front (SPEC 3.6)
extern const ModemDef k_modems[SONDE_NTYPES];
// a batch's modem table: k_modems with the configuration flags applied (SONDE_FLAG_WIDE / _WIDE_AUTO: one decimation step less)
void modem_table(uint32_t flags, int input_kind, ModemDef out[SONDE_NTYPES]);

int modem_div(const ModemDef *md, int type);              // input samples per internal sample
int32_t modem_period0(const ModemDef *md, int type);      // Q16 internal samples per symbol
int modem_nt(const ModemDef *md, int type);               // taps in use per polyphase row
// demod-kernel class of a (decimation, taps) pair: the instantiations of sd_demod_kernel; -1: none
extern const int k_cls_decim[4], k_cls_nt[4];
int modem_class(const ModemDef *md, int type);
// upper bound of the bits a channel of this type produces in a submit of max_samples (at the fastest symbol clock the loop allows)
uint64_t bits_per_submit(const ModemDef *md, int type, uint32_t max_samples);
// what the kernels read of the table (sonde_dev.h SdModem)
void modem_fill(const ModemDef *md, SdModem out[SONDE_NTYPES]);

void make_taps(const ModemDef *md, int type, float *out /* [SD_NPHASE][SD_NTAPS] */);

// ---- FEC tables, each into the caller's array
// GF(2^8), primitive polynomial 0x11D, in the log domain without zero tests: log 0 = 768 (above any sum of valid logs), the antilog
// periodic below 768 and zero above (GF_EXP2 in framer_kernel.hip)
#define SD_GFEXP_BYTES 2304
void fec_gf256_tables(uint8_t exp2[SD_GFEXP_BYTES], uint16_t log2[256]);
// byte-slice tables of the multipliers c_j = alpha^(4j), j = 0..23 (framer_kernel.hip gf_swar_mul):
// words 0,1: c*x for x = 0..7;  words 2,3: c*(x << 3);  word 4: c*(x << 6), x = 0..3;  words 5..7 unused
void fec_gf256_swar(uint32_t sw[24 * 8]);
// GF(2^6)/x^6+x+1 tables for BCH(63,51): exp[128] then log[64]
void fec_gf64_tables(uint8_t g64[192]);
// M10 checksum: c' = f(c, b) is GF(2)-linear, c' = A c + B b; row k holds A^k B e_j for the eight unit bytes e_j (sd_fixed.h)
void fec_m10_table(uint16_t tab[99 * 8]);
// MRZ-N1 CRC16 (reflected 0xA001) as a GF(2) matrix, laid out like the M10 table: row k holds the CRC, run from 0, of the unit byte e_j
// followed by k zero bytes (check_rescue_kernel.hip: the column of a frame bit, SPEC 3.3f)
void fec_mrz_table(uint16_t tab[43 * 8]);
#pragma GCC visibility pop
