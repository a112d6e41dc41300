// sd_design.h -- the filter prototype of SPEC 3.7, which the VFO front-end, the tuner (SPEC 3.9) and the channelizer (SPEC 3.5: its
// window and its 12/5 resampler) all use, and pi.  Pure host code (sd_design.cpp), double; the tables are part of the
// bit-exactness contract: the order of every operation is the SPEC's.
#pragma once
#include <stddef.h>
#include <vector>

constexpr double SD_PI = 3.14159265358979323846;

#pragma GCC visibility push(hidden)
// N taps of Blackman-windowed sinc at cutoff fc (cycles per sample): h[i] = sinc_fc(i - (N - 1) / 2) (0.42 - 0.5 cos + 0.08 cos)
std::vector<double> sd_design_prototype(size_t N, double fc);
// the prototype h of up * T taps as `up` polyphase rows of T float taps, each row normalised to unit DC gain:
// g[p][t] = (float)(h[t up + p] / sum_t h[t up + p]), the sum over t ascending
void sd_design_rows(const std::vector<double> &h, size_t up, size_t T, float *g);
#pragma GCC visibility pop
