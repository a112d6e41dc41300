// sd_design.cpp -- the filter prototype (sd_design.h)
#include <math.h>
#include "sd_design.h"

std::vector<double> sd_design_prototype(size_t N, double fc)
{
	std::vector<double> h(N);
	for (size_t i = 0; i < N; i++) {
		const double t = (double)i - 0.5 * (double)(N - 1);
		const double x = (double)i / (double)(N - 1);
		const double w = 0.42 - 0.5 * cos(2.0 * SD_PI * x) + 0.08 * cos(4.0 * SD_PI * x);
		const double s = (t == 0.0) ? 2.0 * fc : sin(2.0 * SD_PI * fc * t) / (SD_PI * t);
		h[i] = s * w;
	}
	return h;
}

void sd_design_rows(const std::vector<double> &h, size_t up, size_t T, float *g)
{
	for (size_t p = 0; p < up; p++) {
		double sum = 0.0;
		for (size_t t = 0; t < T; t++) sum += h[t * up + p];
		for (size_t t = 0; t < T; t++) g[p * T + t] = (float)(h[t * up + p] / sum);
	}
}
