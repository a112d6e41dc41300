// sd_host.h -- the error message behind sonde_last_error() (sd_host.cpp), for every host source of the library
#pragma once
int sd_fail_msg(const char *what);      // records the message, returns -1: for pure-host sources (no HIP include)
// the first step of every create behind its argument checks: makes `device` the current HIP device; on failure records
// "<fn>: no such HIP device (this library has no CPU path)" with the HIP error, if there is one, and returns -1
__attribute__((visibility("hidden"))) int sd_select_device(int device, const char *fn);
// HIP sources use sd_fail(what, hipError_t) of launch.h, which appends the HIP error's text, and check HIP calls with
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return sd_fail(#x, e_); } while (0)
// the same with the entry point's name in front (a string literal)
#define HIPCHK_IN(fn, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return sd_fail(fn ": " #x, e_); } while (0)
