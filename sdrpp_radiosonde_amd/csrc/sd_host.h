// sd_host.h -- the error message behind sonde_last_error() (sd_host.cpp), for every host source of the library
#pragma once
int sd_fail_msg(const char *what);      // records the message, returns -1: for pure-host sources (no HIP include)
// HIP sources use sd_fail(what, hipError_t) of launch.h, which appends the HIP error's text; the batch files check HIP calls with
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return sd_fail(#x, e_); } while (0)
