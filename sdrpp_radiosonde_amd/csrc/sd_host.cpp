// sd_host.cpp -- the error text behind sonde_last_error(), shared by every host object of the library, and the version string.
#include <string>
#include "launch.h"
#include "sd_host.h"

static thread_local std::string g_err;

int sd_fail(const char *what, hipError_t e)
{
	g_err = what;
	if (e != hipSuccess) { g_err += ": "; g_err += hipGetErrorString(e); }
	return -1;
}
int sd_fail_msg(const char *what) { return sd_fail(what, hipSuccess); }

extern "C" const char *sonde_last_error(void) { return g_err.c_str(); }
extern "C" const char *sonde_version(void) { return "sonde_mi355 0.1 (gfx950)"; }
