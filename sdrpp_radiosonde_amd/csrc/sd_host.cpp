// sd_host.cpp -- the error text behind sonde_last_error() and the device selection, shared by every host object of the library, and the
// version string.
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

int sd_select_device(int device, const char *fn)
{
	int ndev = 0;
	const hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || device < 0 || device >= ndev)
		return sd_fail((std::string(fn) + ": no such HIP device (this library has no CPU path)").c_str(), e);
	HIPCHK(hipSetDevice(device));
	return 0;
}

extern "C" const char *sonde_last_error(void) { return g_err.c_str(); }
extern "C" const char *sonde_version(void) { return "sonde_mi355 0.1 (gfx950)"; }
