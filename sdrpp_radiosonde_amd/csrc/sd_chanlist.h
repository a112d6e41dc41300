// sd_chanlist.h -- how a list of channel numbers reaches a kernel without a host synchronisation (SPEC 3.12: the restart launches of
// SondeBatch and SondeDetector).  The list is written into pinned host memory the kernel reads in place; a buffer is taken again
// only once the event recorded behind its kernel has completed (hipEventQuery: no wait), otherwise another one is allocated.  A
// live loop that restarts once per submit ends up with two or three buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

struct SdChanLists {
	struct Buf { uint32_t *host = nullptr, *dev = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool queued = false; };
	std::vector<Buf> bufs;

	// a buffer that holds `list`, or null; call done() behind the kernel that reads it
	Buf *put(const uint32_t *list, size_t n)
	{
		Buf *b = nullptr;
		for (Buf &c : bufs)
			if (c.cap >= n && (!c.queued || hipEventQuery(c.ev) == hipSuccess)) { b = &c; break; }
		(void)hipGetLastError();        // (hipErrorNotReady of a query is no error)
		if (!b) {
			Buf c;
			c.cap = n < 256 ? 256 : n;
			if (hipHostMalloc((void **)&c.host, c.cap * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) return nullptr;
			if (hipHostGetDevicePointer((void **)&c.dev, c.host, 0) != hipSuccess ||
			    hipEventCreateWithFlags(&c.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(c.host); return nullptr; }
			bufs.push_back(c);
			b = &bufs.back();
		}
		memcpy(b->host, list, n * sizeof(uint32_t));
		b->queued = false;
		return b;
	}
	hipError_t done(Buf *b, hipStream_t s)
	{
		const hipError_t e = hipEventRecord(b->ev, s);
		b->queued = e == hipSuccess;
		return e;
	}
	void destroy()
	{
		for (Buf &c : bufs) { if (c.ev) (void)hipEventDestroy(c.ev); (void)hipHostFree(c.host); }
		bufs.clear();
	}
};
