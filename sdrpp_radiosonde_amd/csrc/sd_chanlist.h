// sd_chanlist.h -- how a list of channel numbers reaches a kernel without a host synchronisation (SPEC 3.12: the restart launches of
// SondeBatch and SondeDetector).  The list is written into pinned host memory the kernel reads in place; a buffer is taken again
// only once the event recorded behind its kernel has completed (hipEventQuery: no wait), otherwise another one is allocated.  A
// live loop that restarts once per submit ends up with two or three buffers.  The buffers and their events go with the object that
// holds the SdChanLists (sd_devmem.h), which has waited for its kernels by then.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <utility>
#include <vector>
#include "sd_devmem.h"

struct __attribute__((visibility("hidden"))) SdChanLists {
	struct Buf { PinnedBuf<uint32_t> list; DevEvent ev; bool queued = false; };
	std::vector<Buf> bufs;

	// a buffer that holds `list` (the kernel reads list.dev()), or null; call done() behind the kernel that reads it
	Buf *put(const uint32_t *list, size_t n)
	{
		Buf *b = nullptr;
		for (Buf &c : bufs)
			if (c.list.cap() >= n && (!c.queued || hipEventQuery(c.ev) == hipSuccess)) { b = &c; break; }
		(void)hipGetLastError();        // (hipErrorNotReady of a query is no error)
		if (!b) {
			Buf c;
			if (c.list.alloc(n < 256 ? 256 : n) != hipSuccess || c.ev.create(hipEventDisableTiming) != hipSuccess) return nullptr;
			bufs.push_back(std::move(c));
			b = &bufs.back();
		}
		memcpy(b->list.host(), list, n * sizeof(uint32_t));
		b->queued = false;
		return b;
	}
	hipError_t done(Buf *b, hipStream_t s)
	{
		const hipError_t e = hipEventRecord(b->ev, s);
		b->queued = e == hipSuccess;
		return e;
	}
};
