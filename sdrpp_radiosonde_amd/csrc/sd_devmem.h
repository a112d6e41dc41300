// sd_devmem.h -- the one way the host objects own what HIP hands out: device memory (DevBuf, DevPair), pinned host memory (PinnedBuf),
// events (DevEvent) and streams (DevStream).  Each is a move-only member that releases what it holds when the object is deleted, on
// the device that is current then: a destroy entry selects the object's device, waits for the object's own work and deletes -- it
// names no member, and the order in which the members go does not matter.  Every call returns the hipError_t of the HIP call that
// failed, for HIPCHK (sd_host.h); each owner converts to the plain handle, which is what launchers and HIP calls take.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#pragma GCC visibility push(hidden)       // the instantiations stay out of the library's exported symbols
// One allocation of n elements of T; move-only.  A second alloc / zeros / upload replaces the first.
template <typename T> class DevBuf {
	T *p_ = nullptr;
	void drop() { (void)hipFree(p_); p_ = nullptr; }
public:
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
	~DevBuf() { drop(); }
	hipError_t alloc(size_t n) { drop(); return hipMalloc((void **)&p_, n * sizeof(T)); }
	hipError_t zeros(size_t n) { const hipError_t e = alloc(n); return e != hipSuccess ? e : hipMemset(p_, 0, n * sizeof(T)); }
	hipError_t upload(const T *src, size_t n)
	{
		const hipError_t e = alloc(n);
		return e != hipSuccess ? e : hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
	}
	operator T *() const { return p_; }
};

// State carried from submit to submit, double-buffered: a submit's kernels read in() and write out() (the workgroup that writes the
// state is not the one that reads it), then the host flips.
template <typename T> class DevPair {
	DevBuf<T> b_[2];
	unsigned k_ = 0;
public:
	hipError_t zeros(size_t n) { const hipError_t e = b_[0].zeros(n); return e != hipSuccess ? e : b_[1].zeros(n); }
	T *in() const { return b_[k_]; }
	T *out() const { return b_[k_ ^ 1u]; }
	void flip() { k_ ^= 1u; }
};

// n elements of T in pinned host memory that a kernel reads in place through dev(); move-only.  One alloc per object.
template <typename T> class PinnedBuf {
	T *host_ = nullptr, *dev_ = nullptr;
	size_t cap_ = 0;
public:
	PinnedBuf() = default;
	PinnedBuf(PinnedBuf &&o) noexcept : host_(o.host_), dev_(o.dev_), cap_(o.cap_) { o.host_ = o.dev_ = nullptr; o.cap_ = 0; }
	~PinnedBuf() { (void)hipHostFree(host_); }
	hipError_t alloc(size_t n)
	{
		const hipError_t e = hipHostMalloc((void **)&host_, n * sizeof(T), hipHostMallocDefault);
		if (e != hipSuccess) return e;
		cap_ = n;
		return hipHostGetDevicePointer((void **)&dev_, host_, 0);
	}
	T *host() const { return host_; }
	T *dev() const { return dev_; }
	size_t cap() const { return cap_; }
};

// An event / a non-blocking stream; move-only.  One create per object (SondeChannelizer creates some of its own only when they are needed).
template <typename H, hipError_t (*Destroy)(H)> class DevHandle {
protected:
	H h_ = nullptr;
public:
	DevHandle() = default;
	DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
	~DevHandle() { if (h_) (void)Destroy(h_); }
	operator H() const { return h_; }
};
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> { hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&h_, flags); } };
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> { hipError_t create() { return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); } };
#pragma GCC visibility pop
