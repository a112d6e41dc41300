// sd_devmem.h -- the one way the host objects own device memory.  The raw helpers take a pointer member and a size in bytes (the batch
// object, batch_impl.h); DevBuf / DevPair are the members of the front-end objects: what they own is freed when the object is
// deleted, on the device that is current then (every destroy selects the object's device first).  Every call returns the
// hipError_t of the HIP call that failed, for HIPCHK (sd_host.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

template <typename T> static hipError_t dev_alloc(T *&p, size_t bytes) { return hipMalloc((void **)&p, bytes); }
template <typename T> static hipError_t dev_upload(T *&p, const void *src, size_t bytes)
{
	const hipError_t e = dev_alloc(p, bytes);
	return e != hipSuccess ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
}
template <typename T> static hipError_t dev_zeros(T *&p, size_t bytes)
{
	const hipError_t e = dev_alloc(p, bytes);
	return e != hipSuccess ? e : hipMemset(p, 0, bytes);
}

#pragma GCC visibility push(hidden)       // the instantiations stay out of the library's exported symbols
// One allocation of n elements of T; move-only.  A second alloc / zeros / upload replaces the first.
template <typename T> class DevBuf {
	T *p_ = nullptr;
	void drop() { (void)hipFree(p_); p_ = nullptr; }
public:
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
	~DevBuf() { drop(); }
	hipError_t alloc(size_t n) { drop(); return dev_alloc(p_, n * sizeof(T)); }
	hipError_t zeros(size_t n) { drop(); return dev_zeros(p_, n * sizeof(T)); }
	hipError_t upload(const T *src, size_t n) { drop(); return dev_upload(p_, src, n * sizeof(T)); }
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
#pragma GCC visibility pop
