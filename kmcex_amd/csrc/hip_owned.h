// hip_owned.h -- the owners of what the host layer takes from HIP: device and pinned buffers, streams, events.  Host code.
//
// A buffer keeps its pointer and its capacity together and frees itself; a stream is drained, then destroyed, by its
// destructor.  Every allocation passes through kmx_owned_alloc, which times the device allocations (KMX_CTRL_DEBUG) and
// hosts the test hook KMX_FAIL_ALLOC; its two counters are defined once, in kmx_api.hip.  The by-value kernel argument
// blocks of kmx_types.h stay plain structs of raw pointers: they are views, filled from these owners.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <utility>

#define RCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

extern std::atomic<unsigned long long> kmx_malloc_ns;       // time inside hipMalloc (KMX_CTRL_DEBUG=1 prints it per build)
// KMX_FAIL_ALLOC=n (test hook): armed at the entry of a C entry point, process-wide because helper threads allocate too.
// The n-th allocation made while it runs returns hipErrorOutOfMemory without calling HIP.  0: idle.
extern std::atomic<long long> kmx_fail_alloc;
// the one place every owner below allocates through
inline hipError_t kmx_owned_alloc(void **p, size_t bytes, bool pinned, unsigned host_flags)
{
	if (kmx_fail_alloc.load(std::memory_order_relaxed) > 0 && kmx_fail_alloc.fetch_sub(1) == 1) return hipErrorOutOfMemory;
	if (pinned) return hipHostMalloc(p, bytes, host_flags);
	const auto t0 = std::chrono::steady_clock::now();
	const hipError_t e = hipMalloc(p, bytes);
	kmx_malloc_ns += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
	return e;
}

template <typename T, bool PINNED> class HipBuf {
	T *p_ = nullptr;
	size_t n_ = 0;                                                  // elements asked for
	unsigned host_flags_ = 0;

public:
	HipBuf() = default;
	explicit HipBuf(unsigned host_flags) : host_flags_(host_flags) {}
	HipBuf(HipBuf &&o) noexcept : p_(o.p_), n_(o.n_), host_flags_(o.host_flags_) { o.p_ = nullptr; o.n_ = 0; }
	HipBuf &operator=(HipBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
	~HipBuf() { reset(); }
	void reset()
	{
		if (p_) { if (PINNED) (void)hipHostFree(p_); else (void)hipFree(p_); }
		p_ = nullptr;
		n_ = 0;
	}
	// n elements (none: 16 bytes); what was held goes first.  A failure leaves the buffer empty with capacity 0.
	hipError_t alloc(size_t n)
	{
		reset();
		const hipError_t e = kmx_owned_alloc((void **)&p_, n ? n * sizeof(T) : 16, PINNED, host_flags_);
		if (e != hipSuccess) p_ = nullptr; else n_ = n;
		return e;
	}
	// grow-only: reallocated only when n exceeds what is there (bench loops rebuild the same sizes), after `st` has drained
	hipError_t ensure(size_t n, hipStream_t st)
	{
		if (p_ && n <= n_) return hipSuccess;
		if (p_) { const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) return e; }
		return alloc(n);
	}
	T *get() const { return p_; }
	size_t cap() const { return n_; }
	operator T *() const { return p_; }
};
template <typename T> struct DevBuf : HipBuf<T, false> {
	using HipBuf<T, false>::HipBuf;
};
template <typename T> struct PinBuf : HipBuf<T, true> {
	using HipBuf<T, true>::HipBuf;                                  // PinBuf<u64> h{hipHostMallocMapped}
};

// created on first use (ensure), with the flags every call site of its kind uses
class Stream {
	hipStream_t s_ = nullptr;

public:
	Stream() = default;
	Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
	Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
	~Stream() { reset(); }
	hipError_t ensure() { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
	void reset()
	{
		if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); }
		s_ = nullptr;
	}
	operator hipStream_t() const { return s_; }
};
class Event {
	hipEvent_t e_ = nullptr;

public:
	Event() = default;
	Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
	Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
	~Event() { reset(); }
	void reset()
	{
		if (e_) (void)hipEventDestroy(e_);
		e_ = nullptr;
	}
	hipError_t ensure(unsigned flags = hipEventDisableTiming) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
	operator hipEvent_t() const { return e_; }
};

template <typename F> struct ScopeExit {
	F f;
	explicit ScopeExit(F g) : f(g) {}
	~ScopeExit() { f(); }
};
template <typename F> static ScopeExit<F> scope_exit(F f) { return ScopeExit<F>(f); }
