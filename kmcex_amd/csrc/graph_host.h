// graph_host.h -- what the host layers of the graph calls share (unitig_host.h, map_host.h, contig_host.h, resolve_host.h,
// pair_host.h).  Included into kmx_api.hip in front of them.  The checks of offsets, CSR, unitig lengths, k and buffers are
// in graph_checks.h, which needs no HIP; here are the owner of a call's temporary device buffers and the phase clock.
#include "graph_checks.h"

static int graph_nomem(const char *what) { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of %s could not be allocated", what); }

// The device buffers a host form stages its input and output in for the length of one call.  Every buffer is a DevBuf of its
// own.  The first allocation that fails is remembered and nothing is allocated or copied after it: a call site stages
// everything, then asks status() once.  Uploads, downloads and the zeroing are enqueued on the model's stream; a count of 0
// enqueues nothing and its host pointer may be null.  finish() is the host form's final wait.  However the call ends, the
// stream is drained before a buffer is freed.
class Staging {
	kmx_model *m;
	const char *what;                                              // for the message of KMX_E_NOMEM
	std::vector<DevBuf<unsigned char>> bufs;
	std::vector<std::pair<uint64_t *, std::vector<uint64_t>>> adds;
	hipError_t err = hipSuccess;
	bool nomem = false;
	void note(hipError_t e) { if (err == hipSuccess) err = e; }

public:
	Staging(kmx_model *mm, const char *w) : m(mm), what(w) {}
	Staging(const Staging &) = delete;
	~Staging() { (void)hipStreamSynchronize(m->stream); }
	// an output buffer of n elements (none: still an allocation); null once something has failed
	template <typename T> T *out(u64 n)
	{
		if (err != hipSuccess) return nullptr;
		bufs.emplace_back();
		note(bufs.back().alloc(n ? n * sizeof(T) : 0));
		nomem = err != hipSuccess;
		return (T *)bufs.back().get();
	}
	template <typename T> T *zeroed(u64 n)
	{
		T *d = out<T>(n);
		if (d && n) note(hipMemsetAsync(d, 0, n * sizeof(T), m->stream));
		return d;
	}
	// n elements of host memory as the device's type of the same layout, in a buffer of max(n, room) elements
	template <typename T, typename H> T *in(const H *h, u64 n, u64 room = 0)
	{
		static_assert(sizeof(T) == sizeof(H), "one layout");
		T *d = out<T>(std::max(n, room));
		if (d && n) note(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, m->stream));
		return d;
	}
	template <typename T, typename H> void down(H *h, const T *d, u64 n)
	{
		static_assert(sizeof(T) == sizeof(H), "one layout");
		if (n && err == hipSuccess) note(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, m->stream));
	}
	// h[i] += d[i] for i < n, once finish() has waited
	void down_add(uint64_t *h, const void *d, u64 n)
	{
		if (!n || err != hipSuccess) return;
		adds.emplace_back(h, std::vector<uint64_t>(n));
		note(hipMemcpyAsync(adds.back().second.data(), d, n * 8, hipMemcpyDeviceToHost, m->stream));
	}
	// KMX_OK, KMX_E_NOMEM for an allocation that failed, KMX_E_NODEVICE for a copy
	int status() const
	{
		if (nomem) return graph_nomem(what);
		if (err != hipSuccess) return fail(KMX_E_NODEVICE, "staging %s failed: %s", what, hipGetErrorString(err));
		return KMX_OK;
	}
	int finish()
	{
		note(hipStreamSynchronize(m->stream));
		TRY(status());
		for (auto &a : adds)
			for (size_t i = 0; i < a.second.size(); i++) a.first[i] += a.second[i];
		adds.clear();
		return KMX_OK;
	}
};

// A lap adds the time since the last one to phase_s[phase]: only under kmx_set_profile(m, 1), where every phase waits for the
// stream.
struct PhaseClock {
	kmx_model *m;
	double *phase_s;
	std::chrono::steady_clock::time_point t0;
	PhaseClock(kmx_model *mm, double *s) : m(mm), phase_s(s) { if (m->prof.on) { hipStreamSynchronize(m->stream); t0 = std::chrono::steady_clock::now(); } }
	void lap(int phase)
	{
		if (!m->prof.on) return;
		hipStreamSynchronize(m->stream);
		const auto t1 = std::chrono::steady_clock::now();
		phase_s[phase] += std::chrono::duration<double>(t1 - t0).count();
		t0 = t1;
	}
};
