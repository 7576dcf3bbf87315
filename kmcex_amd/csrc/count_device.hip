// count_device.hip -- kmx_count_*: sort, run-length encode, merge and filter the keys k_count_windows emits.
//
// A piece of window keys is sorted with rocPRIM's radix sort (two-word keys: by the low word, then stably by the high one)
// and run-length encoded; its (key, count) pairs are merged into the session's running listing, which is sorted and
// unique, and equal keys are then reduced with a saturating sum.  The listing's keys are in the packed layout of
// include/kmx.h (W words per key, word 0 most significant), so the build takes them as they are.  rocPRIM is the vendor
// primitive for these whole-array passes, as for the rest table (rest_device.hip); its scratch is small beside the arrays.
#include "hip_owned.h"
#include "launchers.h"
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace {

struct K2 { u64 hi, lo; };                                          // a two-word key, word 0 (hi) most significant
__host__ __device__ inline bool operator==(const K2 &a, const K2 &b) { return a.hi == b.hi && a.lo == b.lo; }
__host__ __device__ inline bool operator!=(const K2 &a, const K2 &b) { return !(a == b); }
struct K2Less {
	__host__ __device__ bool operator()(const K2 &a, const K2 &b) const { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
};
struct SatAdd {
	__host__ __device__ u32 operator()(u32 a, u32 b) const { const u32 s = a + b; return s < a ? 0xFFFFFFFFu : s; }
};

__global__ __launch_bounds__(256) void k_zip2(const u64 *hi, const u64 *lo, u64 n, K2 *out)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = K2{hi[i], lo[i]};
}
// keep[i] = ci <= c[i] <= cx; the kept counts are capped to cs afterwards (k_cap)
__global__ __launch_bounds__(256) void k_keep(const u32 *c, u64 n, u32 ci, u32 cx, unsigned char *keep)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < n) keep[i] = c[i] >= ci && c[i] <= cx;
}
__global__ __launch_bounds__(256) void k_cap(u32 *c, const unsigned long long *n, u32 cs)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < *n && c[i] > cs) c[i] = cs;
}

inline unsigned nblk(u64 n) { return (unsigned)((n + 255) / 256); }

template <typename KT, typename LESS>
hipError_t merge_t(const KT *a, const u32 *ac, u64 na, const KT *b, const u32 *bc, u64 nb, KT *m, u32 *mc, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::merge(nullptr, bytes, a, b, m, ac, bc, mc, (size_t)na, (size_t)nb, LESS(), st));
	RCHK(tmp.ensure(bytes, st));
	return rocprim::merge(tmp.get(), bytes, a, b, m, ac, bc, mc, (size_t)na, (size_t)nb, LESS(), st);
}

template <typename KT>
hipError_t reduce_t(const KT *m, const u32 *mc, u64 n, KT *out, u32 *oc, unsigned long long *d_nout, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::reduce_by_key(nullptr, bytes, m, mc, (size_t)n, out, oc, d_nout, SatAdd(), rocprim::equal_to<KT>(), st));
	RCHK(tmp.ensure(bytes, st));
	return rocprim::reduce_by_key(tmp.get(), bytes, m, mc, (size_t)n, out, oc, d_nout, SatAdd(), rocprim::equal_to<KT>(), st);
}

template <typename KT>
hipError_t filter_t(const KT *in, const u32 *ic, u64 n, u32 ci, u32 cs, u32 cx, KT *out, u32 *oc, unsigned char *keep, unsigned long long *d_nout, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	hipLaunchKernelGGL(k_keep, dim3(nblk(n)), dim3(256), 0, st, ic, n, ci, cx, keep);
	size_t b1 = 0, b2 = 0;
	RCHK(rocprim::select(nullptr, b1, in, keep, out, d_nout, (size_t)n, st));
	RCHK(rocprim::select(nullptr, b2, ic, keep, oc, d_nout, (size_t)n, st));
	RCHK(tmp.ensure(b1 > b2 ? b1 : b2, st));
	size_t bytes = tmp.cap();
	RCHK(rocprim::select(tmp.get(), bytes, in, keep, out, d_nout, (size_t)n, st));
	bytes = tmp.cap();
	RCHK(rocprim::select(tmp.get(), bytes, ic, keep, oc, d_nout, (size_t)n, st));
	hipLaunchKernelGGL(k_cap, dim3(nblk(n)), dim3(256), 0, st, oc, (const unsigned long long *)d_nout, cs);
	return hipGetLastError();
}

}   // namespace

namespace kmxk {

// One piece of n window keys (W = 1: lo[n]; W = 2: hi[n], lo[n]; pa = lo, with hi at pa + cap) -> its distinct keys in the
// packed layout at pa, their counts in pc, how many at *d_nu.  pb (2 cap words) is scratch.
hipError_t count_piece(int W, int k, u64 *pa, u64 *pb, u64 cap, u64 n, u32 *pc, unsigned long long *d_nu, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	if (W == 1) {
		RCHK(rocprim::radix_sort_keys(nullptr, bytes, pa, pb, (size_t)n, 0, 2 * k, st));
		RCHK(tmp.ensure(bytes, st));
		RCHK(rocprim::radix_sort_keys(tmp.get(), bytes, pa, pb, (size_t)n, 0, 2 * k, st));
		bytes = 0;
		RCHK(rocprim::run_length_encode(nullptr, bytes, pb, (size_t)n, pa, pc, d_nu, st));
		RCHK(tmp.ensure(bytes, st));
		return rocprim::run_length_encode(tmp.get(), bytes, pb, (size_t)n, pa, pc, d_nu, st);
	}
	u64 *lo = pa, *hi = pa + cap, *lo2 = pb, *hi2 = pb + cap;
	size_t b1 = 0, b2 = 0;
	RCHK(rocprim::radix_sort_pairs(nullptr, b1, lo, lo2, hi, hi2, (size_t)n, 0, 64, st));
	RCHK(rocprim::radix_sort_pairs(nullptr, b2, hi2, hi, lo2, lo, (size_t)n, 0, 2 * k - 64, st));
	RCHK(tmp.ensure(b1 > b2 ? b1 : b2, st));
	bytes = tmp.cap();
	RCHK(rocprim::radix_sort_pairs(tmp.get(), bytes, lo, lo2, hi, hi2, (size_t)n, 0, 64, st));          // by the low word
	bytes = tmp.cap();
	RCHK(rocprim::radix_sort_pairs(tmp.get(), bytes, hi2, hi, lo2, lo, (size_t)n, 0, 2 * k - 64, st));  // stably by the high word
	K2 *z = (K2 *)pb;
	hipLaunchKernelGGL(k_zip2, dim3(nblk(n)), dim3(256), 0, st, (const u64 *)hi, (const u64 *)lo, n, z);
	bytes = 0;
	RCHK(rocprim::run_length_encode(nullptr, bytes, (const K2 *)z, (size_t)n, (K2 *)pa, pc, d_nu, st));
	RCHK(tmp.ensure(bytes, st));
	return rocprim::run_length_encode(tmp.get(), bytes, (const K2 *)z, (size_t)n, (K2 *)pa, pc, d_nu, st);
}

// the running listing a[na] + a piece's b[nb] (both sorted, unique) -> m[na + nb], merged; keys in the packed layout
hipError_t count_merge(int W, const u64 *a, const u32 *ac, u64 na, const u64 *b, const u32 *bc, u64 nb, u64 *m, u32 *mc, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	if (W == 1) return merge_t<u64, rocprim::less<u64>>(a, ac, na, b, bc, nb, m, mc, tmp, st);
	return merge_t<K2, K2Less>((const K2 *)a, ac, na, (const K2 *)b, bc, nb, (K2 *)m, mc, tmp, st);
}

// merged m[n] -> out: equal (adjacent) keys once, their counts summed with saturation; how many at *d_nout
hipError_t count_reduce(int W, const u64 *m, const u32 *mc, u64 n, u64 *out, u32 *oc, unsigned long long *d_nout, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	if (W == 1) return reduce_t<u64>(m, mc, n, out, oc, d_nout, tmp, st);
	return reduce_t<K2>((const K2 *)m, mc, n, (K2 *)out, oc, d_nout, tmp, st);
}

// the listing's keys with ci <= count <= cx -> out (counts capped to cs), how many at *d_nout; keep[n] is scratch
hipError_t count_filter(int W, const u64 *in, const u32 *ic, u64 n, u32 ci, u32 cs, u32 cx, u64 *out, u32 *oc, unsigned char *keep, unsigned long long *d_nout, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	RCHK(hipMemsetAsync(d_nout, 0, sizeof(unsigned long long), st));
	if (!n) return hipSuccess;
	if (W == 1) return filter_t<u64>(in, ic, n, ci, cs, cx, out, oc, keep, d_nout, tmp, st);
	return filter_t<K2>((const K2 *)in, ic, n, ci, cs, cx, (K2 *)out, oc, keep, d_nout, tmp, st);
}

}   // namespace kmxk
