// edit_device.hip -- kmx_edit_seqs_dev / kmx_apply_edits_dev: the edit list sorted, and applied to the bases it was found on.
//
// The sites of kmx_edit_seqs append their edits in whatever order the waves finish; rocPRIM's radix sort (the vendor
// primitive for a plain key sort, as for the rest table) makes the list ascending, which is what makes it identical
// across runs, variants and chunk sizes.  Applying it is a streaming copy: an edit's shift is its rank among the insertions
// minus its rank among the deletions (one exclusive scan over the list, both ranks in one 64-bit word), and 16 input bytes
// find theirs by binary search in the list, which is small beside the bases and stays in L2.
#include "hip_owned.h"
#include "launchers.h"
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace {

inline unsigned nblk(u64 n) { return (unsigned)((n + 255) / 256); }

// INS in the low half, DEL in the high one; entry n is 0, so the exclusive scan of n + 1 entries ends with the totals
__global__ __launch_bounds__(256) void k_edit_kinds(const u64 *edits, u64 n, u64 *kind)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	const u32 op = i < n ? (u32)(edits[i] >> 4) & 15u : 0u;
	kind[i] = (u64)(op == 3) | ((u64)(op == 2) << 32);
}

// the first edit at or behind position p
__device__ __forceinline__ u64 edit_lower(const u64 *edits, u64 n, u64 p)
{
	u64 lo = 0, hi = n;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if ((edits[mid] >> 8) < p) lo = mid + 1; else hi = mid;
	}
	return lo;
}
__device__ __forceinline__ u64 edit_shift(u64 sc) { return (sc & 0xFFFFFFFFULL) - (sc >> 32); }   // (mod 2^64: added to a position)

__global__ __launch_bounds__(256) void k_edit_offsets(const u64 *offs, u64 n_seqs, u64 n_bases, const u64 *edits, u64 n, const u64 *scan, u64 *offs_out)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > n_seqs) return;
	const u64 o = offs[i] < n_bases ? offs[i] : n_bases;
	offs_out[i] = o + edit_shift(scan[edit_lower(edits, n, o)]);
}

// a thread per 16 input bytes: one 16-byte copy when no edit falls among them and both sides are aligned, byte by byte otherwise.
// Nothing is written at or behind out[out_cap], whatever the list holds.
__global__ __launch_bounds__(256) void k_edit_apply(const unsigned char *in, u64 n_bases, const u64 *edits, u64 n, const u64 *scan, unsigned char *out, u64 out_cap)
{
	const u64 b0 = ((u64)blockIdx.x * 256 + threadIdx.x) * 16;
	if (b0 >= n_bases) return;
	const u64 b1 = b0 + 16 < n_bases ? b0 + 16 : n_bases;
	u64 i = edit_lower(edits, n, b0);
	const u64 i1 = edit_lower(edits, n, b1);
	u64 o = b0 + edit_shift(scan[i]);
	if (i == i1 && b1 - b0 == 16 && o <= out_cap && out_cap - o >= 16 && !(((uintptr_t)(in + b0) | (uintptr_t)(out + o)) & 15)) {
		*(uint4 *)(out + o) = *(const uint4 *)(in + b0);
		return;
	}
	for (u64 p = b0; p < b1; p++) {
		u32 c = in[p];
		bool drop = false;
		for (; i < i1 && (edits[i] >> 8) == p; i++) {
			const u32 op = (u32)(edits[i] >> 4) & 15u, b = (u32)"ACGT"[edits[i] & 3];
			if (op == 1) c = b;
			else if (op == 2) drop = true;
			else if (op == 3) { if (o < out_cap) out[o] = (unsigned char)b; o++; }
		}
		if (drop) continue;
		if (o < out_cap) out[o] = (unsigned char)c;
		o++;
	}
}

}   // namespace

namespace kmxk {

hipError_t edit_sort(u64 *keys, u64 *alt, u64 n, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	if (n < 2) return hipSuccess;
	size_t bytes = 0;
	RCHK(rocprim::radix_sort_keys(nullptr, bytes, (const u64 *)keys, alt, (size_t)n, 0, 64, st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::radix_sort_keys(tmp.get(), bytes, (const u64 *)keys, alt, (size_t)n, 0, 64, st));
	return hipMemcpyAsync(keys, alt, n * 8, hipMemcpyDeviceToDevice, st);
}

// scan: room for 2 (n + 1) words; *d_total receives the totals (INS low, DEL high).  out / offs_out as kmx_apply_edits_dev.
hipError_t edit_apply(const unsigned char *in, const u64 *offs, u64 n_seqs, u64 n_bases, const u64 *edits, u64 n, u64 *scan, unsigned char *out, u64 out_cap, u64 *offs_out, unsigned long long *d_total, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	u64 *kind = scan + (n + 1);
	hipLaunchKernelGGL(k_edit_kinds, dim3(nblk(n + 1)), dim3(256), 0, st, edits, n, kind);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const u64 *)kind, scan, (u64)0, (size_t)(n + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const u64 *)kind, scan, (u64)0, (size_t)(n + 1), rocprim::plus<u64>(), st));
	RCHK(hipMemcpyAsync(d_total, scan + n, 8, hipMemcpyDeviceToDevice, st));
	hipLaunchKernelGGL(k_edit_offsets, dim3(nblk(n_seqs + 1)), dim3(256), 0, st, offs, n_seqs, n_bases, edits, n, (const u64 *)scan, offs_out);
	if (n_bases) hipLaunchKernelGGL(k_edit_apply, dim3(nblk((n_bases + 15) / 16)), dim3(256), 0, st, in, n_bases, edits, n, (const u64 *)scan, out, out_cap);
	return hipGetLastError();
}

}   // namespace kmxk
