// walk_kernels.h -- kmx_unitig_walk_segs*: the segments of a batch of mapped reads threaded through the unitig graph (the rule:
// include/kmx.h; the host side: map_host.h; the launcher: unitig_device.hip).  One lane per segment; the kernels, in the order
// the launcher runs them:
//   k_walk_first   per read: the flag byte of its first segment becomes WALK_START (the bytes are zero before);
//   k_walk_join    per segment: itself and its predecessor (two neighbouring 24-byte records), m_u of the predecessor's unitig and
//                  its row of the CSR, at most 4 entries: the kind of the join, if there is one.  It writes the flag byte (walk
//                  start, step start, kind), the join's d and its overlap in one word, +1 on the traversed link, and the call's
//                  five counters (summed in LDS, one atomic per block and counter);
//   (an exclusive scan of the pair (walk starts, step starts), read straight from the flag bytes: unitig_device.hip)
//   k_walk_heads   per segment that starts a walk: the walk's record with its head fields, its sums zero; per segment that starts a
//                  step: the step; per read: walk_offsets;
//   k_walk_sums    per segment: what the walk's record takes from it, as integer atomics (one per wave and field where a whole
//                  wave lies in one walk); the walk's last segment adds the tail fields.
// Every decision looks at one segment, its predecessor and one row, so the result is a function of (segments, CSR, m_u,
// parameters) alone.  No lane walks a read or a walk.  Row bounds are clamped into [0, n_links], a segment with o >= 2 U joins
// nothing and has no m_u looked up, seg_offsets are clamped into [0, n_segs], and every store is checked against its capacity.
#pragma once
#include "kmx_types.h"

static constexpr u64 WALK_NO_LINK = ~0ULL;

__device__ __forceinline__ u64 walk_clamp(u64 x, u64 hi) { return x < hi ? x : hi; }

// thread r < n_seqs
__global__ __launch_bounds__(256) void k_walk_first(WalkDev D)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	if (r >= D.n_seqs) return;
	const u64 a = walk_clamp(D.so[r], D.n_segs), b = walk_clamp(D.so[r + 1], D.n_segs);
	if (a < b) D.flag[a] = WALK_START;
}

// thread i < n_segs: segment B = segs[i] and the join A -> B with its predecessor
__global__ __launch_bounds__(256) void k_walk_join(WalkDev D)
{
	__shared__ unsigned int s_cnt[WALK_C_N];
	if (threadIdx.x < WALK_C_N) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < D.n_segs) {
		const MapSeg B = D.segs[i];
		unsigned f = WALK_START | WALK_STEP;
		u32 jn = 0;
		if (i > 0 && !(D.flag[i] & WALK_START)) {
			const MapSeg A = D.segs[i - 1];
			const long long g = (long long)(B.pos - A.pos - (u64)A.n_windows);
			unsigned kind = 0;
			long long d = 0;
			u64 e = WALK_NO_LINK;
			if (g >= 0 && g <= (long long)D.max_gap && (u64)A.o < 2 * D.U && (u64)B.o < 2 * D.U) {
				const long long mA = (long long)D.mu[A.o >> 1], endA = (long long)A.off + (long long)A.n_windows - 1, offB = (long long)B.off;
				const u64 lo = walk_clamp(D.loffs[A.o], D.n_links), hi0 = walk_clamp(D.loffs[A.o + 1], D.n_links);
				const u64 hi = hi0 > lo ? (hi0 - lo > 4 ? lo + 4 : hi0) : lo;
				for (u64 t = lo; t < hi; t++)
					if (e == WALK_NO_LINK && D.links[t] == B.o) e = t;
				if (g == 0) {
					if (endA == mA - 1 && offB == 0 && e != WALK_NO_LINK) kind = WALK_EDGE;
				} else {
					const long long di = (offB - endA - 1) - g, da = (mA - 1 - endA) + offB - g, lim = (long long)D.max_indel;
					if (B.o == A.o && offB > endA && di >= -lim && di <= lim) { kind = WALK_INSIDE; d = di; }
					else if (e != WALK_NO_LINK && da >= -lim && da <= lim) { kind = WALK_ACROSS; d = da; }
				}
			}
			if (kind) {
				const long long ov = (long long)D.k - 1 - g;
				f = kind | (kind == WALK_INSIDE ? 0u : (unsigned)WALK_STEP);
				jn = (u32)(ov > 0 ? ov : 0) << 16 | ((u32)(int)d & 0xFFFFu);
				if (kind != WALK_INSIDE && D.link_hits) atomicAdd(D.link_hits + e, 1ULL);
				atomicAdd(&s_cnt[kind == WALK_EDGE ? WALK_C_EDGE : (kind == WALK_INSIDE ? WALK_C_INSIDE : WALK_C_ACROSS)], 1u);
			} else
				atomicAdd(&s_cnt[g == 0 ? WALK_C_UNLINKED : WALK_C_BREAKS], 1u);
		}
		D.flag[i] = (unsigned char)f;
		D.join[i] = jn;
	}
	__syncthreads();
	if (threadIdx.x < WALK_C_N && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// the pair (walk starts, step starts) of segment i from its flag byte (i == n: nothing, so that the exclusive scan ends with the totals)
struct WalkFlagTot {
	const unsigned char *flag;
	u64 n;
	__host__ __device__ WalkTot operator()(u64 i) const
	{
		if (i >= n) return WalkTot{0, 0};
		const unsigned f = flag[i];
		return WalkTot{f & 1u, (f >> 1) & 1u};
	}
};
struct WalkPlus {
	__host__ __device__ WalkTot operator()(const WalkTot &a, const WalkTot &b) const { return WalkTot{a.w + b.w, a.s + b.s}; }
};

// thread i: segment i (i < n_segs) and read i (i <= n_seqs)
__global__ __launch_bounds__(256) void k_walk_heads(WalkDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i <= D.n_seqs) D.wo[i] = D.sc[walk_clamp(D.so[i], D.n_segs)].w;
	if (i >= D.n_segs) return;
	const unsigned f = D.flag[i];
	if (!(f & WALK_STEP)) return;
	const WalkTot t = D.sc[i];
	const MapSeg B = D.segs[i];
	if (D.steps && t.s < D.step_cap) D.steps[t.s] = B.o;
	if ((f & WALK_START) && D.walks && t.w < D.walk_cap)
		D.walks[t.w] = Walk{B.pos, 0 - B.pos, 0, 0, i, t.s, 0, 0, B.off, 0, 0, 0, 0, 0};   // n_span: the tail adds where the walk ends
}

__device__ __forceinline__ u64 walk_xor64(u64 v, int m)
{
	const u32 lo = (u32)__shfl_xor((int)(u32)v, m), hi = (u32)__shfl_xor((int)(u32)(v >> 32), m);
	return (u64)hi << 32 | lo;
}

// thread i < n_segs (every lane of the block stays to the end: the waves shuffle)
__global__ __launch_bounds__(256) void k_walk_sums(WalkDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const bool valid = i < D.n_segs;
	u64 w = ~0ULL, c_map = 0, c_cov = 0;
	u32 c_in = 0, c_ac = 0, c_step = 0;
	int c_d = 0;
	if (valid) {
		w = D.sc[i + 1].w - 1;                                       // segment 0 starts a walk, so the count is at least 1
		if (w < D.walk_cap) {
			const MapSeg B = D.segs[i];
			const unsigned f = D.flag[i];
			const u32 jn = D.join[i];
			c_map = B.n_windows;
			c_cov = (u64)B.n_windows + (u64)(D.k - 1) - (u64)(jn >> 16);
			c_d = (int)(short)(jn & 0xFFFFu);
			c_in = f & WALK_INSIDE ? 1u : 0u;
			c_ac = f & WALK_ACROSS ? 1u : 0u;
			c_step = f & WALK_STEP ? 1u : 0u;
			if (i + 1 == D.n_segs || (D.flag[i + 1] & WALK_START)) {    // the walk's last segment
				atomicAdd((unsigned long long *)&D.walks[w].n_span, (unsigned long long)(B.pos + B.n_windows));
				D.walks[w].off_last = B.off + B.n_windows - 1;
			}
		} else
			w = ~0ULL;
	}
	u32 c_seg = w != ~0ULL ? 1u : 0u;
	const u64 w0 = (u64)(u32)__shfl((int)(u32)(w >> 32), 0) << 32 | (u32)__shfl((int)(u32)w, 0);   // the walk of the wave's first lane
	if (__all(w == w0 && w != ~0ULL)) {                              // the whole wave lies in one walk: one atomic per field
#pragma unroll
		for (int m = 32; m >= 1; m >>= 1) {
			c_map += walk_xor64(c_map, m);
			c_cov += walk_xor64(c_cov, m);
			c_d += __shfl_xor(c_d, m);
			c_in += (u32)__shfl_xor((int)c_in, m);
			c_ac += (u32)__shfl_xor((int)c_ac, m);
			c_step += (u32)__shfl_xor((int)c_step, m);
			c_seg += (u32)__shfl_xor((int)c_seg, m);
		}
		if ((threadIdx.x & 63) != 0) return;
	} else if (w == ~0ULL)
		return;
	Walk *W = D.walks + w;
	atomicAdd((unsigned long long *)&W->n_mapped, (unsigned long long)c_map);
	atomicAdd((unsigned long long *)&W->n_covered, (unsigned long long)c_cov);
	atomicAdd(&W->n_segs, c_seg);
	if (c_step) atomicAdd(&W->n_steps, c_step);
	if (c_in) atomicAdd(&W->n_inside, c_in);
	if (c_ac) atomicAdd(&W->n_across, c_ac);
	if (c_d) atomicAdd(&W->indel, c_d);
}
