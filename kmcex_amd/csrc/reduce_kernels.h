// reduce_kernels.h -- kmx_unitig_pair_reduce*: a pair list without the entries that skip a unitig (the rule: include/kmx.h; the
// host side: reduce_host.h; the launchers: unitig_device.hip).  The kernels, in the order the host runs them:
//   k_red_rows     one lane per list entry: eligibility and g into its record; its two rows src << 32 | dst at 2 i and 2 i + 1
//                  with the row's number as the value, RED_NO_KEY for an entry that gives none.  IGNORED and BELOW_MIN are summed
//                  in LDS: one global atomic per block and counter;
//   (the launcher sorts the 2 E (key, value) pairs by key, stably: rows of one key are in entry order)
//   k_red_verdict  8 lanes per entry, the grouping of the unitig kernels: a row is as long as the degree of its unitig, and one
//                  lane per entry would leave a wavefront waiting on a repeat's hub.  Four lower-bound searches give out(a) and
//                  out(c ^ 1); lane l takes rows l, l + 8, ... of the shorter one: one more search for first(., .), two g from the
//                  records k_red_rows wrote, m_b from uoffsets.  The group folds (count, smallest b, its row, its delta) by
//                  shuffles and lane 0 writes the record (never its g, which other groups read meanwhile) and the keep flag;
//   (the launcher scans the flags)
//   k_red_compact  behind the host's wait for n_out: one lane per entry that stays copies its 32 bytes and writes origin.
// Every index read from the caller's arrays is clamped or checked where it is read and every store is checked against its
// capacity: bad device input gives wrong verdicts, never an access outside a buffer.  The sorted table is the call's own: every
// row in it comes from an eligible entry, so its ends are below 2 U and its entry below n_plinks.
#pragma once
#include "scaffold_kernels.h"

// m_u of unitig u < U from the clamped offsets; 0 for what is shorter than k
__device__ __forceinline__ u64 red_m(const RedDev &D, u64 u)
{
	const u64 a = ctg_min(D.uoffs[u], D.n_ubases), b = ctg_min(D.uoffs[u + 1], D.n_ubases);
	const u64 len = b > a ? b - a : 0;
	return len >= (u64)D.k ? len - (u64)D.k + 1 : 0;
}

// the first position in skey[0, n) whose key is not below `key`
__device__ __forceinline__ u64 red_lower(const u64 *skey, u64 n, u64 key)
{
	u64 lo = 0, hi = n;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (skey[mid] < key) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

__device__ __forceinline__ u64 red_shfl(u64 v, int src)
{
	return (u64)(u32)__shfl((int)(u32)(v >> 32), src, 8) << 32 | (u32)__shfl((int)(u32)v, src, 8);
}
__device__ __forceinline__ u64 red_shfl_xor(u64 v, int m)
{
	return (u64)(u32)__shfl_xor((int)(u32)(v >> 32), m, 8) << 32 | (u32)__shfl_xor((int)(u32)v, m, 8);
}

// thread i < n_plinks
__global__ __launch_bounds__(256) void k_red_rows(RedDev D)
{
	__shared__ unsigned int s_cnt[2];
	if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	int c = -1;
	if (i < D.n_plinks) {
		const PairLink E = D.plinks[i];
		const bool link = (u64)E.a < 2 * D.U && (u64)E.b < 2 * D.U && (E.a >> 1) != (E.b >> 1) && E.n_pairs >= 1;
		u64 k0 = RED_NO_KEY, k1 = RED_NO_KEY;
		long long g = 0;
		if (!link) c = RED_IGNORED;
		else if (E.n_pairs < D.min_pairs) c = RED_BELOW_MIN;
		else {
			g = (long long)((u64)D.inner - 1 - E.sum_dist / E.n_pairs);
			k0 = (u64)E.a << 32 | E.b;
			k1 = (u64)(E.b ^ 1u) << 32 | (E.a ^ 1u);
		}
		D.rrecs[i] = PairReduce{c < 0 ? (u32)RED_KEPT : (u32)c, 0xFFFFFFFFu, 0, 0, g, 0};
		D.key[2 * i] = k0; D.key[2 * i + 1] = k1;
		D.val[2 * i] = (u32)(2 * i); D.val[2 * i + 1] = (u32)(2 * i + 1);
	}
	for (int j = RED_IGNORED; j <= RED_BELOW_MIN; j++) {
		const u64 b = __ballot(c == j);
		if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_cnt[j], (unsigned int)__popcll(b));
	}
	__syncthreads();
	if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// 8 lanes per entry i < n_plinks (the table is sorted; the records hold what k_red_rows wrote)
__global__ __launch_bounds__(256) void k_red_verdict(RedDev D)
{
	__shared__ unsigned int s_cnt[4];                              // KEPT, TRANSITIVE, COMPLEX, the rows enumerated
	if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = ((u64)blockIdx.x * 256 + threadIdx.x) >> 3;
	const u32 l = threadIdx.x & 7;
	const u64 R = 2 * D.n_plinks;
	const bool live = i < D.n_plinks && D.rrecs[i].verdict == RED_KEPT;   // eligible: only this group writes that word, behind this read
	u32 a = 0, c = 0;
	u64 bound = 0;
	if (live) {
		const PairLink E = D.plinks[i];
		a = E.a; c = E.b;
		const u32 o = (l & 2) ? (c ^ 1u) : a;                      // lanes 0, 1: out(a); lanes 2, 3: out(c ^ 1); the others repeat them
		bound = red_lower(D.skey, R, (u64)(o + (l & 1)) << 32);
	}
	const u64 lo_a = red_shfl(bound, 0), hi_a = red_shfl(bound, 1), lo_c = red_shfl(bound, 2), hi_c = red_shfl(bound, 3);
	const u64 r_a = hi_a - lo_a, r_c = hi_c - lo_c;
	const u32 side = r_a <= r_c ? 0 : 1;
	const u64 lo = side ? lo_c : lo_a, n_row = side ? r_c : r_a;
	const bool cplx = n_row > (u64)D.max_row;
	u32 n_via = 0;
	u64 best = ~0ULL;                                              // b << 32 | the row's place in out(.), counted from the end on side 1
	long long best_delta = 0;
	if (live && !cplx) {
		const long long g_i = D.rrecs[i].g;
		for (u64 r = l; r < n_row; r += 8) {
			const u32 dst = (u32)D.skey[lo + r];
			const u64 j = D.sval[lo + r] >> 1;
			const u32 b = side ? dst ^ 1u : dst;
			const u64 fkey = side ? (u64)a << 32 | b : (u64)b << 32 | c;
			const u64 p = red_lower(D.skey, R, fkey);
			if (p >= R || D.skey[p] != fkey) continue;
			const u64 f = D.sval[p] >> 1;
			if (j >= D.n_plinks || f >= D.n_plinks || (u64)(b >> 1) >= D.U) continue;
			const u64 sum = (u64)D.rrecs[j].g + red_m(D, b >> 1) + (u64)D.rrecs[f].g;
			const long long delta = (long long)((u64)g_i - sum);
			if (delta < -(long long)D.tol || delta > (long long)D.tol) continue;
			n_via++;
			const u64 t = (u64)b << 32 | (u32)(side ? n_row - 1 - r : r);
			if (t < best) { best = t; best_delta = delta; }
		}
	}
	for (int m = 1; m < 8; m <<= 1) {
		n_via += (u32)__shfl_xor((int)n_via, m, 8);
		const u64 ob = red_shfl_xor(best, m);
		const long long od = (long long)red_shfl_xor((u64)best_delta, m);
		if (ob < best) { best = ob; best_delta = od; }
	}
	if (i < D.n_plinks && l == 0) {
		u32 keep = 1;
		if (live) {
			const u32 v = cplx ? RED_COMPLEX : n_via ? RED_TRANSITIVE : RED_KEPT;
			PairReduce *Q = D.rrecs + i;
			Q->verdict = v; Q->via = n_via ? (u32)(best >> 32) : 0xFFFFFFFFu; Q->n_via = n_via; Q->side = side;
			Q->delta = n_via ? best_delta : 0;
			keep = v != RED_TRANSITIVE;
			atomicAdd(&s_cnt[v - RED_KEPT], 1u);
			if (!cplx && n_row) atomicAdd(&s_cnt[3], (unsigned int)n_row);
		}
		D.flag[i] = keep;
	}
	__syncthreads();
	if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(D.cnt + RED_KEPT + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// what the scan adds up: the flag of entry i as 64 bits, 0 at and behind n
struct RedFlag {
	const u32 *flag;
	u64 n;
	__host__ __device__ u64 operator()(u64 i) const { return i < n ? (u64)flag[i] : 0; }
};

// thread i < n_plinks (D.sc: the scanned flags; the host has seen that sc[n_plinks] <= D.cap)
__global__ __launch_bounds__(256) void k_red_compact(RedDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= D.n_plinks || !D.flag[i]) return;
	const u64 p = D.sc[i];
	if (p >= D.cap) return;
	if (D.lout) D.lout[p] = D.plinks[i];
	if (D.origin) D.origin[p] = (u32)i;
}
