// pair_kernels.h -- kmx_unitig_pair_walks*: the two mates of every read pair placed in the unitig graph (the rule: include/kmx.h;
// the host side: pair_host.h; the launcher: unitig_device.hip).  The kernels, in the order the launcher runs them:
//   k_pair_anchor    per walk: its read, by a search in walk_offsets; if it is a candidate, one 64-bit atomicMax of
//                    min(n_mapped, 2^32 - 1) << 32 | ~(index within the read) on the read's word (zero before: no candidate), so
//                    the largest n_mapped wins and a tie goes to the lowest index, in whatever order the lanes arrive;
//   k_pair_items     per entry of the input list: its key and its index, the first n_in work items of the fold;
//   k_pair_classify  per pair: two anchor words, two walk records, two steps, two m_u and one row of at most 4 entries: the class,
//                    the record, +1 on hist or pair_hits, the work item (its key PAIR_NO_KEY when the pair is no link) and the
//                    call's counters (summed in LDS, one atomic per block and counter);
//   (the work items sorted by key with their indices, and an exclusive scan of the key changes: unitig_device.hip)
//   k_pair_fold      per sorted work item: what it adds to the record of its run, as integer atomics, so no order shows;
//   k_pair_store     per merged record: into the caller's list, only where the merged count fits the capacity.
// No lane walks a read.  walk_offsets are clamped into [0, n_walks], a walk whose last step lies outside steps is no candidate,
// row bounds are clamped into [0, n_links], at most 4 entries of a row are read, and every store is checked against its capacity.
#pragma once
#include "kmx_types.h"

static constexpr u64 PAIR_NO_KEY = ~0ULL, PAIR_NO_WALK = ~0ULL;

__device__ __forceinline__ u64 pair_clamp(u64 x, u64 hi) { return x < hi ? x : hi; }

// the inner end (o, x) of walk w < n_walks if it is a candidate
__device__ __forceinline__ bool pair_inner(const PairDev &D, u64 w, u32 &o, u32 &x, u64 &n_mapped, u64 &n_span)
{
	const Walk *W = D.walks + w;
	n_mapped = W->n_mapped;
	const u64 fs = W->first_step, ns = W->n_steps;
	if (n_mapped < (u64)D.min_mapped || ns < 1) return false;
	const u64 at = fs + ns - 1;
	if (at < fs || at >= D.n_steps) return false;
	o = D.steps[at];
	if ((u64)o >= 2 * D.U) return false;
	x = W->off_last;
	if (x >= D.mu[o >> 1]) return false;
	n_span = W->n_span;
	return true;
}

// thread w < n_walks; n_seqs > 0
__global__ __launch_bounds__(256) void k_pair_anchor(PairDev D)
{
	const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
	if (w >= D.n_walks) return;
	u64 lo = 0, hi = D.n_seqs;                                       // the last read whose walks start at or in front of w
	while (hi - lo > 1) {
		const u64 mid = lo + (hi - lo) / 2;
		if (pair_clamp(D.wo[mid], D.n_walks) <= w) lo = mid; else hi = mid;
	}
	const u64 a = pair_clamp(D.wo[lo], D.n_walks), b = pair_clamp(D.wo[lo + 1], D.n_walks);
	if (w < a || w >= b || w - a >= 0xFFFFFFFFULL) return;
	u32 o, x;
	u64 nm, span;
	if (!pair_inner(D, w, o, x, nm, span)) return;
	const u64 word = (nm < 0xFFFFFFFFULL ? nm : 0xFFFFFFFFULL) << 32 | (u64)(u32)~(u32)(w - a);
	atomicMax(D.anchor + lo, (unsigned long long)word);
}

// thread i < n_in
__global__ __launch_bounds__(256) void k_pair_items(PairDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= D.n_in) return;
	D.key[i] = (u64)D.plinks[i].a << 32 | D.plinks[i].b;
	D.idx[i] = i;
}

// thread p < n_pairs
__global__ __launch_bounds__(256) void k_pair_classify(PairDev D)
{
	__shared__ unsigned int s_cnt[PAIR_C_N];
	if (threadIdx.x < PAIR_C_N) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
	if (p < D.n_pairs) {
		u64 wk[2] = {PAIR_NO_WALK, PAIR_NO_WALK}, span[2] = {0, 0};
		u32 o[2] = {0, 0}, x[2] = {0, 0};
#pragma unroll
		for (int s = 0; s < 2; s++) {
			const u64 word = D.anchor[2 * p + s];
			if (!word) continue;
			const u64 w = pair_clamp(D.wo[2 * p + s], D.n_walks) + (u64)(u32)~(u32)word;
			u64 nm;
			if (w < D.n_walks && pair_inner(D, w, o[s], x[s], nm, span[s])) wk[s] = w;
		}
		const bool pa = wk[0] != PAIR_NO_WALK, pb = wk[1] != PAIR_NO_WALK;
		if (!pa) o[0] = x[0] = 0;
		if (pb) { x[1] = D.mu[o[1] >> 1] - 1 - x[1]; o[1] ^= 1u; } else o[1] = x[1] = 0;
		Pair R{wk[0], wk[1], PAIR_NONE, 0xFFFFFFFFu, o[0], x[0], o[1], x[1], 0, 0, 0};
		u64 key = PAIR_NO_KEY;
		u32 dist = 0;
		if (!pa || !pb) {
			R.cls = pa || pb ? PAIR_SINGLE : PAIR_NONE;
			atomicAdd(&s_cnt[pa || pb ? PAIR_C_SINGLE : PAIR_C_NONE], 1u);
		} else if (o[0] == o[1]) {
			R.cls = PAIR_SAME;
			R.d = (long long)x[1] - (long long)x[0];
			R.frag = (long long)((u64)R.d + span[0] + span[1] + (u64)D.k - 2);
			atomicAdd(&s_cnt[PAIR_C_SAME], 1u);
			if (R.frag < 0) atomicAdd(&s_cnt[PAIR_C_NEGATIVE], 1u);
			else if (D.hist) {
				const u64 bin = (u64)R.frag / D.bin_width;
				atomicAdd(D.hist + (bin < D.n_bins ? bin : D.n_bins - 1), 1ULL);
			}
		} else if (o[0] == (o[1] ^ 1u)) {
			R.cls = PAIR_INVERTED;
			atomicAdd(&s_cnt[PAIR_C_INVERTED], 1u);
		} else {
			R.d = ((long long)D.mu[o[0] >> 1] - 1 - (long long)x[0]) + (long long)x[1];
			if (R.d > (long long)D.max_dist) {
				R.cls = PAIR_FAR;
				atomicAdd(&s_cnt[PAIR_C_FAR], 1u);
			} else {
				R.cls = PAIR_LINK;
				atomicAdd(&s_cnt[PAIR_C_LINK], 1u);
				const u64 lo = pair_clamp(D.loffs[o[0]], D.n_links), hi0 = pair_clamp(D.loffs[(u64)o[0] + 1], D.n_links);
				const u64 hi = hi0 > lo ? (hi0 - lo > 4 ? lo + 4 : hi0) : lo;
				u64 e = PAIR_NO_KEY;
				for (u64 t = lo; t < hi; t++)
					if (e == PAIR_NO_KEY && D.links[t] == o[1]) e = t;
				if (e != PAIR_NO_KEY) {
					R.edge = (u32)e;
					if (D.pair_hits) atomicAdd(D.pair_hits + e, 1ULL);
					atomicAdd(&s_cnt[PAIR_C_ADJACENT], 1u);
				}
				const u64 fw = (u64)o[0] << 32 | o[1], bw = (u64)(o[1] ^ 1u) << 32 | (o[0] ^ 1u);
				key = fw < bw ? fw : bw;
				dist = (u32)R.d;
			}
		}
		if (D.pairs) D.pairs[p] = R;
		if (D.n_items) {
			D.key[D.n_in + p] = key;
			D.idx[D.n_in + p] = D.n_in + p;
			D.dist[p] = dist;
		}
	}
	__syncthreads();
	if (threadIdx.x < PAIR_C_N && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// 1 where sorted item i opens a run of a key (i == n: nothing, so that the exclusive scan ends with the merged count)
struct PairKeyFlag {
	const u64 *skey;
	u64 n;
	__host__ __device__ u64 operator()(u64 i) const { return i < n && skey[i] != ~0ULL && (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0; }
};

// thread i < n_items: sorted item i into the record of its run (mrg is all zero before; min_dist is kept inverted)
__global__ __launch_bounds__(256) void k_pair_fold(PairDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= D.n_items) return;
	const u64 key = D.skey[i];
	if (key == PAIR_NO_KEY) return;
	const u64 run = D.sc[i + 1] - 1, j = D.sidx[i];                  // an item with a key lies in or behind the first run
	if (run >= D.n_items || j >= D.n_items) return;
	u64 n = 1, sum;
	u32 mn, mx;
	if (j < D.n_in) {
		const PairLink L = D.plinks[j];
		n = L.n_pairs; sum = L.sum_dist; mn = L.min_dist; mx = L.max_dist;
	} else
		sum = mn = mx = D.dist[j - D.n_in];
	PairLink *M = D.mrg + run;
	if (i == 0 || D.skey[i - 1] != key) { M->a = (u32)(key >> 32); M->b = (u32)key; }
	atomicAdd((unsigned long long *)&M->n_pairs, (unsigned long long)n);
	atomicAdd((unsigned long long *)&M->sum_dist, (unsigned long long)sum);
	atomicMax(&M->min_dist, ~mn);
	atomicMax(&M->max_dist, mx);
}

// thread i < min(n_items, cap)
__global__ __launch_bounds__(256) void k_pair_store(PairDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 tot = D.sc[D.n_items];
	if (tot > D.cap || i >= tot || i >= D.n_items) return;
	PairLink L = D.mrg[i];
	L.min_dist = ~L.min_dist;
	D.plinks[i] = L;
}
