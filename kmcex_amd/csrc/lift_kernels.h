// lift_kernels.h -- kmx_unitig_pair_lift*: a unitig-level pair list in contig coordinates (the rule: include/kmx.h; the host side:
// lift_host.h; the launchers: unitig_device.hip).  The kernels, in the order the host runs them:
//   k_lift_classify  one lane per list entry: two place loads, two crec loads and four uoffsets loads give where its two oriented
//                    unitigs lie; the class and the record; the work item (its key LIFT_NO_KEY when the entry is no LINK, its
//                    index, and n, sum, lo, hi after the shift).  The call's counters are summed in LDS: one global atomic per
//                    block and counter;
//   (the launcher sorts the (key, index) pairs by key, stably, and scans the key changes)
//   k_lift_fold      per sorted work item.  After a lift many entries share a contig pair, so runs are long, and one atomic per
//                    item and field would queue a whole wavefront on one record.  The items are sorted, so the lanes of a
//                    wavefront that share a run are contiguous: a segmented reduction by shuffles (six steps over n, sum, min,
//                    max) leaves the run's part in the last lane of the segment, which alone issues the four integer atomics
//                    for that (wavefront, run).  Sums, minima and maxima of integers: the bytes do not depend on the order.
//                    k_lift_fold<LIFT_FOLD_PLAIN> is the lane-per-item fold of k_pair_fold, kept for the measurement;
//   k_lift_store     per sorted work item the index of its run into lrec[].out (from the scan: it needs no capacity), and per
//                    merged record its copy into lout, only where the merged count fits the capacity.
// No lane walks a run.  Every index read from the caller's arrays is checked where it is read (an end that is not placed makes
// the entry IGNORED), uoffsets are clamped into [0, n_ubases], and every store is checked against its capacity.
#pragma once
#include "kmx_types.h"

__device__ __forceinline__ u64 lift_min(u64 a, u64 b) { return a < b ? a : b; }

// where oriented unitig o < 2 U lies: false when it is not placed; else its oriented contig, start(o), tail(o) and m
__device__ __forceinline__ bool lift_end(const LiftDev &D, u32 o, u32 &O, long long &start, long long &tail, long long &m)
{
	const u64 u = o >> 1;
	const CtgPlace P = D.place[u];
	const u64 c = P.oc >> 1;
	if (c >= D.C) return false;
	const u64 M = D.crec[c].n_kmers;
	const u64 x = lift_min(D.uoffs[u], D.n_ubases), y = lift_min(D.uoffs[u + 1], D.n_ubases);
	const u64 len = y > x ? y - x : 0;
	const u64 mu = len >= (u64)D.k ? len - (u64)D.k + 1 : 0;
	if (M >> 32 || (u64)P.off + mu > M) return false;
	const u32 r = (o ^ P.oc) & 1u;
	O = (u32)(2 * c) | r;
	m = (long long)mu;
	start = r ? (long long)M - (long long)P.off - m : (long long)P.off;
	tail = (long long)M - start - m;
	return true;
}

// thread i < n_plinks
__global__ __launch_bounds__(256) void k_lift_classify(LiftDev D)
{
	__shared__ unsigned long long s_cnt[LIFT_C_N];
	if (threadIdx.x < LIFT_C_N) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < D.n_plinks) {
		const PairLink E = D.plinks[i];
		PairLift R{LIFT_IGNORED, 0xFFFFFFFFu, 0, 0, 0, 0, 0};
		PairLink W{0, 0, 0, 0, 0, 0};
		u64 key = LIFT_NO_KEY;
		u32 A = 0, B = 0;
		long long sa = 0, ta = 0, ma = 0, sb = 0, tb = 0, mb = 0;
		const bool link = (u64)E.a < 2 * D.U && (u64)E.b < 2 * D.U && (E.a >> 1) != (E.b >> 1) && E.n_pairs != 0;
		if (link && lift_end(D, E.a, A, sa, ta, ma) && lift_end(D, E.b, B, sb, tb, mb)) {
			R.A = A; R.B = B;
			if (A == B) {
				R.cls = LIFT_SAME;
				R.shift = sb - sa - ma + 1;
				if ((long long)E.min_dist + R.shift < 0) {
					atomicAdd(&s_cnt[LIFT_C_SAME_BACK], 1ULL);
					atomicAdd(&s_cnt[LIFT_C_PAIRS_SAME_BACK], (unsigned long long)E.n_pairs);
				} else
					atomicAdd(&s_cnt[LIFT_C_SUM_SAME_D], (unsigned long long)(E.sum_dist + E.n_pairs * (u64)R.shift));
			} else if (A == (B ^ 1u))
				R.cls = LIFT_INVERTED;
			else {
				R.shift = ta + sb;
				const long long lo = (long long)E.min_dist + R.shift, hi = (long long)E.max_dist + R.shift;
				if (lo > (long long)D.max_dist || hi >= (1LL << 32))
					R.cls = LIFT_FAR;
				else {
					R.cls = LIFT_LINK;
					const u64 fw = (u64)A << 32 | B, bw = (u64)(B ^ 1u) << 32 | (A ^ 1u);
					R.flipped = bw < fw;
					key = bw < fw ? bw : fw;
					W = PairLink{(u32)(key >> 32), (u32)key, E.n_pairs, E.sum_dist + E.n_pairs * (u64)R.shift, (u32)lo, (u32)hi};
				}
			}
		}
		atomicAdd(&s_cnt[R.cls], 1ULL);
		atomicAdd(&s_cnt[LIFT_C_PAIRS + R.cls], (unsigned long long)E.n_pairs);
		D.lrec[i] = R;
		D.key[i] = key;
		D.idx[i] = (u32)i;
		D.item[i] = W;
	}
	__syncthreads();
	if (threadIdx.x < LIFT_C_N && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, s_cnt[threadIdx.x]);
}

// 1 where sorted item i opens a run of a key (i == n: nothing, so that the exclusive scan ends with the merged count)
struct LiftKeyFlag {
	const u64 *skey;
	u64 n;
	__host__ __device__ u64 operator()(u64 i) const { return i < n && skey[i] != ~0ULL && (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0; }
};

__device__ __forceinline__ u64 lift_shfl_up(u64 v, unsigned d)
{
	return (u64)(u32)__shfl_up((int)(u32)(v >> 32), d) << 32 | (u32)__shfl_up((int)(u32)v, d);
}
__device__ __forceinline__ u64 lift_shfl_down(u64 v, unsigned d)
{
	return (u64)(u32)__shfl_down((int)(u32)(v >> 32), d) << 32 | (u32)__shfl_down((int)(u32)v, d);
}

// thread i < n_plinks rounded up to whole wavefronts: sorted item i into the record of its run (mrg is all zero before; min_dist
// is kept inverted).  Every lane of a wavefront takes part in the shuffles; a lane without an item carries the neutral element
template <int FOLD> __global__ __launch_bounds__(256) void k_lift_fold(LiftDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 E = D.n_plinks;
	u64 key = LIFT_NO_KEY, run = E, n = 0, sum = 0;
	u32 inv = 0, mx = 0;
	if (i < E) {
		key = D.skey[i];
		const u64 j = D.sidx[i];
		if (key != LIFT_NO_KEY && j < E) {
			run = D.sc[i + 1] - 1;                                   // an item with a key lies in or behind the first run
			const PairLink W = D.item[j];
			n = W.n_pairs; sum = W.sum_dist; inv = ~W.min_dist; mx = W.max_dist;
		}
	}
	bool last = true;
	u64 before = LIFT_NO_KEY;                                      // the key in front of this item
	if (FOLD == LIFT_FOLD_WAVE) {
		const u32 lane = threadIdx.x & 63;
		before = lift_shfl_up(key, 1);
		const u64 behind = lift_shfl_down(key, 1);
		bool head = lane == 0 || before != key;
		last = lane == 63 || behind != key;
#pragma unroll
		for (unsigned d = 1; d < 64; d <<= 1) {
			const u64 on = lift_shfl_up(n, d), os = lift_shfl_up(sum, d);
			const u32 oi = (u32)__shfl_up((int)inv, d), om = (u32)__shfl_up((int)mx, d);
			const int oh = __shfl_up((int)head, d);
			if (lane >= d && !head) {
				n += on; sum += os;
				inv = oi > inv ? oi : inv; mx = om > mx ? om : mx;
				head = oh != 0;
			}
		}
		if (lane == 0) before = i && i < E ? D.skey[i - 1] : LIFT_NO_KEY;
	} else
		before = i && i < E ? D.skey[i - 1] : LIFT_NO_KEY;
	if (key == LIFT_NO_KEY || run >= E) return;
	PairLink *M = D.mrg + run;
	if (i == 0 || before != key) { M->a = (u32)(key >> 32); M->b = (u32)key; }
	if (!last) return;
	atomicAdd((unsigned long long *)&M->n_pairs, (unsigned long long)n);
	atomicAdd((unsigned long long *)&M->sum_dist, (unsigned long long)sum);
	atomicMax(&M->min_dist, inv);
	atomicMax(&M->max_dist, mx);
}

// thread i < n_plinks (D.sc: the scanned key changes, D.mrg: the folded records)
__global__ __launch_bounds__(256) void k_lift_store(LiftDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 E = D.n_plinks;
	if (i >= E) return;
	const u64 tot = D.sc[E];
	if (D.skey[i] != LIFT_NO_KEY) {
		const u64 j = D.sidx[i];
		if (j < E) D.lrec[j].out = (u32)(D.sc[i + 1] - 1);
	}
	if (!D.lout || tot > D.cap || i >= tot) return;
	PairLink L = D.mrg[i];
	L.min_dist = ~L.min_dist;
	D.lout[i] = L;
}
