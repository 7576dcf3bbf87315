// pair_path_kernels.h -- kmx_unitig_pair_paths*: the one graph path an entry of the pair list stands for, and the credit to its
// interior unitigs and edges (the rule: include/kmx.h; the host side: pair_path_host.h; the launchers: unitig_device.hip).  The
// kernels, in the order the host runs them:
//   k_pp_search   one lane per list entry: its class, its window bounds lo and hi, then a depth-first enumeration of the prefixes
//                 from a.  The stack is (oriented unitig, next row position) per level, at most 17 levels, and lies in LDS
//                 indexed [level][lane]: a private array under a running index would live in scratch memory on this target.  W
//                 is one register: a push adds m of the child, a pop subtracts it again.  A visit costs the two row bounds, at
//                 most 4 link loads for the hit test and two offsets for m; the rows of a small neighbourhood stay in the
//                 caches.  The first hit's steps go to work[i * max_steps ..]; the lane stops once its counter has passed
//                 max_visits, so no entry costs more than max_visits + 1 visits.  The seven verdict counters are summed per wave,
//                 then in LDS: one global atomic per block and counter;
//   (an exclusive scan of the PATH entries' n_steps: unitig_device.hip)
//   k_pp_apply    one lane per list entry: first_step; for a PATH its steps into psteps where they fit, one integer atomic per
//                 interior unitig into through and one per edge into path_hits, n_added and n_missing through LDS.
// Every row bound is clamped into [0, n_links], at most 4 entries of a row are read, an entry >= 2 U is neither matched nor
// extended, and every store is checked against its capacity: bad device input gives wrong paths, never an access outside a
// buffer.  The counts are those of the rule whatever the order of the search, so the bytes are a function of the input alone.
#pragma once
#include "resolve_kernels.h"

static constexpr int PP_LEVELS = PP_MAX_STEPS + 1;

// the clamped row of oriented unitig o < 2 U
__device__ __forceinline__ void pp_row(const PathDev &D, u64 o, u64 *lo, u32 *n)
{
	const u64 a = thr_min(D.loffs[o], D.n_links), b = thr_min(D.loffs[o + 1], D.n_links);
	*lo = a;
	*n = b > a ? (u32)thr_min(b - a, 4) : 0u;
}
// the index of t among the read entries of the row of o < 2 U (the first match), or 4; *lo: where the row starts
__device__ __forceinline__ u32 pp_find(const PathDev &D, u32 o, u32 t, u64 *lo)
{
	u32 n, at = 4;
	pp_row(D, o, lo, &n);
	for (u32 j = 0; j < n; j++)
		if (at == 4 && D.links[*lo + j] == t) at = j;
	return at;
}
// m_u of unitig u < U: its windows, 0 for what is shorter than k
__device__ __forceinline__ u64 pp_m(const PathDev &D, u64 u)
{
	const u64 a = D.uoffs[u], b = D.uoffs[u + 1];
	const u64 len = b > a ? b - a : 0;
	return len >= (u64)D.k ? len - (u64)D.k + 1 : 0;
}
__device__ __forceinline__ bool pp_is_link(const PathDev &D, const PairLink &E)
{
	return (u64)E.a < 2 * D.U && (u64)E.b < 2 * D.U && (E.a >> 1) != (E.b >> 1) && E.n_pairs >= 1;
}

// thread i < n_plinks
__global__ __launch_bounds__(256) void k_pp_search(PathDev D)
{
	__shared__ u32 s_node[PP_LEVELS][256];
	__shared__ unsigned char s_pos[PP_LEVELS][256];
	__shared__ unsigned int s_cnt[PP_COMPLEX + 1];
	const u32 tid = threadIdx.x;
	if (tid <= PP_COMPLEX) s_cnt[tid] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + tid;
	int verdict = -1;
	if (i < D.n_plinks) {
		const PairLink E = D.plinks[i];
		PairPath R{0, 0, 0, 0, 0, 0};
		if (!pp_is_link(D, E)) verdict = PP_IGNORED;
		else if (E.n_pairs < D.min_pairs) verdict = PP_BELOW_MIN;
		else {
			const u64 g = (u64)D.inner - 1 - E.sum_dist / E.n_pairs;    // signed 64-bit, wrapping like the scaffold's
			const long long lo = (long long)(g - D.tol), hi = (long long)(g + D.tol);
			verdict = PP_NO_PATH;
			if (hi >= 0) {
				const u32 max_steps = D.max_steps < PP_MAX_STEPS ? D.max_steps : PP_MAX_STEPS;
				u32 *const work = D.work + i * max_steps;
				u32 cnt = 0, hits = 0, level = 0, ht = 0;
				u64 W = 0, hW = 0;                                        // 0 <= W <= hi throughout
				// the prefix that ends at v on `level`: counted, and a hit iff b is in the row of v and W >= lo
				auto visit = [&](u32 v) {
					if (++cnt > D.max_visits) return false;
					u64 rlo;
					if ((long long)W >= lo && pp_find(D, v, E.b, &rlo) < 4) {
						if (!hits) {
							ht = level;
							hW = W;
							for (u32 j = 1; j <= level; j++) work[j - 1] = s_node[j][tid];
						}
						hits++;
					}
					return true;
				};
				s_node[0][tid] = E.a;
				s_pos[0][tid] = 0;
				bool ok = visit(E.a);
				while (ok) {
					const u32 v = s_node[level][tid], p = s_pos[level][tid];
					u64 rlo;
					u32 n;
					pp_row(D, v, &rlo, &n);
					if (level < max_steps && p < n) {
						s_pos[level][tid] = (unsigned char)(p + 1);
						const u32 c = D.links[rlo + p];
						if ((u64)c >= 2 * D.U) continue;
						const u64 mc = pp_m(D, c >> 1);
						if (mc > (u64)hi - W) continue;
						level++;
						s_node[level][tid] = c;
						s_pos[level][tid] = 0;
						W += mc;
						ok = visit(c);
					} else {
						if (!level) break;
						W -= pp_m(D, v >> 1);
						level--;
					}
				}
				if (!ok) { verdict = PP_COMPLEX; R.n_visited = D.max_visits + 1; }
				else {
					R.n_visited = cnt;
					R.n_hits = hits;
					if (hits >= 2) verdict = PP_AMBIGUOUS;
					else if (hits == 1) {
						verdict = ht ? PP_PATH : PP_ADJACENT;
						R.n_steps = ht;
						R.windows = hW;
					}
				}
			}
		}
		R.verdict = (u32)verdict;
		D.precs[i] = R;
	}
	for (int j = 0; j <= PP_COMPLEX; j++) {
		const u64 b = __ballot(verdict == j);
		if ((tid & 63) == 0 && b) atomicAdd(&s_cnt[j], (unsigned int)__popcll(b));
	}
	__syncthreads();
	if (tid <= PP_COMPLEX && s_cnt[tid]) atomicAdd(D.cnt + tid, (unsigned long long)s_cnt[tid]);
}

// what the scan adds up: the steps of entry i, for a PATH only; 0 at i == n (the scan ends with the total)
struct PairPathSteps {
	const PairPath *precs;
	u64 n;
	__host__ __device__ u64 operator()(u64 i) const { return i < n && precs[i].verdict == PP_PATH ? (u64)precs[i].n_steps : 0; }
};

// thread i < n_plinks (D.sc: the scanned steps)
__global__ __launch_bounds__(256) void k_pp_apply(PathDev D)
{
	__shared__ unsigned int s_cnt[2];
	const u32 tid = threadIdx.x;
	if (tid < 2) s_cnt[tid] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + tid;
	u32 added = 0, missing = 0;
	if (i < D.n_plinks) {
		const u32 verdict = D.precs[i].verdict;
		if (verdict == PP_PATH || verdict == PP_ADJACENT) D.precs[i].first_step = D.sc[i];
		if (verdict == PP_PATH) {
			const PairLink E = D.plinks[i];
			const u32 max_steps = D.max_steps < PP_MAX_STEPS ? D.max_steps : PP_MAX_STEPS;
			const u32 t = D.precs[i].n_steps < max_steps ? D.precs[i].n_steps : max_steps;
			const u32 *const work = D.work + i * max_steps;
			const u64 first = D.sc[i];
			u32 P = E.a, x = work[0];
			for (u32 j = 1; j <= t; j++) {
				const u32 N = j < t ? work[j] : E.b;
				if (D.psteps && first + j - 1 < D.cap) D.psteps[first + j - 1] = x;
				u32 in = 4, out = 4;
				u64 rlo = 0, plo = 0;
				const bool inside = (u64)x < 2 * D.U && (u64)P < 2 * D.U && (u64)N < 2 * D.U;
				if (inside) {
					in = pp_find(D, x ^ 1u, P ^ 1u, &rlo);
					out = pp_find(D, x, N, &rlo);
				}
				if (in != 4 && out != 4) {
					const u32 a = x & 1u ? out : in, b = x & 1u ? in : out;
					if (D.through) atomicAdd(D.through + 16 * (u64)(x >> 1) + 4 * a + b, (unsigned long long)E.n_pairs);
					added++;
				} else
					missing++;
				if (D.path_hits && inside) {
					const u32 e = pp_find(D, P, x, &plo);                  // the edge v_(j-1) -> v_j ...
					if (e != 4) atomicAdd(D.path_hits + plo + e, (unsigned long long)E.n_pairs);
					if (j == t && out != 4) atomicAdd(D.path_hits + rlo + out, (unsigned long long)E.n_pairs);   // ... and the last one, v_t -> b
				}
				P = x;
				x = N;
			}
		}
	}
	if (added) atomicAdd(&s_cnt[0], added);
	if (missing) atomicAdd(&s_cnt[1], missing);
	__syncthreads();
	if (tid < 2 && s_cnt[tid]) atomicAdd(D.cnt + PP_C_ADDED + tid, (unsigned long long)s_cnt[tid]);
}
