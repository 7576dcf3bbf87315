// resolve_kernels.h -- kmx_unitig_walk_through*: the reads per (way in, way out) of every unitig, counted from the walks (the rule:
// include/kmx.h; the host side: resolve_host.h; the launcher: unitig_device.hip).  The kernels, in the order the launcher runs them:
//   k_thr_mark     per walk: the byte of its first step becomes 1 (the bytes, n_steps + 1 of them, are zero before);
//   k_thr_count    per step: it is interior iff neither its own byte nor the next one is set and it is neither the first nor the
//                  last step of the array.  An interior step reads its two neighbours and two rows of the CSR, at most 4 entries
//                  each, and issues one atomicAdd; the call's three counters are summed in LDS, one atomic per block and counter.
// Every decision looks at one step, its two neighbours and two rows, so the result is a function of (walks, steps, CSR) alone.  No
// lane walks a read, a walk or a unitig.  first_step is clamped into [0, n_steps], row bounds into [0, n_links], and a step
// >= 2 U has no row looked up and adds nothing: bad input gives wrong counts, never an access outside a buffer.
#pragma once
#include "kmx_types.h"

static constexpr u32 THR_NONE = 4;

__device__ __forceinline__ u64 thr_min(u64 a, u64 b) { return a < b ? a : b; }

// the index of t among the first 4 entries of the row of oriented unitig o < 2 U (the first match), or THR_NONE
__device__ __forceinline__ u32 thr_find(const ThroughDev &D, u32 o, u32 t)
{
	const u64 lo = thr_min(D.loffs[o], D.n_links), hi0 = thr_min(D.loffs[(u64)o + 1], D.n_links);
	const u64 hi = hi0 > lo ? (hi0 - lo > 4 ? lo + 4 : hi0) : lo;
	u32 at = THR_NONE;
	for (u64 e = lo; e < hi; e++)
		if (at == THR_NONE && D.links[e] == t) at = (u32)(e - lo);
	return at;
}

// thread w < n_walks
__global__ __launch_bounds__(256) void k_thr_mark(ThroughDev D)
{
	const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
	if (w < D.n_walks) D.mark[thr_min(D.walks[w].first_step, D.n_steps)] = 1;
}

// thread i < n_steps: step x = steps[i] between P = steps[i - 1] and N = steps[i + 1]
__global__ __launch_bounds__(256) void k_thr_count(ThroughDev D)
{
	__shared__ unsigned int s_cnt[THR_C_N];
	if (threadIdx.x < THR_C_N) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > 0 && i + 1 < D.n_steps && !D.mark[i] && !D.mark[i + 1]) {
		const u32 x = D.steps[i], P = D.steps[i - 1], N = D.steps[i + 1];
		u32 in = THR_NONE, out = THR_NONE;
		if ((u64)x < 2 * D.U && (u64)P < 2 * D.U && (u64)N < 2 * D.U) {
			in = thr_find(D, x ^ 1u, P ^ 1u);
			out = thr_find(D, x, N);
		}
		atomicAdd(&s_cnt[THR_C_INTERIOR], 1u);
		if (in != THR_NONE && out != THR_NONE) {
			const u32 a = x & 1u ? out : in, b = x & 1u ? in : out;
			atomicAdd(D.through + 16 * (u64)(x >> 1) + 4 * a + b, 1ULL);
			atomicAdd(&s_cnt[THR_C_ADDED], 1u);
		} else
			atomicAdd(&s_cnt[THR_C_MISSING], 1u);
	}
	__syncthreads();
	if (threadIdx.x < THR_C_N && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// ---- kmx_unitig_resolve*: a unitig whose through hits pair its ways in with its ways out one to one is split into one copy per
// way in.  The kernels, in the order the host runs them:
//   k_res_bad      one lane per oriented unitig: an edge with a target >= 2 U or without its mirror marks both its ends (bytes,
//                  zero before), so that neither is resolved and the renaming below never looks for an index that is not there;
//   k_res_verdict  one lane per unitig: its two rows, its 128 bytes of through (16-byte loads), the verdict: the copy count with pi
//                  packed above it, and what the scan adds up: copies, bytes, edges.  The five counters are summed in LDS;
//   (an exclusive scan of the triples: unitig_device.hip; the host waits for its totals and the counters)
//   k_res_place    one lane per input unitig: rplace, and origin, roffsets, records and the two row starts of its <= 4 copies;
//   k_res_rows     one lane per input oriented unitig: its <= 4 edges, each renamed at both ends (the target's copy from the
//                  mirror lookup in a row of 4) and stored once, with link_origin and the hits;
//   k_res_emit     THE BYTES.  k_ctg_emit's tiling of the flat input, the tile's unitig boundaries in LDS; every piece is stored
//                  once per copy as aligned 16-byte words: read once, written p times, no reverse step.
// Every index read from the caller's arrays is clamped where it is read and every store is checked against its capacity.
#include "contig_kernels.h"

enum { RES_TILE = CTG_TILE, RES_NB = CTG_NB };

__device__ __forceinline__ void res_row(const ResDev &D, u64 o, u64 *lo, u32 *n)
{
	const u64 a = thr_min(D.loffs[o], D.n_links), b = thr_min(D.loffs[o + 1], D.n_links);
	*lo = a;
	*n = b > a ? (u32)thr_min(b - a, 4) : 0u;
}
// the index of t in the row of oriented unitig o < 2 U (the first match), or 4
__device__ __forceinline__ u32 res_find(const ResDev &D, u32 o, u32 t)
{
	u64 lo;
	u32 n, at = 4;
	res_row(D, o, &lo, &n);
	for (u32 j = 0; j < n; j++)
		if (at == 4 && D.links[lo + j] == t) at = j;
	return at;
}
__device__ __forceinline__ u64 res_len(const ResDev &D, u64 u)
{
	const u64 a = thr_min(D.uoffs[u], D.n_ubases), b = thr_min(D.uoffs[u + 1], D.n_ubases);
	return b > a ? b - a : 0;
}
__device__ __forceinline__ u32 res_pi(u32 ver, u32 a) { return (ver >> (8 + 2 * a)) & 3u; }
// the a with pi(a) == b (a resolved unitig has one)
__device__ __forceinline__ u32 res_inv(u32 ver, u32 b)
{
	u32 at = 0;
	for (u32 a = 0; a < (ver & 7u); a++)
		if (res_pi(ver, a) == b) at = a;
	return at;
}

// thread o < 2 U (D.bad is zero before)
__global__ __launch_bounds__(256) void k_res_bad(ResDev D)
{
	const u64 o = (u64)blockIdx.x * 256 + threadIdx.x;
	if (o >= 2 * D.U) return;
	u64 lo;
	u32 n;
	res_row(D, o, &lo, &n);
	for (u32 j = 0; j < n; j++) {
		const u32 t = D.links[lo + j];
		if ((u64)t >= 2 * D.U) D.bad[o >> 1] = 1;
		else if (res_find(D, t ^ 1u, (u32)o ^ 1u) == 4) { D.bad[o >> 1] = 1; D.bad[t >> 1] = 1; }
	}
}

// thread u <= U: ver[u] and tot[u] = (copies, their bytes, their edges); tot[U] = 0, so that the exclusive scan ends with the totals
__global__ __launch_bounds__(256) void k_res_verdict(ResDev D, CtgTot *tot)
{
	__shared__ unsigned int s_cnt[RES_C_N];
	if (threadIdx.x < RES_C_N) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	if (u <= D.U) {
		CtgTot t{0, 0, 0};
		if (u < D.U) {
			u64 rl, ll;
			u32 q, p, copies = 1, pi = 0;
			res_row(D, 2 * u, &rl, &q);
			res_row(D, 2 * u + 1, &ll, &p);
			bool cand = p == q && p >= 2 && !D.bad[u];
			for (u32 j = 0; j < q; j++) cand = cand && (u64)(D.links[rl + j] >> 1) != u;
			for (u32 j = 0; j < p; j++) cand = cand && (u64)(D.links[ll + j] >> 1) != u;
			if (cand) {
				u64 T[16];
				const u64 *tp = D.through + 16 * u;
				if (((size_t)tp & 15) == 0) {
#pragma unroll
					for (int i = 0; i < 8; i++) {
						const ulonglong2 v = ((const ulonglong2 *)tp)[i];
						T[2 * i] = v.x;
						T[2 * i + 1] = v.y;
					}
				} else {
#pragma unroll
					for (int i = 0; i < 16; i++) T[i] = tp[i];
				}
				bool crossed = false, one = true;
				u32 nsup = 0, colc = 0;                                // colc: a byte per column
#pragma unroll
				for (u32 a = 0; a < 4; a++) {
					u32 rowc = 0;
#pragma unroll
					for (u32 b = 0; b < 4; b++) {
						const u64 c = T[4 * a + b];
						if (a < p && b < p) {
							if (c >= D.min_reads && c >= 1) { rowc++; colc += 1u << (8 * b); pi |= b << (2 * a); }
							else if (c > D.max_cross) crossed = true;
						}
					}
					nsup += rowc;
					if (a < p && rowc != 1) one = false;
				}
#pragma unroll
				for (u32 b = 0; b < 4; b++)
					if (b < p && ((colc >> (8 * b)) & 0xFFu) != 1) one = false;
				const int kind = crossed ? RES_C_CROSSED : (!nsup ? RES_C_UNSUPPORTED : (one ? RES_C_RESOLVED : RES_C_AMBIGUOUS));
				if (kind == RES_C_RESOLVED) copies = p; else pi = 0;
				atomicAdd(&s_cnt[RES_C_CANDIDATES], 1u);
				atomicAdd(&s_cnt[kind], 1u);
			}
			D.ver[u] = copies | pi << 8;
			t = CtgTot{copies, copies * res_len(D, u), copies > 1 ? 2 * (u64)copies : (u64)p + q};
		}
		tot[u] = t;
	}
	__syncthreads();
	if (threadIdx.x < RES_C_N && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// thread u <= U (D.sc: the scanned triples)
__global__ __launch_bounds__(256) void k_res_place(ResDev D)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	if (u > D.U) return;
	const CtgTot at = D.sc[u];
	if (u == D.U) {
		if (at.n <= D.rec_cap) { D.roffs[at.n] = at.len; D.rloffs[2 * at.n] = at.steps; }
		return;
	}
	const u32 ver = D.ver[u], copies = ver & 7u;
	const u64 len = res_len(D, u);
	u64 rl;
	u32 q;
	res_row(D, 2 * u, &rl, &q);
	D.rplace[u] = ResPlace{(u32)at.n, copies};
	for (u32 c = 0; c < copies; c++) {
		const u64 n = at.n + c;
		if (n >= D.rec_cap) continue;
		D.origin[n] = (u32)u;
		D.roffs[n] = at.len + c * len;
		D.rloffs[2 * n] = copies > 1 ? at.steps + 2 * c : at.steps;
		D.rloffs[2 * n + 1] = copies > 1 ? at.steps + 2 * c + 1 : at.steps + q;
		if (D.rrec) {
			Unitig r = D.urec[u];
			if (copies > 1) r.n_pred = r.n_succ = 1;
			D.rrec[n] = r;
		}
	}
}

// the new name of the target t of an edge out of oriented unitig o
__device__ __forceinline__ u32 res_target(const ResDev &D, u32 o, u32 t)
{
	if ((u64)t >= 2 * D.U) return t;                               // no edge: o's unitig is unresolved, the entry stays what it is
	const u32 v = t >> 1, dt = t & 1u, vv = D.ver[v], cv = vv & 7u;
	const u32 first = (u32)D.sc[v].n;
	if (cv == 1) return 2 * first + dt;
	u32 i = res_find(D, t ^ 1u, o ^ 1u);
	if (i >= cv) i = 0;                                            // (k_res_bad left no resolved target without the mirror)
	return 2 * (first + (dt ? res_inv(vv, i) : i)) + dt;
}

// thread o < 2 U
__global__ __launch_bounds__(256) void k_res_rows(ResDev D)
{
	const u64 o = (u64)blockIdx.x * 256 + threadIdx.x;
	if (o >= 2 * D.U) return;
	const u64 u = o >> 1;
	const u32 d = (u32)o & 1u, ver = D.ver[u], copies = ver & 7u;
	const CtgTot at = D.sc[u];
	u64 lo, rl;
	u32 n, q;
	res_row(D, o, &lo, &n);
	res_row(D, 2 * u, &rl, &q);
	const u32 m = copies > 1 ? copies : n;
	for (u32 c = 0; c < m; c++) {
		const u32 j = copies > 1 ? (d ? c : res_pi(ver, c)) : c;
		const u64 E = copies > 1 ? at.steps + 2 * c + d : at.steps + (d ? q : 0) + c;
		if (j >= n || E >= D.n_links) continue;
		D.rlinks[E] = res_target(D, (u32)o, D.links[lo + j]);
		D.lorigin[E] = lo + j;
		if (D.rhits) D.rhits[E] = D.hits[lo + j];
	}
}

// piece i of the tile [t0, t1), copy c: the bytes of unitig u0 + i that lie in the tile go to rseq[d0, d1); the byte at d0 is s_in[x0]
__device__ __forceinline__ bool res_piece(const u64 *s_off, const u64 *s_base, const unsigned char *s_cp, u32 i, u32 c, u64 t0, u64 t1, u64 *d0, u64 *d1, u32 *x0)
{
	const u64 so = s_off[i], eo = s_off[i + 1];
	if (eo <= so || c >= s_cp[i]) return false;
	const u64 a = ctg_max(so, t0), b = ctg_min(eo, t1);
	if (b <= a) return false;
	const u64 base = s_base[i] + (u64)c * (eo - so);
	*d0 = base + (a - so); *d1 = base + (b - so); *x0 = (u32)(a - t0);
	return true;
}

// one block per tile of RES_TILE input bytes
__global__ __launch_bounds__(256) void k_res_emit(ResDev D)
{
	__shared__ __align__(16) unsigned char s_in[RES_TILE + 16];    // (a word is read behind the last byte)
	__shared__ u64 s_off[RES_NB + 1];
	__shared__ u64 s_base[RES_NB];
	__shared__ unsigned char s_cp[RES_NB];
	__shared__ u32 s_pre[RES_NB + 1];
	__shared__ u32 s_part[256];
	__shared__ u64 s_u0;
	__shared__ u32 s_nseg, s_maxc;
	const u32 tid = threadIdx.x;
	const u64 t0 = (u64)blockIdx.x * RES_TILE, t1 = ctg_min(t0 + RES_TILE, D.n_ubases);
	{
		const u64 p = t0 + (u64)tid * 16;
		if (((size_t)D.useq & 15) == 0 && p + 16 <= D.n_ubases) *(uint4 *)(s_in + tid * 16) = *(const uint4 *)(D.useq + p);
		else
			for (u32 b = 0; b < 16; b++) s_in[tid * 16 + b] = p + b < D.n_ubases ? D.useq[p + b] : (unsigned char)0;
	}
	if (tid < 16) s_in[RES_TILE + tid] = 0;
	if (tid == 0) {                                              // the tile's first unitig: the last one that starts at or in front of t0
		u64 lo = 0, hi = D.U;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (ctg_min(D.uoffs[mid], D.n_ubases) <= t0) lo = mid + 1; else hi = mid;
		}
		s_u0 = lo ? lo - 1 : 0;
		s_nseg = 0;
		s_maxc = 0;
	}
	__syncthreads();
	const u64 u0 = s_u0;
	for (u32 i = tid; i <= RES_NB; i += 256) {
		const u64 u = u0 + i, off = u <= D.U ? ctg_min(D.uoffs[u], D.n_ubases) : D.n_ubases;
		s_off[i] = off;
		if (i < RES_NB) {
			const u32 cp = u < D.U ? D.ver[u] & 7u : 0u;
			s_base[i] = u < D.U ? D.sc[u].len : 0;
			s_cp[i] = (unsigned char)cp;
			if (u < D.U && off < t1) { atomicMax(&s_nseg, i + 1); atomicMax(&s_maxc, cp); }
		}
	}
	__syncthreads();
	const u32 nseg = s_nseg, maxc = s_maxc < 4 ? s_maxc : 4;
	const bool wide = ((size_t)D.rseq & 15) == 0;
	for (u32 c = 0; c < maxc; c++) {                             // (the same for every lane of the block)
		u32 wn[4], sum = 0;                                        // the aligned 16-byte output words each of this lane's 4 pieces touches
		for (u32 j = 0; j < 4; j++) {
			const u32 i = 4 * tid + j;
			u64 d0, d1;
			u32 x0;
			wn[j] = i < nseg && res_piece(s_off, s_base, s_cp, i, c, t0, t1, &d0, &d1, &x0) ? (u32)(((d1 + 15) >> 4) - (d0 >> 4)) : 0;
			sum += wn[j];
		}
		s_part[tid] = sum;
		__syncthreads();
		for (u32 d = 1; d < 256; d <<= 1) {
			const u32 v = tid >= d ? s_part[tid - d] : 0;
			__syncthreads();
			s_part[tid] += v;
			__syncthreads();
		}
		u32 run = s_part[tid] - sum;
		for (u32 j = 0; j < 4; j++) { s_pre[4 * tid + j] = run; run += wn[j]; }
		if (tid == 255) s_pre[RES_NB] = run;
		__syncthreads();
		const u32 total = s_pre[RES_NB];
		for (u32 w = tid; w < total; w += 256) {
			u32 lo = 0, hi = RES_NB;                                 // the last piece with s_pre[i] <= w: the one word w belongs to
			while (lo < hi) {
				const u32 mid = (lo + hi) >> 1;
				if (s_pre[mid] <= w) lo = mid + 1; else hi = mid;
			}
			const u32 i = lo - 1;
			u64 d0, d1;
			u32 x0;
			if (!res_piece(s_off, s_base, s_cp, i, c, t0, t1, &d0, &d1, &x0)) continue;
			const u64 A = ((d0 >> 4) + (w - s_pre[i])) << 4;
			u32 word[4];
			bool full[4];
			for (u32 g = 0; g < 4; g++) {
				u32 v = 0;
				full[g] = A + 4 * g >= d0 && A + 4 * g + 4 <= d1;
				if (full[g]) {                                       // four bytes of the tile from two aligned words of it
					const u32 x = x0 + (u32)(A + 4 * g - d0), y = x & (RES_TILE - 4);
					const u64 two = (u64)*(const u32 *)(s_in + y + 4) << 32 | *(const u32 *)(s_in + y);
					word[g] = (u32)(two >> (8 * (x & 3)));
					continue;
				}
				for (u32 b = 0; b < 4; b++) {
					const u64 d = A + 4 * g + b;
					if (d >= d0 && d < d1) v |= (u32)s_in[(x0 + (u32)(d - d0)) & (RES_TILE - 1)] << (8 * b);
				}
				word[g] = v;
			}
			if (wide && full[0] && full[1] && full[2] && full[3] && A + 16 <= D.seq_cap) {
				*(uint4 *)(D.rseq + A) = make_uint4(word[0], word[1], word[2], word[3]);
				continue;
			}
			for (u32 g = 0; g < 4; g++) {
				if (wide && full[g] && A + 4 * g + 4 <= D.seq_cap) { *(u32 *)(D.rseq + A + 4 * g) = word[g]; continue; }
				for (u32 b = 0; b < 4; b++) {
					const u64 d = A + 4 * g + b;
					if (d >= d0 && d < d1 && d < D.seq_cap) D.rseq[d] = (unsigned char)(word[g] >> (8 * b));
				}
			}
		}
		__syncthreads();                                           // s_part and s_pre are written again for the next copy
	}
}
