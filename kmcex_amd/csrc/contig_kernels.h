// contig_kernels.h -- kmx_unitig_contigs*: contigs from the read-supported edges between unitigs (the rule: include/kmx.h; the
// host side: contig_host.h; the launchers: unitig_device.hip).  The construction of unitig_kernels.h one level up: the items are
// the 2 U oriented unitigs o = 2 u + d, not the 2 n oriented k-mers.  The kernels, in the order the host runs them:
//   k_ctg_sup     one lane per oriented unitig: the support of its at most 4 edges (its own hits plus those of the mirror edge,
//                 looked up in the row of t ^ 1) and best(o);
//   k_ctg_keep    one lane per oriented unitig: the verdict of each of its edges from its support and the two bests (these are
//                 complete only after k_ctg_sup, hence two launches), the kept count and the only kept target with its support;
//                 the four edge counters are summed in LDS, one global atomic per block and counter;
//   k_ctg_init    per oriented unitig the chain link in -> the rank state: a pointer, a rank in steps and a rank in k-mers;
//   k_ctg_round   one round of pointer doubling that carries both ranks and the running minimum of the unitig index;
//   k_ctg_cut     what has not settled lies on a cycle: cut in front of its smallest unitig as stored (k_uni_cut's logic);
//   k_ctg_mark    per unitig: (1, bytes, steps) where a contig starts, to be scanned;
//   k_ctg_rec_init, k_ctg_place   per unitig: its step, its place, its share of the contig's record (integer atomics), where
//                 its bytes go; at a contig's first step the rest of the record, coffsets, and the kept edges at the two ends;
//   k_ctg_emit    THE BYTES.  A block takes a tile of CTG_TILE flat input bytes: wide loads into LDS, the tile's first unitig by
//                 one binary search, the offsets and destinations of the unitigs that start in the tile into LDS, a scan of the
//                 output words each of these pieces covers, then one lane per aligned 16-byte output word: forward pieces are
//                 copies, reverse pieces are read backwards and complemented, and either way a wave stores consecutive aligned
//                 words.  No lane's work grows with the length of a unitig or of a contig.  Its body is ctg_emit_tile, which
//                 k_scf_emit (scaffold_kernels.h) runs with nothing skipped and another capacity;
//   k_ctg_clinks  after the scan of the end counts: one lane per oriented contig writes its row of the contig graph.
// Every index read from the caller's arrays is clamped where it is read and every store is checked against its capacity: bad
// device input gives wrong contigs, never an access outside a buffer.  The chain link is tested from both sides, so whatever
// the input the links form mirror-paired paths and cycles and the doubling ends within its bounded number of rounds.
#pragma once
#include "kmx_types.h"

static constexpr u32 CTG_NONE = 0xFFFFFFFFu;
static constexpr int CTG_TILE = 4096;                          // input bytes per block of k_ctg_emit
static constexpr int CTG_NB = 1024;                            // unitigs that start in a tile: at most CTG_TILE / 5 + 1 for a valid set
static constexpr u64 CTG_REV = 1ULL << 63, CTG_FIRST = 1ULL << 62;   // flags of ubase[u] above the destination

__device__ __forceinline__ u64 ctg_min(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 ctg_max(u64 a, u64 b) { return a > b ? a : b; }
// the row of oriented unitig o < 2 U: bounds clamped into [0, n_links], at most 4 entries
__device__ __forceinline__ void ctg_row(const CtgDev &D, u64 o, u64 *lo, u64 *hi)
{
	const u64 a = ctg_min(D.loffs[o], D.n_links), b = ctg_min(D.loffs[o + 1], D.n_links);
	*lo = a;
	*hi = b > a ? (b - a > 4 ? a + 4 : b) : a;
}
// the k-mers of unitig u < U from the clamped offsets; 0 for what is shorter than k
__device__ __forceinline__ u64 ctg_m(const CtgDev &D, u64 u)
{
	const u64 a = ctg_min(D.uoffs[u], D.n_ubases), b = ctg_min(D.uoffs[u + 1], D.n_ubases);
	const u64 len = b > a ? b - a : 0;
	return len >= (u64)D.k ? len - (u64)D.k + 1 : 0;
}
// sup * ratio < best, the product in 128 bits
__device__ __forceinline__ bool ctg_lt(u64 sup, u32 ratio, u64 best) { return __umul64hi(sup, (u64)ratio) == 0 && sup * (u64)ratio < best; }

// thread o < 2 U
__global__ __launch_bounds__(256) void k_ctg_sup(CtgDev D)
{
	const u64 o = (u64)blockIdx.x * 256 + threadIdx.x;
	if (o >= 2 * D.U) return;
	u64 lo, hi, best = 0;
	ctg_row(D, o, &lo, &hi);
	for (u64 e = lo; e < hi; e++) {
		const u32 t = D.links[e];
		u64 s = 0;
		if ((u64)t < 2 * D.U) {
			s = D.hits[e];
			u64 ml, mh, f = ~0ULL;
			ctg_row(D, t ^ 1u, &ml, &mh);
			for (u64 g = ml; g < mh; g++)
				if (f == ~0ULL && D.links[g] == ((u32)o ^ 1u)) f = g;
			if (f != ~0ULL && f != e) s += D.hits[f];              // a self-mirror edge counts once; no mirror: its own hits
			best = ctg_max(best, s);
		}
		D.esup[e] = s;
	}
	D.best[o] = best;
}

// thread o < 2 U
__global__ __launch_bounds__(256) void k_ctg_keep(CtgDev D)
{
	__shared__ unsigned int s_cnt[4];
	if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 o = (u64)blockIdx.x * 256 + threadIdx.x;
	if (o < 2 * D.U) {
		u64 lo, hi, os = 0;
		u32 nk = 0, ot = CTG_NONE, c[4] = {0, 0, 0, 0};
		ctg_row(D, o, &lo, &hi);
		const u64 bo = D.best[o];
		for (u64 e = lo; e < hi; e++) {
			const u32 t = D.links[e];
			unsigned char keep = 0;
			if ((u64)t < 2 * D.U) {                                // a target >= 2 U is no edge
				const u64 s = D.esup[e];
				c[CTG_C_LINKS]++;
				if (s < D.min_reads) c[CTG_C_BELOW_MIN]++;
				else if (D.ratio && (ctg_lt(s, D.ratio, bo) || ctg_lt(s, D.ratio, D.best[t ^ 1u]))) c[CTG_C_BELOW_RATIO]++;
				else { keep = 1; c[CTG_C_KEPT]++; nk++; ot = t; os = s; }
			}
			D.ekeep[e] = keep;
		}
		D.nk[o] = (unsigned char)nk;
		D.only[o] = nk == 1 ? ot : CTG_NONE;
		D.supo[o] = nk == 1 ? os : 0;
		for (int j = 0; j < 4; j++)
			if (c[j]) atomicAdd(&s_cnt[j], c[j]);
	}
	__syncthreads();
	if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// the chain link into oriented unitig x < 2 U, or CTG_NONE: p -> x iff outK[p] = {x}, outK[x ^ 1] = {p ^ 1} (the mirror side,
// which is inK[x] = {p}) and x != p ^ 1.  Tested from both sides, so p -> x iff (x ^ 1) -> (p ^ 1) whatever the input.
__device__ __forceinline__ u32 ctg_link_in(const CtgDev &D, u32 x)
{
	const u32 y = x ^ 1u;
	if (D.nk[y] != 1) return CTG_NONE;
	const u32 t = D.only[y];
	if ((u64)t >= 2 * D.U || t == x) return CTG_NONE;              // y -> y ^ 1 is a hairpin
	const u32 p = t ^ 1u;
	if (D.nk[p] != 1 || D.only[p] != x) return CTG_NONE;
	return p;
}

// thread x < 2 U
__global__ __launch_bounds__(256) void k_ctg_init(CtgDev D, CtgRank *rank, u32 *mn)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	bool link = false;
	if (x < 2 * D.U) {
		const u32 p = ctg_link_in(D, (u32)x);
		link = p != CTG_NONE;
		rank[x] = link ? CtgRank{p, 1, ctg_m(D, p >> 1)} : CtgRank{(u32)x, 0, 0};
		mn[x] = (u32)(x >> 1);
	}
	const u64 b = __ballot(link);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(D.cnt + CTG_C_CHAIN, (unsigned long long)__popcll(b));
}

// k_uni_round with two ranks: a head has steps == 0; step ranks on a cycle saturate, so nothing on a cycle ever looks like one
__global__ __launch_bounds__(256) void k_ctg_round(const CtgRank *pin, const u32 *mnin, CtgRank *pout, u32 *mnout, u64 n2, u32 *moved)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	if (x >= n2) return;
	const CtgRank a = pin[x];
	CtgRank o = a;
	u32 m = mnin ? mnin[x] : 0;
	if (a.steps != 0 && a.ptr < n2) {
		const CtgRank b = pin[a.ptr];
		if (b.steps != 0) {
			const u64 s = (u64)a.steps + b.steps;
			o = CtgRank{b.ptr, s > 0xFFFFFFFFULL ? 0xFFFFFFFFu : (u32)s, a.kmers + b.kmers};
			if (mnin) { const u32 mp = mnin[a.ptr]; m = mp < m ? mp : m; }
			*moved = 1;
		}
	}
	pout[x] = o;
	if (mnout) mnout[x] = m;
}

// after the last round: what has not settled lies on a cycle whose smallest unitig is mn[x]
__global__ __launch_bounds__(256) void k_ctg_cut(CtgDev D, const CtgRank *pin, const u32 *mnin, CtgRank *pout)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	if (x >= 2 * D.U) return;
	const CtgRank a = pin[x];
	if (a.steps == 0 || (u64)a.ptr >= 2 * D.U || pin[a.ptr].steps == 0) { pout[x] = a; return; }   // a head, or its pointer is one: settled
	const u32 s = 2 * mnin[x];                                   // the representative starts here ...
	u32 in = ctg_link_in(D, (u32)x);
	if ((u32)x == s || in == (s ^ 1u)) in = CTG_NONE;            // ... and its mirror ends at the other orientation
	pout[x] = in == CTG_NONE ? CtgRank{(u32)x, 0, 0} : CtgRank{in, 1, ctg_m(D, in >> 1)};
	D.circ[x >> 1] = 1;                                          // (both orientations write the same value)
}

// where unitig u lies: s = its orientation on the representative, h = the representative's first step, hm = the mirror's, r and
// koff = its rank there in steps and in k-mers, n_steps and n_kmers of the contig
struct CtgAt {
	u32 s, h, hm, r, n_steps;
	u64 koff, n_kmers;
};
__device__ __forceinline__ CtgAt ctg_at(const CtgDev &D, const CtgRank *rank, u64 u)
{
	const CtgRank a = rank[2 * u], b = rank[2 * u + 1];
	const u64 all = a.kmers + b.kmers + ctg_m(D, u);
	const u32 n = a.steps + b.steps + 1;
	if ((a.ptr >> 1) <= (b.ptr >> 1)) return CtgAt{0, a.ptr, b.ptr, a.steps, n, a.kmers, all};   // equal only for a single step: as stored
	return CtgAt{1, b.ptr, a.ptr, b.steps, n, b.kmers, all};
}

// thread u <= U: tot[u] = (1, bytes, steps) where a contig starts at unitig u, tot[U] = 0: the exclusive scan ends with the totals
__global__ __launch_bounds__(256) void k_ctg_mark(CtgDev D, const CtgRank *rank, CtgTot *tot)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	if (u > D.U) return;
	CtgTot t{0, 0, 0};
	if (u < D.U) {
		const CtgAt q = ctg_at(D, rank, u);
		if (q.r == 0) t = CtgTot{1, q.n_kmers + (u64)D.k - 1, q.n_steps};
	}
	tot[u] = t;
}

// thread c < the number of contigs (D.sc[U].n)
__global__ __launch_bounds__(256) void k_ctg_rec_init(CtgDev D)
{
	const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
	if (c < D.U && c < D.sc[D.U].n) D.crec[c] = Contig{0, 0, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, ~0ULL, 0, 0};
}

// thread u <= U (D.sc: the scanned marks; D.clc is zero before)
__global__ __launch_bounds__(256) void k_ctg_place(CtgDev D, const CtgRank *rank)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	bool circular = false, multi = false;
	if (u == D.U) { if (D.sc[u].n <= D.U) D.coffs[D.sc[u].n] = D.sc[u].len; }
	else if (u < D.U) {
		const CtgAt q = ctg_at(D, rank, u);
		if ((u64)(q.h >> 1) < D.U && (u64)(q.hm >> 1) < D.U) {
			const CtgTot at = D.sc[q.h >> 1];
			const u64 c = at.n;
			const u32 x = (u32)(2 * u) + q.s;
			if (c < D.U) {
				if (at.steps + q.r < D.U) D.steps[at.steps + q.r] = x;
				D.place[u] = CtgPlace{(u32)(2 * c) + q.s, (u32)q.koff};
				D.ubase[u] = ((at.len + q.koff) & (CTG_FIRST - 1)) | (q.s ? CTG_REV : 0) | (q.r == 0 ? CTG_FIRST : 0);
				Contig *R = D.crec + c;
				if (D.urec) {
					const Unitig r = D.urec[u];
					atomicAdd((unsigned long long *)&R->sum_count, (unsigned long long)r.sum_count);
					atomicMin(&R->min_count, r.min_count);
					atomicMax(&R->max_count, r.max_count);
				}
				const u32 in = ctg_link_in(D, x);                       // a cycle's first step keeps its link in: the closing link
				if (in != CTG_NONE) {
					const u64 s = D.supo[in];
					atomicAdd((unsigned long long *)&R->sum_support, (unsigned long long)s);
					atomicMin((unsigned long long *)&R->min_support, (unsigned long long)s);
				}
				if (q.r == 0) {
					const u32 tail = q.hm ^ 1u;
					D.coffs[c] = at.len;
					R->n_kmers = q.n_kmers;
					R->first_step = at.steps;
					R->n_steps = q.n_steps;
					R->circular = D.circ[u];
					R->n_pred = D.nk[q.h ^ 1u];
					R->n_succ = D.nk[tail];
					if (!D.urec) R->min_count = 0;                      // (nothing adds to these two where this lane stores them)
					if (in == CTG_NONE && q.n_steps == 1) R->min_support = 0;
					D.clc[2 * c] = D.nk[tail];
					D.clc[2 * c + 1] = D.nk[q.h ^ 1u];
					D.last[2 * c] = tail;
					D.last[2 * c + 1] = q.h ^ 1u;
					circular = D.circ[u] != 0;
					multi = q.n_steps > 1;
				}
			}
		}
	}
	const u64 bc = __ballot(circular), bm = __ballot(multi);
	if ((threadIdx.x & 63) == 0) {
		if (bc) atomicAdd(D.cnt + CTG_C_CIRCULAR, (unsigned long long)__popcll(bc));
		if (bm) atomicAdd(D.cnt + CTG_C_MULTI, (unsigned long long)__popcll(bm));
	}
}

// thread oc <= 2 C (C = D.sc[U].n; D.clsc: the scanned end counts, [2 U + 1])
__global__ __launch_bounds__(256) void k_ctg_clinks(CtgDev D)
{
	const u64 oc = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 C = ctg_min(D.sc[D.U].n, D.U);
	if (oc > 2 * C) return;
	const u64 at = D.clsc[oc];
	D.cloffs[oc] = at;
	if (oc == 2 * C) return;
	const u32 o = D.last[oc];
	if ((u64)o >= 2 * D.U) return;
	u64 lo, hi, j = 0;
	ctg_row(D, o, &lo, &hi);
	for (u64 e = lo; e < hi; e++) {
		const u32 t = D.links[e];
		if ((u64)t >= 2 * D.U || !D.ekeep[e]) continue;
		if (at + j < D.n_links) {
			D.clinks[at + j] = D.place[t >> 1].oc ^ (t & 1u);        // the oriented contig whose first step is t
			D.csup[at + j] = D.esup[e];
		}
		j++;
	}
}

// ---- the byte emit

// the complement of four bytes of uppercase ACGT at once (A <-> T differ in 0x15, C <-> G in 0x04; bit 1 tells the pairs apart)
__device__ __forceinline__ u32 ctg_comp4(u32 w)
{
	const u32 m = (w >> 1) & 0x01010101u;
	return w ^ 0x15151515u ^ (m | (m << 4));
}

// piece i of the tile [t0, t1): the bytes of unitig u0 + i that lie in the tile and are emitted (a step that is not marked
// CTG_FIRST never writes its first `later_skip` bytes: k - 1 for a contig, 0 for a scaffold).  They go to out[d0, d1); the byte at
// d0 is s_in[x0], the next one s_in[x0 + 1] (forward) or s_in[x0 - 1] (rev).
__device__ __forceinline__ bool ctg_piece(const u64 *s_off, const u64 *s_base, u32 i, u64 t0, u64 t1, u64 later_skip, u64 *d0, u64 *d1, u32 *x0, bool *rev)
{
	const u64 so = s_off[i], eo = s_off[i + 1];
	if (eo <= so) return false;
	const u64 len = eo - so, a = ctg_max(so, t0), b = ctg_min(eo, t1);
	if (b <= a) return false;
	const u64 ja = a - so, jb = b - so, w = s_base[i], base = w & (CTG_FIRST - 1), skip = (w & CTG_FIRST) ? 0 : later_skip;
	*rev = (w & CTG_REV) != 0;
	if (!*rev) {
		const u64 j0 = ctg_max(ja, skip);
		if (jb <= j0) return false;
		*d0 = base + j0; *d1 = base + jb; *x0 = (u32)(so + j0 - t0);
	} else {
		const u64 lim = len > skip ? len - skip : 0, j1 = ctg_min(jb, lim);
		if (j1 <= ja) return false;
		*d0 = base + (len - j1); *d1 = base + (len - ja); *x0 = (u32)(so + j1 - 1 - t0);
	}
	return true;
}

// The tile of block blockIdx.x of a unitig set (useq, uoffs, U, n_ubases) into out[cap]: ubase[u] says where the oriented string
// of unitig u goes.  Shared by k_ctg_emit and k_scf_emit (scaffold_kernels.h).
__device__ __forceinline__ void ctg_emit_tile(const unsigned char *useq, const u64 *uoffs, u64 U, u64 n_ubases, const u64 *ubase, u64 later_skip, unsigned char *out, u64 cap)
{
	__shared__ __align__(16) unsigned char s_in[CTG_TILE + 16];    // (a word is read behind the last byte)
	__shared__ u64 s_off[CTG_NB + 1];
	__shared__ u64 s_base[CTG_NB];
	__shared__ u32 s_pre[CTG_NB + 1];
	__shared__ u32 s_part[256];
	__shared__ u64 s_u0;
	__shared__ u32 s_nseg;
	const u32 tid = threadIdx.x;
	const u64 t0 = (u64)blockIdx.x * CTG_TILE, t1 = ctg_min(t0 + CTG_TILE, n_ubases);
	{
		const u64 p = t0 + (u64)tid * 16;
		if (((size_t)useq & 15) == 0 && p + 16 <= n_ubases) *(uint4 *)(s_in + tid * 16) = *(const uint4 *)(useq + p);
		else
			for (u32 b = 0; b < 16; b++) s_in[tid * 16 + b] = p + b < n_ubases ? useq[p + b] : (unsigned char)0;
	}
	if (tid == 0) {                                              // the tile's first unitig: the last one that starts at or in front of t0
		u64 lo = 0, hi = U;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (ctg_min(uoffs[mid], n_ubases) <= t0) lo = mid + 1; else hi = mid;
		}
		s_u0 = lo ? lo - 1 : 0;
		s_nseg = 0;
	}
	__syncthreads();
	const u64 u0 = s_u0;
	for (u32 i = tid; i <= CTG_NB; i += 256) {
		const u64 u = u0 + i, off = u <= U ? ctg_min(uoffs[u], n_ubases) : n_ubases;
		s_off[i] = off;
		if (i < CTG_NB) {
			s_base[i] = u < U ? ubase[u] : 0;
			if (u < U && off < t1) atomicMax(&s_nseg, i + 1);
		}
	}
	__syncthreads();
	const u32 nseg = s_nseg;
	u32 wn[4], sum = 0;                                            // the aligned 16-byte output words each of this lane's 4 pieces touches
	for (u32 j = 0; j < 4; j++) {
		const u32 i = 4 * tid + j;
		u64 d0, d1;
		u32 x0;
		bool rev;
		wn[j] = i < nseg && ctg_piece(s_off, s_base, i, t0, t1, later_skip, &d0, &d1, &x0, &rev) ? (u32)(((d1 + 15) >> 4) - (d0 >> 4)) : 0;
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
	if (tid == 255) s_pre[CTG_NB] = run;
	__syncthreads();
	const u32 total = s_pre[CTG_NB];
	const bool wide = ((size_t)out & 15) == 0;
	for (u32 w = tid; w < total; w += 256) {
		u32 lo = 0, hi = CTG_NB;                                     // the last piece with s_pre[i] <= w: the one word w belongs to
		while (lo < hi) {
			const u32 mid = (lo + hi) >> 1;
			if (s_pre[mid] <= w) lo = mid + 1; else hi = mid;
		}
		const u32 i = lo - 1;
		u64 d0, d1;
		u32 x0;
		bool rev;
		if (!ctg_piece(s_off, s_base, i, t0, t1, later_skip, &d0, &d1, &x0, &rev)) continue;
		const u64 A = ((d0 >> 4) + (w - s_pre[i])) << 4;
		u32 word[4];
		bool full[4];
		for (u32 g = 0; g < 4; g++) {
			u32 v = 0;
			full[g] = A + 4 * g >= d0 && A + 4 * g + 4 <= d1;
			if (full[g]) {                                           // four bytes of the tile from two aligned words of it
				const u32 x = rev ? x0 - (u32)(A + 4 * g - d0) - 3 : x0 + (u32)(A + 4 * g - d0), y = x & (CTG_TILE - 4);
				const u64 two = (u64)*(const u32 *)(s_in + y + 4) << 32 | *(const u32 *)(s_in + y);
				v = (u32)(two >> (8 * (x & 3)));
				word[g] = rev ? ctg_comp4(__builtin_bswap32(v)) : v;
				continue;
			}
			for (u32 b = 0; b < 4; b++) {
				const u64 d = A + 4 * g + b;
				if (d >= d0 && d < d1) {
					const u32 x = rev ? x0 - (u32)(d - d0) : x0 + (u32)(d - d0);
					v |= (u32)s_in[x & (CTG_TILE - 1)] << (8 * b);
				}
			}
			word[g] = rev ? ctg_comp4(v) : v;
		}
		if (wide && full[0] && full[1] && full[2] && full[3] && A + 16 <= cap) {
			*(uint4 *)(out + A) = make_uint4(word[0], word[1], word[2], word[3]);
			continue;
		}
		for (u32 g = 0; g < 4; g++) {
			if (wide && full[g] && A + 4 * g + 4 <= cap) { *(u32 *)(out + A + 4 * g) = word[g]; continue; }
			for (u32 b = 0; b < 4; b++) {
				const u64 d = A + 4 * g + b;
				if (d >= d0 && d < d1 && d < cap) out[d] = (unsigned char)(word[g] >> (8 * b));
			}
		}
	}
}

// one block per tile of CTG_TILE input bytes
__global__ __launch_bounds__(256) void k_ctg_emit(CtgDev D)
{
	ctg_emit_tile(D.useq, D.uoffs, D.U, D.n_ubases, D.ubase, (u64)(D.k - 1), D.cseq, D.n_ubases);
}
