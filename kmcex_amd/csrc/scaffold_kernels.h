// scaffold_kernels.h -- kmx_unitig_scaffold*: scaffolds from the pair links between unitigs (the rule: include/kmx.h; the host
// side: scaffold_host.h; the launchers: unitig_device.hip).  The construction of contig_kernels.h on another edge set: the edges
// are the entries of a list of unbounded degree, not rows of at most 4, and the bytes carry gaps.  The kernels, in the order the
// host runs them:
//   k_scf_best    one lane per list entry: a pair link raises best[a] and best[b ^ 1] by a 64-bit atomicMax;
//   k_scf_keep    one lane per list entry: its verdict from the two bests (complete only after k_scf_best, hence two launches);
//                 a kept entry adds 1 to nk[a] and nk[b ^ 1] and lowers only[a] and only[b ^ 1] to its index.  The five entry
//                 counters are summed per wave, then in LDS: one global atomic per block and counter.  No lane's work depends on
//                 a unitig's degree;
//   k_scf_init    per oriented unitig the chain link in -> the rank state: a pointer, a rank in steps and a rank in BYTES, the
//                 bytes of the step in front plus the N of the link;
//   k_ctg_round   the contigs' doubling round as it is (contig_kernels.h): it is generic in (pointer, steps, 64-bit rank);
//   k_scf_cut     what has not settled lies on a cycle: cut in front of its smallest unitig as stored (k_ctg_cut's logic);
//   k_scf_mark    per unitig: (1, bytes, steps) where a scaffold starts, to be scanned;
//   k_scf_rec_init, k_scf_place   per unitig: its step, its place, its share of the scaffold's record (integer atomics), where
//                 its bytes go; at a scaffold's first step the rest of the record and soffsets;
//   k_scf_emit    the bytes, once the host has seen that they fit and has filled sseq[0, n_sbases) with 'N': the tile emit of
//                 the contigs (ctg_emit_tile) with nothing skipped.  A piece's edge words are written byte by byte inside the
//                 piece only, so the N runs between the pieces stay.
// Every index read from the caller's arrays is clamped or checked where it is read and every store is checked against its
// capacity: bad device input gives wrong scaffolds, never an access outside a buffer.  The chain link is tested from both sides,
// so whatever the list holds the links form mirror-paired paths and cycles and the doubling ends within its bounded rounds.
#pragma once
#include "contig_kernels.h"

static constexpr u32 SCF_NONE = 0xFFFFFFFFu;

// the clamped bytes of unitig u < U
__device__ __forceinline__ u64 scf_len(const ScfDev &D, u64 u)
{
	const u64 a = ctg_min(D.uoffs[u], D.n_ubases), b = ctg_min(D.uoffs[u + 1], D.n_ubases);
	return b > a ? b - a : 0;
}
// its k-mers; 0 for what is shorter than k
__device__ __forceinline__ u64 scf_m(const ScfDev &D, u64 u)
{
	const u64 len = scf_len(D, u);
	return len >= (u64)D.k ? len - (u64)D.k + 1 : 0;
}
// entry E is a pair link
__device__ __forceinline__ bool scf_is_link(const ScfDev &D, const PairLink &E)
{
	return (u64)E.a < 2 * D.U && (u64)E.b < 2 * D.U && (E.a >> 1) != (E.b >> 1) && E.n_pairs >= 1;
}
// the gap of a pair link: est = inner - 1 - sum_dist / n_pairs - (k - 1) in signed 64-bit arithmetic (it wraps like the host's),
// the N written = est clamped into [min_n, max_n]
__device__ __forceinline__ u32 scf_gap(const ScfDev &D, const PairLink &E, long long *est)
{
	const u64 dist = E.sum_dist / E.n_pairs;
	const long long e = (long long)((u64)D.inner - 1 - dist - (u64)(D.k - 1));
	*est = e;
	return e < (long long)D.min_n ? D.min_n : e > (long long)D.max_n ? D.max_n : (u32)e;
}

// thread i < n_plinks
__global__ __launch_bounds__(256) void k_scf_best(ScfDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= D.n_plinks) return;
	const PairLink E = D.plinks[i];
	if (!scf_is_link(D, E)) return;
	atomicMax((unsigned long long *)D.best + E.a, (unsigned long long)E.n_pairs);
	atomicMax((unsigned long long *)D.best + (E.b ^ 1u), (unsigned long long)E.n_pairs);
}

// thread i < n_plinks (D.nk is zero and D.only all ones before)
__global__ __launch_bounds__(256) void k_scf_keep(ScfDev D)
{
	__shared__ unsigned int s_cnt[5];
	if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	int c = -1;                                                    // the counter this entry adds to behind SCF_C_LINKS
	bool link = false;
	if (i < D.n_plinks) {
		const PairLink E = D.plinks[i];
		link = scf_is_link(D, E);
		if (!link) c = SCF_C_IGNORED;
		else if (E.n_pairs < D.min_pairs) c = SCF_C_BELOW_MIN;
		else if (D.ratio && (ctg_lt(E.n_pairs, D.ratio, D.best[E.a]) || ctg_lt(E.n_pairs, D.ratio, D.best[E.b ^ 1u]))) c = SCF_C_BELOW_RATIO;
		else {
			c = SCF_C_KEPT;
			atomicAdd(D.nk + E.a, 1u);
			atomicAdd(D.nk + (E.b ^ 1u), 1u);
			atomicMin(D.only + E.a, (u32)i);
			atomicMin(D.only + (E.b ^ 1u), (u32)i);
		}
	}
	const u64 bl = __ballot(link);
	if ((threadIdx.x & 63) == 0 && bl) atomicAdd(&s_cnt[SCF_C_LINKS], (unsigned int)__popcll(bl));
	for (int j = SCF_C_IGNORED; j <= SCF_C_KEPT; j++) {
		const u64 b = __ballot(c == j);
		if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_cnt[j], (unsigned int)__popcll(b));
	}
	__syncthreads();
	if (threadIdx.x < 5 && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// the chain link into oriented unitig x < 2 U, or SCF_NONE: p -> x through entry *e iff that entry is the one kept edge out of p
// and, mirrored, the one kept edge out of x ^ 1.  Tested from both sides, so p -> x iff (x ^ 1) -> (p ^ 1) whatever the list.
__device__ __forceinline__ u32 scf_link_in(const ScfDev &D, u32 x, PairLink *E)
{
	const u32 y = x ^ 1u;
	if (D.nk[y] != 1) return SCF_NONE;
	const u32 e = D.only[y];
	if ((u64)e >= D.n_plinks) return SCF_NONE;
	*E = D.plinks[e];
	u32 t;
	if (E->a == y) t = E->b;                                       // y -> t is the entry itself ...
	else if ((E->b ^ 1u) == y) t = E->a ^ 1u;                      // ... or its mirror
	else return SCF_NONE;
	if ((u64)t >= 2 * D.U || (t >> 1) == (y >> 1) || E->n_pairs < 1) return SCF_NONE;
	const u32 p = t ^ 1u;
	if (D.nk[p] != 1 || D.only[p] != e) return SCF_NONE;
	return p;
}

// thread x < 2 U
__global__ __launch_bounds__(256) void k_scf_init(ScfDev D, CtgRank *rank, u32 *mn)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	bool entry = false;                                            // the link in is an entry as it is listed: each chain entry once
	if (x < 2 * D.U) {
		PairLink E;
		const u32 p = scf_link_in(D, (u32)x, &E);
		long long est;
		rank[x] = p != SCF_NONE ? CtgRank{p, 1, scf_len(D, p >> 1) + scf_gap(D, E, &est)} : CtgRank{(u32)x, 0, 0};
		mn[x] = (u32)(x >> 1);
		entry = p != SCF_NONE && E.a == p && E.b == (u32)x;
	}
	const u64 b = __ballot(entry);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(D.cnt + SCF_C_CHAIN, (unsigned long long)__popcll(b));
}

// after the last round: what has not settled lies on a cycle whose smallest unitig is mn[x]
__global__ __launch_bounds__(256) void k_scf_cut(ScfDev D, const CtgRank *pin, const u32 *mnin, CtgRank *pout)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	if (x >= 2 * D.U) return;
	const CtgRank a = pin[x];
	if (a.steps == 0 || (u64)a.ptr >= 2 * D.U || pin[a.ptr].steps == 0) { pout[x] = a; return; }   // a head, or its pointer is one: settled
	const u32 s = 2 * mnin[x];                                   // the representative starts here ...
	PairLink E;
	u32 in = scf_link_in(D, (u32)x, &E);
	if ((u32)x == s || in == (s ^ 1u)) in = SCF_NONE;            // ... and its mirror ends at the other orientation
	long long est;
	pout[x] = in == SCF_NONE ? CtgRank{(u32)x, 0, 0} : CtgRank{in, 1, scf_len(D, in >> 1) + scf_gap(D, E, &est)};
	D.circ[x >> 1] = 1;                                          // (both orientations write the same value)
}

// where unitig u lies: s = its orientation on the representative, h = the representative's first step, hm = the mirror's, r and
// boff = its rank there in steps and in bytes, n_steps and n_bases of the scaffold
struct ScfAt {
	u32 s, h, hm, r, n_steps;
	u64 boff, n_bases;
};
__device__ __forceinline__ ScfAt scf_at(const ScfDev &D, const CtgRank *rank, u64 u)
{
	const CtgRank a = rank[2 * u], b = rank[2 * u + 1];
	const u64 all = a.kmers + b.kmers + scf_len(D, u);           // the bytes and gaps in front of u, those behind it (the mirror's rank), its own
	const u32 n = a.steps + b.steps + 1;
	if ((a.ptr >> 1) <= (b.ptr >> 1)) return ScfAt{0, a.ptr, b.ptr, a.steps, n, a.kmers, all};   // equal only for a single step: as stored
	return ScfAt{1, b.ptr, a.ptr, b.steps, n, b.kmers, all};
}

// thread u <= U: tot[u] = (1, bytes, steps) where a scaffold starts at unitig u, tot[U] = 0: the exclusive scan ends with the totals
__global__ __launch_bounds__(256) void k_scf_mark(ScfDev D, const CtgRank *rank, CtgTot *tot)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	if (u > D.U) return;
	CtgTot t{0, 0, 0};
	if (u < D.U) {
		const ScfAt q = scf_at(D, rank, u);
		if (q.r == 0) t = CtgTot{1, q.n_bases, q.n_steps};
	}
	tot[u] = t;
}

// thread s < the number of scaffolds (D.sc[U].n)
__global__ __launch_bounds__(256) void k_scf_rec_init(ScfDev D)
{
	const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
	if (s < D.U && s < D.sc[D.U].n) D.srec[s] = Scaffold{0, 0, 0, 0xFFFFFFFFu, 0, 0, 0, 0, ~0ULL, 0};
}

// thread u <= U (D.sc: the scanned marks)
__global__ __launch_bounds__(256) void k_scf_place(ScfDev D, const CtgRank *rank)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	bool circular = false, multi = false;
	if (u == D.U) { if (D.sc[u].n <= D.U) D.soffs[D.sc[u].n] = D.sc[u].len; }
	else if (u < D.U) {
		const ScfAt q = scf_at(D, rank, u);
		if ((u64)(q.h >> 1) < D.U && (u64)(q.hm >> 1) < D.U) {
			const CtgTot at = D.sc[q.h >> 1];
			const u64 c = at.n;
			const u32 x = (u32)(2 * u) + q.s;
			if (c < D.U) {
				PairLink E;
				const u32 in = scf_link_in(D, x, &E);                  // a cycle's first step keeps its link in: the closing link
				long long est = 0;
				const u32 n_gap = in != SCF_NONE ? scf_gap(D, E, &est) : 0;
				if (at.steps + q.r < D.U) D.steps[at.steps + q.r] = ScfStep{x, n_gap, est};
				D.place[u] = ScfPlace{(u32)(2 * c) + q.s, q.r, q.boff};
				D.ubase[u] = ((at.len + q.boff) & (CTG_FIRST - 1)) | (q.s ? CTG_REV : 0);
				Scaffold *R = D.srec + c;
				atomicAdd((unsigned long long *)&R->n_kmers, (unsigned long long)scf_m(D, u));
				if (D.urec) {
					const Unitig r = D.urec[u];
					atomicAdd((unsigned long long *)&R->sum_count, (unsigned long long)r.sum_count);
					atomicMin(&R->min_count, r.min_count);
					atomicMax(&R->max_count, r.max_count);
				}
				if (in != SCF_NONE) {
					atomicAdd((unsigned long long *)&R->sum_pairs, (unsigned long long)E.n_pairs);
					atomicMin((unsigned long long *)&R->min_pairs, (unsigned long long)E.n_pairs);
					if (q.r != 0) atomicAdd((unsigned long long *)&R->n_gap_bases, (unsigned long long)n_gap);   // the closing link is not spelled
				}
				if (q.r == 0) {
					circular = D.circ[u] != 0;
					multi = q.n_steps > 1;
					D.soffs[c] = at.len;
					R->n_bases = q.n_bases;
					R->first_step = (u32)at.steps;
					R->n_steps = q.n_steps | (circular ? SCF_CIRCULAR : 0);
					if (!D.urec) R->min_count = 0;                      // (nothing adds to these two where this lane stores them)
					if (!multi) R->min_pairs = 0;
				}
			}
		}
	}
	const u64 bc = __ballot(circular), bm = __ballot(multi);
	if ((threadIdx.x & 63) == 0) {
		if (bc) atomicAdd(D.cnt + SCF_C_CIRCULAR, (unsigned long long)__popcll(bc));
		if (bm) atomicAdd(D.cnt + SCF_C_MULTI, (unsigned long long)__popcll(bm));
	}
}

// one block per tile of CTG_TILE input bytes; sseq[0, n_sbases) holds 'N' before
__global__ __launch_bounds__(256) void k_scf_emit(ScfDev D)
{
	ctg_emit_tile(D.useq, D.uoffs, D.U, D.n_ubases, D.ubase, 0, D.sseq, D.seq_cap);
}
