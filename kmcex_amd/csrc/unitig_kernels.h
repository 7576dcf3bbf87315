// unitig_kernels.h -- kmx_unitigs: the compacted de Bruijn graph of a sorted listing (the rule: include/kmx.h).
//
// The listing is its own exact membership structure: a k-mer is a node iff a search of the sorted k-mers finds it with a count
// of at least thr.  The kernels, in the order the host runs them (unitig_device.hip, unitig_host.h):
//   k_uni_index   one pass over the listing: validates it (strictly ascending, canonical, nothing above bit 2k) and fills
//                 start[p] = the first entry whose top `bits` bits are at least p, so a probe searches one bucket of a few
//                 entries instead of the whole listing;
//   k_uni_adj     a group of 8 lanes per entry asks the 8 neighbours of its listed orientation (4 successors, 4 predecessors);
//                 one ballot gives the degrees, and where a side has exactly one neighbour that lane leaves its oriented index;
//   k_uni_init    per ORIENTED node (2 n of them) the link in, from the two entries' degrees; rank state: a node without a
//                 link in is a head;
//   k_uni_round   one round of pointer doubling along the links in, from one copy of the state into the other (a head is the
//                 node of rank 0, never "a node that points at itself": a cycle of 2^j nodes does that too); a word tells
//                 the host that something moved.  After ceil(log2 n) + 1 rounds only nodes on cycles still move; their running
//                 minimum of the listing index has covered the whole cycle by then;
//   k_uni_cut     nodes that have not settled lie on cycles: each cycle is cut in front of its smallest entry in the listed
//                 orientation (and the mirror cycle behind that entry's reverse complement), then ranked again like a path;
//   k_uni_mark    per entry: which of its two orientations lies on the representative (the path of a mirror pair whose head
//                 has the smaller listing index; a single node as listed), whether it is the head, the unitig's length;
//   k_uni_emit    per entry, after the scan of the marks: its bytes (all k at the head, the last one otherwise), its count into
//                 the record with integer atomics, and at the head the rest of the record.
// kmx_unitig_graph* add the edges between unitigs (the rule: include/kmx.h), after the ranking and beside the emit:
//   k_uni_lmark   per entry: at a head, the edges that leave its unitig's two ends (n_pred + n_succ), to be scanned, and the
//                 unitig's head and tail entry into two lists by unitig number;
//   k_uni_links   a group of 8 lanes per unitig: lanes 0..3 append a base to the representative's last k-mer (the tail entry),
//                 lanes 4..7 to the reverse complement of its first (the head entry); a neighbour that is found is the first
//                 k-mer of one oriented unitig, whose number its own place gives; one ballot gives the slot.  Interior
//                 entries are never visited.
// No lane walks a path: the longest unitig costs rounds (log), never a loop.  Every store is checked against its capacity.
#pragma once
#include "device_common.h"
#include "kmx_types.h"

struct UniK {                                                  // a k-mer as a 2k-bit integer, right-aligned in 128 bits
	u64 hi, lo;
};

template <int W> __device__ __forceinline__ UniK uni_load(const u64 *km, u64 i)
{
	if (W == 1) return UniK{0, km[i]};
	return UniK{km[2 * i], km[2 * i + 1]};
}
__device__ __forceinline__ bool uni_less(UniK a, UniK b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ bool uni_eq(UniK a, UniK b) { return a.hi == b.hi && a.lo == b.lo; }
__device__ __forceinline__ UniK uni_shr(UniK a, int s)         // 0 <= s < 128
{
	if (s == 0) return a;
	if (s >= 64) return UniK{0, a.hi >> (s - 64)};
	return UniK{a.hi >> s, (a.lo >> s) | (a.hi << (64 - s))};
}
__device__ __forceinline__ UniK uni_mask(int k)                // 2k is never 64: k is odd
{
	if (2 * k < 64) return UniK{0, (1ULL << (2 * k)) - 1};
	return UniK{(1ULL << (2 * k - 64)) - 1, ~0ULL};
}
__device__ __forceinline__ UniK uni_rc(UniK x, int k)
{
	const UniK m = uni_mask(k);
	const UniK c{~x.hi & m.hi, ~x.lo & m.lo};
	return uni_shr(UniK{rev2_u64(c.lo), rev2_u64(c.hi)}, 128 - 2 * k);
}
__device__ __forceinline__ UniK uni_succ(UniK x, int k, u32 c)  // x[1:] + c
{
	const UniK m = uni_mask(k);
	return UniK{((x.hi << 2) | (x.lo >> 62)) & m.hi, ((x.lo << 2) | c) & m.lo};
}
__device__ __forceinline__ UniK uni_pred(UniK x, int k, u32 c)  // c + x[:-1]
{
	UniK y = uni_shr(x, 2);
	const int s = 2 * k - 2;
	if (s < 64) y.lo |= (u64)c << s; else y.hi |= (u64)c << (s - 64);
	return y;
}
__device__ __forceinline__ u32 uni_prefix(const UniDev &d, UniK x)
{
	const u64 p = uni_shr(x, d.shift).lo, top = (1ULL << d.bits) - 1;
	return (u32)(p < top ? p : top);                            // (a valid k-mer never exceeds top; a listing that does is refused)
}

// the entry holding the canonical k-mer q, or UNI_NONE: one bucket of start[], then a binary search inside it
template <int W> __device__ __forceinline__ u32 uni_find(const UniDev &d, UniK q)
{
	const u32 p = uni_prefix(d, q);
	u64 lo = d.start[p], hi = d.start[p + 1];
	if (hi > d.n) hi = d.n;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (uni_less(uni_load<W>(d.km, mid), q)) lo = mid + 1; else hi = mid;
	}
	return lo < d.n && uni_eq(uni_load<W>(d.km, lo), q) ? (u32)lo : UNI_NONE;
}

// thread i <= n; entry i fills start[] for the prefixes behind entry i - 1's up to its own, thread n the rest up to 2^bits
template <int W> __global__ __launch_bounds__(256) void k_uni_index(UniDev d)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > d.n) return;
	u64 p0 = 0, p1 = 1ULL << d.bits;                             // start[p0 .. p1] = i
	if (i < d.n) {
		const UniK x = uni_load<W>(d.km, i), m = uni_mask(d.k);
		bool bad = (x.hi & ~m.hi) != 0 || (x.lo & ~m.lo) != 0 || uni_less(uni_rc(x, d.k), x);
		p1 = uni_prefix(d, x);
		if (i) {
			const UniK w = uni_load<W>(d.km, i - 1);
			bad = bad || !uni_less(w, x);
			p0 = (u64)uni_prefix(d, w) + 1;
		}
		if (bad) *d.err = 1;
	}
	else if (i) p0 = (u64)uni_prefix(d, uni_load<W>(d.km, i - 1)) + 1;
	for (u64 p = p0; p <= p1; p++) d.start[p] = (u32)i;
}

// 8 lanes per entry: lanes 0..3 the successors x[1:] + c, lanes 4..7 the predecessors c + x[:-1] of the listed orientation
template <int W> __global__ __launch_bounds__(256) void k_uni_adj(UniDev d)
{
	const u64 g = (u64)blockIdx.x * 256 + threadIdx.x, i = g >> 3;
	const u32 l = threadIdx.x & 7, c = l & 3;
	bool hit = false;
	u32 tgt = UNI_NONE;
	const bool node = i < d.n && d.cnt[i] >= d.thr;
	if (node) {
		const UniK x = uni_load<W>(d.km, i);
		const UniK y = l < 4 ? uni_succ(x, d.k, c) : uni_pred(x, d.k, c), r = uni_rc(y, d.k);
		const bool fwd = !uni_less(r, y);
		const u32 j = uni_find<W>(d, fwd ? y : r);
		if (j != UNI_NONE && d.cnt[j] >= d.thr) { hit = true; tgt = 2 * j + (fwd ? 0u : 1u); }
	}
	const u64 b = __ballot(hit);
	const u32 m8 = (u32)(b >> (threadIdx.x & 56)) & 0xFFu;       // the 8 lanes of this entry (a wave holds 8 whole groups)
	if (i >= d.n) return;
	const u32 ns = __popc(m8 & 15u), np = __popc(m8 >> 4);
	if (l == 0) {
		d.deg[i] = node ? (unsigned char)(ns | (np << 3) | UNI_DEG_NODE) : (unsigned char)0;
		if (ns != 1) d.succ1[i] = UNI_NONE;
		if (np != 1) d.pred1[i] = UNI_NONE;
	}
	if (hit && l < 4 && ns == 1) d.succ1[i] = tgt;
	if (hit && l >= 4 && np == 1) d.pred1[i] = tgt;
}

__device__ __forceinline__ u32 uni_outdeg(const unsigned char *deg, u32 x) { const u32 g = deg[x >> 1]; return (x & 1) ? (g >> 3) & 7u : g & 7u; }
__device__ __forceinline__ u32 uni_indeg(const unsigned char *deg, u32 x) { const u32 g = deg[x >> 1]; return (x & 1) ? g & 7u : (g >> 3) & 7u; }
// the link into oriented node x, or UNI_NONE: its only predecessor, whose only successor is x, of another entry.  The
// predecessors of a reverse complement are the successors of the listed orientation, mirrored.
__device__ __forceinline__ u32 uni_link_in(const UniDev &d, u32 x)
{
	const u32 i = x >> 1;
	if (!(d.deg[i] & UNI_DEG_NODE)) return UNI_NONE;
	u32 p = (x & 1) ? d.succ1[i] : d.pred1[i];
	if (p == UNI_NONE) return UNI_NONE;
	if (x & 1) p ^= 1u;
	if ((p >> 1) == i || (p >> 1) >= d.n || uni_outdeg(d.deg, p) != 1) return UNI_NONE;
	return p;
}
__device__ __forceinline__ u64 uni_pair(u32 ptr, u32 rank) { return (u64)ptr << 32 | rank; }

__global__ __launch_bounds__(256) void k_uni_init(UniDev d, u64 *pair, u32 *mn)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	if (x >= 2 * d.n) return;
	const u32 p = uni_link_in(d, (u32)x);
	pair[x] = p == UNI_NONE ? uni_pair((u32)x, 0) : uni_pair(p, 1);
	mn[x] = (u32)(x >> 1);
}

// A head has rank 0 (and points at itself); a node has settled when its pointer is a head.  "Points at itself" alone would not
// do: on a cycle of 2^j nodes every pointer comes back to its own node after round j, with rank 2^j.  Ranks on a cycle only
// grow (they saturate instead of wrapping to 0), so nothing on a cycle ever looks like a head.  mn may be null (after the cut
// nothing lies on a cycle).
__device__ __forceinline__ u32 uni_rank_add(u32 a, u32 b) { const u64 s = (u64)a + b; return s > 0xFFFFFFFFULL ? 0xFFFFFFFFu : (u32)s; }
__global__ __launch_bounds__(256) void k_uni_round(const u64 *pin, const u32 *mnin, u64 *pout, u32 *mnout, u64 n2, u32 *moved)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	if (x >= n2) return;
	const u64 a = pin[x];
	const u32 p = (u32)(a >> 32);
	u64 o = a;
	u32 m = mnin ? mnin[x] : 0;
	if ((u32)a != 0 && p < n2) {
		const u64 b = pin[p];
		if ((u32)b != 0) {
			o = uni_pair((u32)(b >> 32), uni_rank_add((u32)a, (u32)b));
			if (mnin) { const u32 mp = mnin[p]; m = mp < m ? mp : m; }
			*moved = 1;
		}
	}
	pout[x] = o;
	if (mnout) mnout[x] = m;
}

// after the last round: what has not settled lies on a cycle whose smallest entry is mn[x]
__global__ __launch_bounds__(256) void k_uni_cut(UniDev d, const u64 *pin, const u32 *mnin, u64 *pout)
{
	const u64 x = (u64)blockIdx.x * 256 + threadIdx.x;
	if (x >= 2 * d.n) return;
	const u64 a = pin[x];
	const u32 p = (u32)(a >> 32);
	if ((u32)a == 0 || p >= 2 * d.n || (u32)pin[p] == 0) { pout[x] = a; return; }   // a head, or its pointer is one: settled
	const u32 s = 2 * mnin[x];                                   // the representative starts here ...
	u32 in = uni_link_in(d, (u32)x);
	if ((u32)x == s || in == (s ^ 1u)) in = UNI_NONE;            // ... and its mirror ends at the reverse complement
	pout[x] = in == UNI_NONE ? uni_pair((u32)x, 0) : uni_pair(in, 1);
	d.deg[x >> 1] |= UNI_DEG_CIRC;                               // (both orientations write the same byte value)
}

// where entry i lies: s = its orientation on the representative, h = the representative's head, r = its rank there, m = the
// unitig's k-mers, hm = the head of the mirror path (the reverse complement of the representative's tail)
struct UniPlace {
	u32 s, h, r, m, hm;
};
__device__ __forceinline__ UniPlace uni_place(const u64 *pair, u64 i)
{
	const u64 a = pair[2 * i], b = pair[2 * i + 1];
	const u32 ha = (u32)(a >> 32), hb = (u32)(b >> 32), ra = (u32)a, rb = (u32)b;
	const bool fwd = (ha >> 1) <= (hb >> 1);                     // equal only for a single node: as listed
	return fwd ? UniPlace{0, ha, ra, ra + rb + 1, hb} : UniPlace{1, hb, rb, ra + rb + 1, ha};
}

// thread i <= n: tot[i] = (1, bytes) where a unitig starts at entry i, tot[n] = (0, 0): the exclusive scan ends with the totals
__global__ __launch_bounds__(256) void k_uni_mark(UniDev d, const u64 *pair, UniTot *tot)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > d.n) return;
	UniTot t{0, 0};
	if (i < d.n && (d.deg[i] & UNI_DEG_NODE)) {
		const UniPlace q = uni_place(pair, i);
		if (q.r == 0) t = UniTot{1, (u64)q.m + (u64)d.k - 1};
	}
	tot[i] = t;
}

__global__ __launch_bounds__(256) void k_uni_rec_init(Unitig *rec, u64 n)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	if (u < n) rec[u] = Unitig{0, 0, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, {0, 0, 0, 0}};
}

// thread i <= n (sc: the scanned marks, sc[n] the totals).  seq[seq_cap], offs[rec_cap + 1], rec[rec_cap] (may be null).
template <int W> __global__ __launch_bounds__(256) void k_uni_emit(UniDev d, const u64 *pair, const UniTot *sc, unsigned char *seq, u64 seq_cap, u64 *offs, Unitig *rec, u64 rec_cap)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > d.n) return;
	if (i == d.n) { if (sc[i].n <= rec_cap) offs[sc[i].n] = sc[i].len; return; }
	if (!(d.deg[i] & UNI_DEG_NODE)) return;
	const UniPlace q = uni_place(pair, i);
	if ((q.h >> 1) >= d.n) return;
	const UniTot at = sc[q.h >> 1];
	UniK x = uni_load<W>(d.km, i);
	if (q.s) x = uni_rc(x, d.k);
	const u32 c = d.cnt[i];
	if (rec && at.n < rec_cap) {
		Unitig *R = rec + at.n;
		atomicAdd((unsigned long long *)&R->sum_count, (unsigned long long)c);
		atomicMin(&R->min_count, c);
		atomicMax(&R->max_count, c);
	}
	if (q.r) {
		const u64 o = at.len + (u64)d.k - 1 + q.r;
		if (o < seq_cap) seq[o] = (unsigned char)"ACGT"[x.lo & 3];
		return;
	}
	if (at.n <= rec_cap) offs[at.n] = at.len;
	for (int j = 0; j < d.k; j++) {
		const u64 o = at.len + (u64)j;
		if (o < seq_cap) seq[o] = (unsigned char)"ACGT"[uni_shr(x, 2 * (d.k - 1 - j)).lo & 3];
	}
	if (rec && at.n < rec_cap) {
		Unitig *R = rec + at.n;
		const u32 tail = q.hm ^ 1u;
		R->n_kmers = q.m;
		R->first_node = q.h >> 1;
		R->circular = (d.deg[q.h >> 1] & UNI_DEG_CIRC) ? 1 : 0;
		R->n_pred = (unsigned char)uni_indeg(d.deg, q.h);
		R->n_succ = (unsigned char)((tail >> 1) < d.n ? uni_outdeg(d.deg, tail) : 0);
		R->first_fwd = (unsigned char)!(q.h & 1);
	}
}

// ---- edges between unitigs.  An oriented unitig is 2 u + d: d = 0 as emitted, d = 1 its reverse complement.

// thread i <= n (sc: the scanned marks): lc[i] = the edges out of both orientations of the unitig whose head is entry i, 0
// elsewhere and at i = n; head_of[u], tail_of[u] = the head and the tail entry of unitig u.  The two lists take the place of
// succ1 and pred1, which nothing reads once the ranks stand.
__global__ __launch_bounds__(256) void k_uni_lmark(UniDev d, const u64 *pair, const UniTot *sc, u64 *lc)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > d.n) return;
	u64 t = 0;
	if (i < d.n && (d.deg[i] & UNI_DEG_NODE)) {
		const UniPlace q = uni_place(pair, i);
		const u32 tail = q.hm ^ 1u;
		if (q.r == 0 && (q.h >> 1) < d.n && (tail >> 1) < d.n) {
			t = uni_indeg(d.deg, q.h) + uni_outdeg(d.deg, tail);
			const u64 u = sc[i].n;
			if (u < d.n) { d.succ1[u] = (u32)i; d.pred1[u] = tail >> 1; }
		}
	}
	lc[i] = t;
}

// 8 lanes per unitig u <= n_uni (sc: the scanned marks, lsc: the scanned counts of k_uni_lmark; lsc[n] the total; head_of and
// tail_of: d.succ1 and d.pred1 as k_uni_lmark left them).  Lanes 0..3 append c to the tail entry's k-mer as it lies on the
// representative: the row of 2 u, which starts at lsc[head of u]; lanes 4..7 to the reverse complement of the head entry's:
// the row of 2 u + 1, behind the n_succ edges of the other.  loffs[2 rec_cap + 1], links[link_cap]; the group of u = n_uni
// writes the last offset.
template <int W> __global__ __launch_bounds__(256) void k_uni_links(UniDev d, const u64 *pair, const UniTot *sc, const u64 *lsc, u64 n_uni, u64 *loffs, u64 rec_cap, u32 *links, u64 link_cap)
{
	const u64 g = (u64)blockIdx.x * 256 + threadIdx.x, u = g >> 3;
	const u32 l = threadIdx.x & 7, c = l & 3;
	bool hit = false;
	u32 to = 0;
	u64 row = 0;
	const u32 head = u < n_uni && u < d.n ? d.succ1[u] : UNI_NONE;
	const u32 i = head == UNI_NONE ? UNI_NONE : l < 4 ? d.pred1[u] : head;
	if (i < d.n && head < d.n && (d.deg[i] & UNI_DEG_NODE)) {
		const UniPlace q = uni_place(pair, i);
		const u32 tail = q.hm ^ 1u;
		const bool mine = (q.h >> 1) == head && (l < 4 ? q.r + 1 == q.m : q.r == 0);
		if (mine && (tail >> 1) < d.n) {
			const u32 ns = uni_outdeg(d.deg, tail);
			row = lsc[head] + (l < 4 ? 0 : ns);
			if (l == 4 && 2 * u + 1 <= 2 * rec_cap) { loffs[2 * u] = row - ns; loffs[2 * u + 1] = row; }
			// the entry as the source's last k-mer: on the representative for d = 0, on its mirror for d = 1
			UniK x = uni_load<W>(d.km, i);
			if ((q.s != 0) != (l >= 4)) x = uni_rc(x, d.k);
			if (l < 4 ? uni_outdeg(d.deg, 2 * i + q.s) : uni_outdeg(d.deg, 2 * i + (q.s ^ 1u))) {
				const UniK y = uni_succ(x, d.k, c), r = uni_rc(y, d.k);
				const bool fwd = !uni_less(r, y);
				const u32 j = uni_find<W>(d, fwd ? y : r);
				if (j != UNI_NONE && (d.deg[j] & UNI_DEG_NODE)) {
					// y starts its oriented unitig: the representative of j's unitig if y is j's orientation there, else its mirror
					const UniPlace p = uni_place(pair, j);
					if ((p.h >> 1) < d.n) {
						hit = true;
						to = (u32)(2 * sc[p.h >> 1].n) + ((fwd ? 0u : 1u) == p.s ? 0u : 1u);
					}
				}
			}
		}
	}
	const u64 b = __ballot(hit);
	const u32 m4 = (u32)(b >> ((threadIdx.x & 56) + (l & 4))) & 0xFu;  // the 4 lanes of this row
	if (u == n_uni && l == 0 && 2 * n_uni <= 2 * rec_cap) loffs[2 * n_uni] = lsc[d.n];
	if (hit) {
		const u64 o = row + __popc(m4 & ((1u << c) - 1u));
		if (o < link_cap) links[o] = to;
	}
}

// ---- cleaning (kmx_*unitig_graph_clean*; the rule: include/kmx.h).  A round reads the records and the CSR the two emits have
// written for the working counts, takes one verdict per unitig, and zeroes the working counts of the unitigs that go.
//   k_uni_clean   a group of 8 lanes per unitig: its record, its two rows, the rows of at most 4 targets and the records of at
//                 most 16 competitors; one verdict byte per unitig (0, or the KMX_CLEAN_* bit of what removes it) and, per wave,
//                 one integer atomic per kind (ballot + popcount);
//   k_uni_drop    per entry: a node's unitig number from its place and the scanned marks, as in k_uni_emit; a set verdict
//                 zeroes the working count, stores the round, and counts the k-mer (one atomic per wave).
// No lane walks a unitig.
__device__ __forceinline__ bool uni_short_tip(const Unitig &r, u32 max_tip) { return !r.circular && r.n_kmers <= max_tip && (r.n_pred == 0) != (r.n_succ == 0); }
__device__ __forceinline__ bool uni_arm(const Unitig &r, u32 max_bubble) { return !r.circular && r.n_kmers <= max_bubble && r.n_pred == 1 && r.n_succ == 1; }
// entry e of the row of oriented unitig o, or UNI_NONE where the row is shorter (or anything lies outside the arrays)
__device__ __forceinline__ u32 uni_row_at(const UniClean &c, u64 o, u32 e)
{
	if (o >= 2 * c.n_uni) return UNI_NONE;
	const u64 a = c.loffs[o], b = c.loffs[o + 1];
	if (a + e >= b || a + e >= c.n_links) return UNI_NONE;
	const u32 t = c.links[a + e];
	return t < 2 * c.n_uni ? t : UNI_NONE;
}

// 8 lanes per unitig u < n_uni.  A tip: lane l looks at target l >> 1 of the attached end's row and at entries 2 (l & 1) and
// 2 (l & 1) + 1 of in(target); the target is answered when one of its two lanes found a competitor that beats u.  An arm: lanes
// 0..3 look at one entry of in(b) each.  cnt[3]: tips, islands, bubbles of this round.
// The records and the CSR are the ones the two emits of this round have just written on the same stream, so a row count outside
// [1, 4], an offset behind n_links or a target behind 2 U cannot occur; the checks only keep every access inside the arrays.
// Where one fails the lane finds no competitor, so the verdict falls to "stays": a damaged CSR would remove too little and
// never read or write out of bounds, and it raises no error of its own.
__global__ __launch_bounds__(256) void k_uni_clean(UniClean c, unsigned char *verdict, unsigned long long *cnt)
{
	const u64 g = (u64)blockIdx.x * 256 + threadIdx.x, u = g >> 3;
	const u32 l = threadIdx.x & 7;
	bool ok = false;
	u32 kind = 0, n_tgt = 0;
	if (u < c.n_uni) {
		const Unitig r = c.rec[u];
		if (r.circular) kind = 0;
		else if (r.n_pred == 0 && r.n_succ == 0) kind = r.n_kmers <= c.max_tip ? UNI_CLEAN_ISLANDS : 0;
		else if (uni_short_tip(r, c.max_tip)) {
			kind = UNI_CLEAN_TIPS;
			const u64 o = r.n_succ > 0 ? 2 * u : 2 * u + 1;
			n_tgt = r.n_succ > 0 ? r.n_succ : r.n_pred;
			const u32 t = uni_row_at(c, o, l >> 1);
			if (t != UNI_NONE) {
				for (u32 e = 2 * (l & 1); e < 2 * (l & 1) + 2; e++) {
					const u32 s1 = uni_row_at(c, t ^ 1u, e);
					if (s1 == UNI_NONE) continue;
					const u64 w = (s1 ^ 1u) >> 1;
					if (w == u) continue;
					const Unitig q = c.rec[w];
					ok = ok || !uni_short_tip(q, c.max_tip) || q.n_kmers > r.n_kmers || (q.n_kmers == r.n_kmers && (q.sum_count > r.sum_count || (q.sum_count == r.sum_count && w < u)));
				}
			}
		}
		else if (uni_arm(r, c.max_bubble)) {
			kind = UNI_CLEAN_BUBBLES;
			const u32 b = uni_row_at(c, 2 * u, 0), a = uni_row_at(c, 2 * u + 1, 0);
			if (b != UNI_NONE && a != UNI_NONE && (b >> 1) != u && (a >> 1) != u && l < 4) {
				const u32 p1 = uni_row_at(c, b ^ 1u, l);
				if (p1 != UNI_NONE) {
					const u32 p = p1 ^ 1u;
					const u64 v = p >> 1;
					if (v != u) {
						const Unitig q = c.rec[v];
						ok = uni_arm(q, c.max_bubble) && uni_row_at(c, p, 0) == b && uni_row_at(c, p ^ 1u, 0) == a &&
						     (q.sum_count > r.sum_count || (q.sum_count == r.sum_count && (q.n_kmers > r.n_kmers || (q.n_kmers == r.n_kmers && v < u))));
					}
				}
			}
		}
	}
	const u64 bal = __ballot(ok);
	const u32 m8 = (u32)(bal >> (threadIdx.x & 56)) & 0xFFu;     // the 8 lanes of this unitig
	bool go = false;
	if (kind == UNI_CLEAN_ISLANDS) go = true;
	else if (kind == UNI_CLEAN_TIPS) {
		go = n_tgt >= 1 && n_tgt <= 4;
		for (u32 j = 0; j < n_tgt && j < 4; j++) go = go && ((m8 >> (2 * j)) & 3u) != 0;
	}
	else if (kind == UNI_CLEAN_BUBBLES) go = m8 != 0;
	if (!(kind & c.ops)) go = false;
	const u32 v = go ? kind : 0u;
	if (u < c.n_uni && l == 0) verdict[u] = (unsigned char)v;
	const u64 bt = __ballot(l == 0 && v == UNI_CLEAN_TIPS), bi = __ballot(l == 0 && v == UNI_CLEAN_ISLANDS), bb = __ballot(l == 0 && v == UNI_CLEAN_BUBBLES);
	if ((threadIdx.x & 63) == 0) {
		if (bt) atomicAdd(cnt + 0, (unsigned long long)__popcll(bt));
		if (bi) atomicAdd(cnt + 1, (unsigned long long)__popcll(bi));
		if (bb) atomicAdd(cnt + 2, (unsigned long long)__popcll(bb));
	}
}

// thread i < n (sc: the scanned marks).  wcnt[n]: the working counts d.cnt views; removed[n] may be null; cnt[3]: the k-mers
// removed this round
__global__ __launch_bounds__(256) void k_uni_drop(UniDev d, const u64 *pair, const UniTot *sc, const unsigned char *verdict, u64 n_uni, u32 *wcnt, unsigned char *removed, unsigned char round,
                                                  unsigned long long *cnt)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	bool go = false;
	if (i < d.n && (d.deg[i] & UNI_DEG_NODE)) {
		const UniPlace q = uni_place(pair, i);
		if ((q.h >> 1) < d.n) {
			const u64 u = sc[q.h >> 1].n;
			go = u < n_uni && verdict[u] != 0;
		}
	}
	if (go) {
		wcnt[i] = 0;
		if (removed) removed[i] = round;
	}
	const u64 b = __ballot(go);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt + 3, (unsigned long long)__popcll(b));
}
