// map_kernels.h -- kmx_unitig_map_*: where the windows of a batch of reads lie on the unitigs of a listing (the rule:
// include/kmx.h; the host side: map_host.h; the launchers: unitig_device.hip).
//
// The listing is the membership structure (uni_find, unitig_kernels.h); beside it a session keeps one PLACE per entry: the
// unitig that holds it, where, and in which orientation.  The kernels, in the order the host runs them:
//   k_map_mu       per unitig: its number of windows m_u; a unitig shorter than k raises the error word;
//   k_map_index    per byte of the unitig set: the window that starts there, canonicalised, looked up, and its place stored
//                  with a compare-and-swap from "no place"; a byte outside ACGT, a miss or a lost swap raises the error word;
// and per chunk of windows of a batch of reads
//   k_map_windows  the hot kernel, in the tile shape of k_count_windows (256 lanes x 16 consecutive windows, base codes staged
//                  in LDS, sequence boundaries from the clamped offsets): per window the canonical key, uni_find, the place
//                  gather, and its code o << 32 | off (MAP_NONE when it is not mapped).  Stepping one base along a unitig adds
//                  1 to the code, so "the neighbour continues my segment" is code[p - 1] + 1 == code[p].  A lane adds its run's
//                  hits to a unitig with one integer atomic per change of unitig;
//   (a scan of the start flags, read straight from the codes: unitig_device.hip)
//   k_map_starts   per window that starts a segment: its slot from the scan, pos / o / off, and what the read's record and its
//                  segment count take from a start;
//   k_map_ends     per window that ends one (looking one window back, so the chunk's last window waits for the next chunk):
//                  n_windows from the start's position, and what the record takes from an end;
//   k_map_advance  one thread: the segments so far, the start of the segment still open, the chunk's last code.
// Every decision looks at one window and its neighbour, so the list is a function of (listing, unitig set, reads) alone.  No
// lane walks a read or a unitig.  Every store is checked against its capacity; every offset is clamped where it is read.
#pragma once
#include "unitig_kernels.h"

static constexpr int MAP_BT = 256;
static constexpr int MAP_RUN = 16;                                  // consecutive windows rolled by one lane
static constexpr int MAP_WIN = MAP_BT * MAP_RUN;                   // windows per block
static constexpr int MAP_TILE = MAP_WIN + 64;                      // + the k - 1 <= 62 bases of the block's last window

// the offsets of kmx_query_seqs_dev, clamped where they are read (kernels.hip: seq_off, seq_upper, seq_code)
__device__ __forceinline__ u64 map_off(const u64 *offs, u64 i, u64 n_bases) { const u64 o = offs[i]; return o < n_bases ? o : n_bases; }
// first i in [lo, hi) with map_off(i) > p, or hi; reads only offs[lo, hi) whatever the entries hold
__device__ __forceinline__ u64 map_upper(const u64 *offs, u64 lo, u64 hi, u64 p, u64 n_bases)
{
	while (lo < hi) {
		const u64 mid = lo + (hi - lo) / 2;
		if (map_off(offs, mid, n_bases) <= p) lo = mid + 1; else hi = mid;
	}
	return lo;
}
__device__ __forceinline__ u32 map_code(u32 c) { return c == 'A' ? 0u : (c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 4u))); }
// the read that holds position p and where it starts; false when no read does
__device__ __forceinline__ bool map_read_of(const u64 *offs, u64 n_seqs, u64 n_bases, u64 p, u64 *r, u64 *start)
{
	const u64 u = map_upper(offs, 0, n_seqs + 1, p, n_bases);
	if (u < 1 || u > n_seqs) return false;
	*r = u - 1;
	*start = map_off(offs, u - 1, n_bases);
	return *start <= p;
}

// ---- the index

// thread u < U: mu[u] = the windows of unitig u; none, or 2^31 and more, is an error
__global__ __launch_bounds__(256) void k_map_mu(MapDev M, const u64 *uoffs, u64 n_ubases)
{
	const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
	if (u >= M.U) return;
	const u64 a = map_off(uoffs, u, n_ubases), b = map_off(uoffs, u + 1, n_ubases), len = b > a ? b - a : 0;
	const u64 m = len >= (u64)M.d.k ? len - (u64)M.d.k + 1 : 0;
	if (m == 0 || m >> 31) *M.d.err = 1;
	M.mu[u] = (u32)(m >> 31 ? 0 : m);
}

// thread p < n_ubases: the window of the unitig set that starts at byte p, if one does
template <int W> __global__ __launch_bounds__(256) void k_map_index(MapDev M, const unsigned char *useq, const u64 *uoffs, u64 n_ubases)
{
	const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
	if (p >= n_ubases) return;
	u64 u = 0, a = 0;
	if (!map_read_of(uoffs, M.U, n_ubases, p, &u, &a)) return;
	const u64 b = map_off(uoffs, u + 1, n_ubases), k = (u64)M.d.k;
	if (b < a + k || M.mu[u] == 0) return;                          // (k_map_mu has raised the error)
	const u64 j = p - a;
	if (p + k > b) {                                                // the last k - 1 bytes start no window; they are still bytes of the set
		if (map_code(useq[p]) > 3u) *M.d.err = 1;
		return;
	}
	UniK x{0, 0};
	bool bad = false;
	for (u64 t = 0; t < k; t++) {
		const u32 c = map_code(useq[p + t]);
		bad = bad || c > 3u;
		x = UniK{(x.hi << 2) | (x.lo >> 62), (x.lo << 2) | (c & 3u)};
	}
	if (bad) { *M.d.err = 1; return; }
	const UniK r = uni_rc(x, M.d.k);
	const bool fwd = !uni_less(r, x);
	const u32 i = uni_find<W>(M.d, fwd ? x : r);
	if (i == UNI_NONE) { *M.d.err = 1; return; }
	const u64 val = u << 32 | (fwd ? 0ULL : 1ULL << 31) | j;
	if (atomicCAS((unsigned long long *)&M.place[i], (unsigned long long)MAP_NONE, (unsigned long long)val) != (unsigned long long)MAP_NONE) *M.d.err = 1;
}

// ---- a chunk of windows [p0, p0 + n_win) of the reads (v: kmx_types.h SeqView; the bases on hand must hold every window of
// the chunk that fits in its read)

// code[1 + i] = the code of window p0 + i for every i < n_win; hits (may be null) += the mapped windows per unitig
template <int W> __global__ __launch_bounds__(MAP_BT) void k_map_windows(MapDev M, SeqView v, u64 p0, u64 n_win, u64 *code, unsigned long long *hits)
{
	__shared__ unsigned char s_code[MAP_TILE];
	__shared__ u64 s_u[2];
	const int tid = threadIdx.x, k = M.d.k;
	const u64 t0 = p0 + (u64)blockIdx.x * MAP_WIN, p_end = p0 + n_win;
	if (t0 >= p_end) return;
	const u64 t_last = (t0 + MAP_WIN < p_end ? t0 + MAP_WIN : p_end) - 1;
	const u64 b_end = t0 + MAP_WIN + k - 1 < v.g1 ? t0 + MAP_WIN + k - 1 : v.g1;   // the bases this block reads: [t0, b_end)
	if (tid == 0) s_u[0] = map_upper(v.offs, 0, v.n_seqs + 1, t0, v.n_total);
	if (tid == 64) s_u[1] = map_upper(v.offs, 0, v.n_seqs + 1, t_last, v.n_total);
	const unsigned char *src = v.seq + (t0 - v.g0);
	const int nb = b_end > t0 ? (int)(b_end - t0) : 0;
	if (((uintptr_t)src & 3) == 0) {
		for (int j = 4 * tid; j < nb; j += 4 * MAP_BT) {
			if (j + 4 <= nb) {
				const u32 w = *(const u32 *)(src + j);
#pragma unroll
				for (int q = 0; q < 4; q++) s_code[j + q] = (unsigned char)map_code(((w >> (8 * q)) & 0xFFu) & ~0x20u);
			} else
				for (int q = j; q < nb; q++) s_code[q] = (unsigned char)map_code(src[q] & ~0x20u);
		}
	} else
		for (int j = tid; j < nb; j += MAP_BT) s_code[j] = (unsigned char)map_code(src[j] & ~0x20u);
	__syncthreads();

	const u64 q0 = t0 + (u64)tid * MAP_RUN;                          // this lane's first window
	if (q0 >= p_end) return;
	const u64 u0 = s_u[0], u1 = s_u[1];
	u64 u = map_upper(v.offs, u0, u1 > u0 ? u1 : u0, q0, v.n_total);  // sequence u - 1 holds q0 (when 1 <= u <= n_seqs)
	bool in_seq = u >= 1 && u <= v.n_seqs && map_off(v.offs, u - 1, v.n_total) <= q0;
	u64 nxt = u <= v.n_seqs ? map_off(v.offs, u, v.n_total) : ~0ULL;  // where the next sequence starts
	const u64 lmask = k >= 32 ? ~0ULL : (1ULL << (2 * (k & 31))) - 1;
	const u64 hmask = k > 32 ? (1ULL << (2 * k - 64)) - 1 : 0;
	const int rsh = W == 1 ? 2 * k - 2 : 2 * k - 66;
	u64 f_lo = 0, f_hi = 0, r_lo = 0, r_hi = 0;
	int len = 0;                                                     // bases of the current run, up to k
	auto step = [&](u64 j) {
		while (u <= v.n_seqs && nxt <= j) {                          // j starts a later sequence
			u++;
			nxt = u <= v.n_seqs ? map_off(v.offs, u, v.n_total) : ~0ULL;
			in_seq = u <= v.n_seqs;
			len = 0;
		}
		const u32 c = (j < b_end && in_seq) ? (u32)s_code[j - t0] : 4u;
		if (c > 3u) { len = 0; return; }
		if (W == 1) {
			f_lo = ((f_lo << 2) | c) & lmask;
			r_lo = (r_lo >> 2) | ((u64)(3u - c) << rsh);
		} else {
			f_hi = ((f_hi << 2) | (f_lo >> 62)) & hmask;
			f_lo = (f_lo << 2) | c;
			r_lo = (r_lo >> 2) | (r_hi << 62);
			r_hi = (r_hi >> 2) | ((u64)(3u - c) << rsh);
		}
		len = len < k ? len + 1 : k;
	};
	for (int i = 0; i < k - 1; i++) step(q0 + (u64)i);
	u64 hit_u = ~0ULL;                                               // the unitig of the lane's last mapped windows, and how many
	unsigned long long hit_n = 0;
#pragma unroll 4
	for (int r = 0; r < MAP_RUN; r++) {
		step(q0 + (u64)(k - 1 + r));
		if (q0 + r >= p_end) break;
		u64 c = MAP_NONE;
		if (len >= k) {
			const bool fwd = W == 1 ? f_lo <= r_lo : (f_hi < r_hi || (f_hi == r_hi && f_lo <= r_lo));
			const u32 i = uni_find<W>(M.d, fwd ? UniK{f_hi, f_lo} : UniK{r_hi, r_lo});
			const u64 pl = i != UNI_NONE ? M.place[i] : MAP_NONE;
			const u64 un = pl >> 32;
			if (pl != MAP_NONE && un < M.U) {
				const u32 j = (u32)pl & 0x7FFFFFFFu, d = ((u32)(pl >> 31) & 1u) ^ (fwd ? 0u : 1u);
				const u32 off = d ? M.mu[un] - 1u - j : j;
				c = (2 * un + d) << 32 | off;
				if (hits) {
					if (un != hit_u) {
						if (hit_n) atomicAdd(hits + hit_u, hit_n);
						hit_u = un;
						hit_n = 0;
					}
					hit_n++;
				}
			}
		}
		code[1 + (q0 + r - p0)] = c;
	}
	if (hit_n) atomicAdd(hits + hit_u, hit_n);
}

// the start flag of window p0 + i from the codes (i == n_win: 0, so that the exclusive scan ends with the chunk's total)
struct MapStartFlag {
	const u64 *code;
	u64 n_win;
	__host__ __device__ u32 operator()(u64 i) const
	{
		if (i >= n_win) return 0u;
		const u64 c0 = code[i], c1 = code[i + 1];
		return c1 != MAP_NONE && (c0 == MAP_NONE || c0 + 1 != c1) ? 1u : 0u;
	}
};

// thread i < n_win: window p0 + i, if it starts a segment
__global__ __launch_bounds__(256) void k_map_starts(MapChunk C, MapOut O, const u64 *offs, u64 n_seqs, u64 n_total, u64 p0, u64 n_win)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_win) return;
	const u64 c0 = C.code[i], c1 = C.code[i + 1];
	if (c1 == MAP_NONE || (c0 != MAP_NONE && c0 + 1 == c1)) return;
	const u64 p = p0 + i, l = C.ex[i], g = C.state[0] + l;
	if (l < n_win) C.spos[l] = p;
	if (O.segs && g < O.cap) {
		MapSeg *s = O.segs + g;
		s->pos = p;
		s->o = (u32)(c1 >> 32);
		s->off = (u32)c1;
		s->reserved = 0;
	}
	u64 r = 0, start = 0;
	if (!map_read_of(offs, n_seqs, n_total, p, &r, &start)) return;
	atomicAdd((unsigned long long *)(O.so + r), 1ULL);
	if (O.rec) {
		const u64 w = p - start;
		atomicMin((unsigned long long *)&O.rec[r].first_mapped, (unsigned long long)w);
		if (c0 == MAP_NONE && w > 0) atomicAdd((unsigned long long *)&O.rec[r].n_gaps, 1ULL);
	}
}

// thread i < n_win: window p0 - 1 + i, if it ends a segment
__global__ __launch_bounds__(256) void k_map_ends(MapChunk C, MapOut O, const u64 *offs, u64 n_seqs, u64 n_total, u64 p0, u64 n_win)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_win) return;
	const u64 c = C.code[i], nx = C.code[i + 1];
	if (c == MAP_NONE || nx == c + 1 || p0 + i == 0) return;
	const u64 p = p0 + i - 1, e = C.ex[i], base = C.state[0];        // e: the segments of the chunk that start at or before p
	if (e == 0 && base == 0) return;                                 // (cannot be: a mapped window lies in a segment)
	const u64 sp = e ? (e - 1 < n_win ? C.spos[e - 1] : p) : C.state[1], g = base + e - 1;
	const u64 nw = p >= sp ? p - sp + 1 : 0;
	if (O.segs && g < O.cap) O.segs[g].n_windows = (u32)nw;
	if (!O.rec) return;
	u64 r = 0, start = 0;
	if (!map_read_of(offs, n_seqs, n_total, p, &r, &start)) return;
	atomicAdd((unsigned long long *)&O.rec[r].n_mapped, (unsigned long long)nw);
	atomicMax((unsigned long long *)&O.rec[r].longest, (unsigned long long)nw);
	atomicMax((unsigned long long *)&O.rec[r].last_mapped, (unsigned long long)(p - start));
}

// one thread, behind the two kernels above
__global__ void k_map_advance(MapChunk C, u64 n_win)
{
	const u64 t = C.ex[n_win];
	if (t && t <= n_win) C.state[1] = C.spos[t - 1];
	C.state[0] += t;
	C.code[0] = C.code[n_win];
}

// ---- the records: before the first chunk ...
__global__ __launch_bounds__(256) void k_map_rec_init(SeqMap *rec, u64 n_seqs)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < n_seqs) rec[i] = SeqMap{0, 0, 0, 0, ~0ULL, 0, 0, 0};
}

// ... and behind the last one, while so[] still holds the segments per read
__global__ __launch_bounds__(256) void k_map_rec_finish(SeqMap *rec, const u64 *so, const u64 *offs, u64 n_seqs, u64 n_total, int k)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_seqs) return;
	const u64 a = map_off(offs, i, n_total), b = map_off(offs, i + 1, n_total), len = b > a ? b - a : 0;
	SeqMap r = rec[i];
	r.n_windows = len >= (u64)k ? len - (u64)k + 1 : 0;
	r.n_segments = so[i];
	if (r.first_mapped == ~0ULL) r.first_mapped = r.last_mapped = r.n_windows;
	else if (r.first_mapped > 0 && r.n_gaps > 0) r.n_gaps--;         // the first mapped window is no gap
	rec[i] = r;
}
