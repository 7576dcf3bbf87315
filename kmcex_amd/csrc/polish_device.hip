// polish_device.hip -- kmx_polish_seqs*: what happens between two passes of kmx_edit_seqs' kernels, and the final gather.
//
// A pass runs the edit pipeline (edit_kernels.h, as it is) on the ACTIVE reads: a contiguous batch with offsets of its own
// and a map from its reads to the caller's (pass 1: the caller's buffers themselves, the map is the identity).  Then
//   fold:   the pass's kmx_seq_edits records are added into the reads' kmx_seq_polish records through the map; a read is
//           marked NEXT (edited, and another pass may run), PARK (it retires and has to be kept) or STAY (pass 1 found
//           nothing: it retires where it lies, in the caller's input).  On pass max_passes every length is final, so every
//           active read is written straight to its place in the output instead (the output is that pass's "parking area");
//   scan:   one exclusive scan over (reads that go on, their bytes after the edits, bytes parked) gives the next batch's
//           offsets and map and the parking offsets; its totals reach the host beside the edit count, in the pass's one wait;
//   place:  a lane per read writes the next batch's offset and map entry or the read's home, and the difference between
//           where its bytes go and where kmx_apply_edits would put them in the whole batch;
//   apply:  one streaming pass over the active bytes, a thread per 16 of them, in k_edit_apply's shape: NEXT reads are
//           written with their edits applied into the next batch, PARK reads into the parking area of this pass, the bytes of
//           STAY reads are not even loaded.
// After the last pass a scan of out_len is offsets_out, and the gather writes every read from its home, a thread per 16
// output bytes.  No kernel walks a read with one lane: the 16-byte threads find their read and their edits by binary
// search in the offsets and the sorted list, which stay in L2.
#include "hip_owned.h"
#include "launchers.h"
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace {

enum { PK_STAY = 0, PK_NEXT = 1, PK_PARK = 2 };
const u64 HOME_MASK = (1ULL << POLISH_HOME_SHIFT) - 1;

inline unsigned nblk(u64 n) { return (unsigned)((n + 255) / 256); }

struct TriPlus {
	__host__ __device__ PolishTri operator()(const PolishTri &a, const PolishTri &b) const { return PolishTri{a.n + b.n, a.next + b.next, a.park + b.park}; }
};

// an offset clamped into [0, n] where it is read; the first i in [lo, hi) whose offset exceeds p, or hi
__device__ __forceinline__ u64 p_off(const u64 *offs, u64 i, u64 n) { const u64 o = offs[i]; return o < n ? o : n; }
__device__ __forceinline__ u64 p_upper(const u64 *offs, u64 lo, u64 hi, u64 p, u64 n)
{
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (p_off(offs, mid, n) <= p) lo = mid + 1; else hi = mid;
	}
	return lo;
}
// the first edit of [lo, hi) at or behind position p, or hi; the shift of a scanned (INS low, DEL high) word (mod 2^64: added
// to a position)
__device__ __forceinline__ u64 p_edit_lower(const u64 *edits, u64 lo, u64 hi, u64 p)
{
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if ((edits[mid] >> 8) < p) lo = mid + 1; else hi = mid;
	}
	return lo;
}
__device__ __forceinline__ u64 p_shift(u64 sc) { return (sc & 0xFFFFFFFFULL) - (sc >> 32); }

// no bases: every read converged in its first pass, as an empty one
__global__ __launch_bounds__(256) void k_polish_empty(SeqPolish *rec, u64 *offs_out, u64 n_seqs)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > n_seqs) return;
	offs_out[i] = 0;
	if (i < n_seqs && rec) rec[i] = SeqPolish{1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
}

// a lane per active read; tri has n_act + 1 entries (the last one 0: the exclusive scan ends with the totals).  len[n_seqs + 1]
// holds every read's current length, the last entry 0: its scan is offsets_out.  last (this is pass max_passes): every read
// retires and is written straight to its place in the output, nothing is scanned (tri is null).
__global__ __launch_bounds__(256) void k_polish_fold(const SeqEdits *re, const u64 *offs, const u64 *ids, u64 n_act, u64 n_bytes, SeqPolish *rec, int pass, int last,
                                                     PolishTri *tri, unsigned char *kind, u64 *home, u64 *len)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > n_act) return;
	if (i == n_act) {
		if (tri) tri[i] = PolishTri{0, 0, 0};
		if (pass == 1) len[i] = 0;
		return;
	}
	const SeqEdits r = re[i];
	const u64 orig = ids ? ids[i] : i;
	const bool edited = (r.n_sub | r.n_del | r.n_ins) != 0;
	SeqPolish *P = rec + orig;
	if (pass == 1) *P = SeqPolish{1, (u64)!edited, r.n_sub, r.n_del, r.n_ins, r.out_len, r.n_windows, r.n_weak, r.n_runs, r.n_sites, r.n_ambiguous, r.n_unfixable};
	else {
		const SeqPolish o = *P;
		*P = SeqPolish{(u64)pass, (u64)!edited, o.n_sub + r.n_sub, o.n_del + r.n_del, o.n_ins + r.n_ins, r.out_len, r.n_windows, r.n_weak, r.n_runs, r.n_sites, r.n_ambiguous, r.n_unfixable};
	}
	len[orig] = r.out_len;
	const int kd = last ? PK_PARK : (edited ? PK_NEXT : (pass > 1 ? PK_PARK : PK_STAY));
	kind[i] = (unsigned char)kd;
	if (tri) tri[i] = PolishTri{(u64)(kd == PK_NEXT), kd == PK_NEXT ? r.out_len : 0, kd == PK_PARK ? r.out_len : 0};
	if (kd == PK_STAY) home[orig] = p_off(offs, i, n_bytes);
}

// INS in the low half, DEL in the high one; entry n is 0 (as k_edit_kinds of edit_device.hip)
__global__ __launch_bounds__(256) void k_polish_kinds(const u64 *edits, u64 n, u64 *kind)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	const u32 op = i < n ? (u32)(edits[i] >> 4) & 15u : 0u;
	kind[i] = (u64)(op == 3) | ((u64)(op == 2) << 32);
}

// a lane per active read (sc: the scanned tri, n_act + 1 entries; escan: the scanned kinds of the pass's n_ed sorted edits).
// delta[i]: what to add to a byte's place in the whole batch after the edits to get its place in the read's target.
// place != null (the last pass, when it is max_passes: every length is final): a read that would be parked goes straight to
// place[its original index], its offset in the output, and the "parking area" of the apply is the output itself.
__global__ __launch_bounds__(256) void k_polish_place(const u64 *offs, const u64 *ids, u64 n_act, u64 n_bytes, const unsigned char *kind, const PolishTri *sc,
                                                      const u64 *edits, u64 n_ed, const u64 *escan, int pass, const u64 *place, u64 *delta, u64 *offs_next, u64 *ids_next, u64 *home)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > n_act) return;
	const PolishTri s = sc ? sc[i] : PolishTri{0, 0, 0};              // (null: the last pass)
	if (i == n_act) { if (offs_next) offs_next[s.n] = s.next; return; }   // (null: no read goes on)
	const int kd = kind[i];
	if (kd == PK_STAY) return;
	const u64 orig = ids ? ids[i] : i, start = p_off(offs, i, n_bytes);
	const u64 g = start + p_shift(escan[p_edit_lower(edits, 0, n_ed, start)]);
	const u64 base = kd == PK_NEXT ? s.next : (place ? place[orig] : s.park);
	delta[i] = base - g;
	if (kd == PK_NEXT) { offs_next[s.n] = base; ids_next[s.n] = orig; }
	else home[orig] = (u64)(place ? POLISH_HOME_PLACED : pass) << POLISH_HOME_SHIFT | (base & HOME_MASK);
}

// A thread per 16 active bytes.  One 16-byte copy when they lie in one read and no edit falls among them, byte by byte
// otherwise (the seams between reads, the neighbourhood of an edit).  Two lanes of the workgroup search the whole offsets and
// the whole list for the ends of its 4096 bytes; every thread then searches between what they found (a few steps).  Nothing
// is written at or behind next[next_cap] / park[park_cap], whatever offsets and list hold.
__global__ __launch_bounds__(256) void k_polish_apply(const unsigned char *in, u64 n_bytes, const u64 *offs, u64 n_act, const unsigned char *kind, const u64 *delta,
                                                      const u64 *edits, u64 n_ed, const u64 *escan, unsigned char *next, u64 next_cap, unsigned char *park, u64 park_cap)
{
	__shared__ u64 s_u[2], s_e[2];
	const u64 t0 = (u64)blockIdx.x * 4096, t1 = t0 + 4096 < n_bytes ? t0 + 4096 : n_bytes;   // (t0 < n_bytes: the grid covers n_bytes)
	if (threadIdx.x == 0) { s_u[0] = p_upper(offs, 0, n_act + 1, t0, n_bytes); s_e[0] = p_edit_lower(edits, 0, n_ed, t0); }
	if (threadIdx.x == 64) { s_u[1] = p_upper(offs, 0, n_act + 1, t1 - 1, n_bytes); s_e[1] = p_edit_lower(edits, 0, n_ed, t1); }
	__syncthreads();
	const u64 b0 = t0 + (u64)threadIdx.x * 16;
	if (b0 >= n_bytes) return;
	const u64 b1 = b0 + 16 < n_bytes ? b0 + 16 : n_bytes;
	const u64 u_lo = s_u[0], u_hi = s_u[1] > s_u[0] ? s_u[1] : s_u[0], e_lo = s_e[0], e_hi = s_e[1] > s_e[0] ? s_e[1] : s_e[0];
	u64 u = p_upper(offs, u_lo, u_hi, b0, n_bytes);                 // read u - 1 holds b0 when 1 <= u <= n_act and it starts at or before b0
	const bool whole = u >= 1 && u <= n_act && p_off(offs, u - 1, n_bytes) <= b0 && p_off(offs, u, n_bytes) >= b1;
	if (whole && kind[u - 1] == PK_STAY) return;
	u64 i = p_edit_lower(edits, e_lo, e_hi, b0);
	const u64 i1 = p_edit_lower(edits, i, e_hi, b1);
	u64 o = b0 + p_shift(escan[i]);                                  // the place of byte b0 in the whole batch after the edits
	if (whole && i == i1 && b1 - b0 == 16) {
		const bool nx = kind[u - 1] == PK_NEXT;
		const u64 d = o + delta[u - 1], cap = nx ? next_cap : park_cap;
		if (d <= cap && cap - d >= 16) {
			uint4 v;
			__builtin_memcpy(&v, in + b0, 16);
			__builtin_memcpy((nx ? next : park) + d, &v, 16);
			return;
		}
	}
	u64 cur = ~0ULL, dl = 0, cap = 0;                                // the read the bytes are in, its target
	unsigned char *tgt = nullptr;
	for (u64 p = b0; p < b1; p++) {
		while (u <= n_act && p_off(offs, u, n_bytes) <= p) u++;
		if (u != cur) {
			cur = u;
			tgt = nullptr;
			if (u >= 1 && u <= n_act && p_off(offs, u - 1, n_bytes) <= p) {
				const int kd = kind[u - 1];
				if (kd != PK_STAY) { tgt = kd == PK_NEXT ? next : park; cap = kd == PK_NEXT ? next_cap : park_cap; dl = delta[u - 1]; }
			}
		}
		u32 c = in[p];
		bool drop = false;
		for (; i < i1 && (edits[i] >> 8) == p; i++) {
			const u32 op = (u32)(edits[i] >> 4) & 15u, b = (u32)"ACGT"[edits[i] & 3];
			if (op == 1) c = b;
			else if (op == 2) drop = true;
			else if (op == 3) { if (tgt && o + dl < cap) tgt[o + dl] = (unsigned char)b; o++; }
		}
		if (drop) continue;
		if (tgt && o + dl < cap) tgt[o + dl] = (unsigned char)c;
		o++;
	}
}

// A thread per 16 output bytes of out[0, n_out), n_out <= the capacity: the reads in the caller's order, each from its home
// (a read the last pass wrote straight to its place has none: area POLISH_HOME_PLACED).  offs_out is this call's own scan
// (non-decreasing); a read's bytes [home, home + out_len) lie inside its area.  The searches are narrowed as in k_polish_apply.
__global__ __launch_bounds__(256) void k_polish_gather(PolishHomes hm, const u64 *home, const u64 *offs_out, u64 n_seqs, unsigned char *out, u64 n_out)
{
	__shared__ u64 s_u[2];
	const u64 t0 = (u64)blockIdx.x * 4096, t1 = t0 + 4096 < n_out ? t0 + 4096 : n_out;
	if (threadIdx.x == 0) s_u[0] = p_upper(offs_out, 0, n_seqs + 1, t0, ~0ULL);
	if (threadIdx.x == 64) s_u[1] = p_upper(offs_out, 0, n_seqs + 1, t1 - 1, ~0ULL);
	__syncthreads();
	const u64 o0 = t0 + (u64)threadIdx.x * 16;
	if (o0 >= n_out) return;
	const u64 o1 = o0 + 16 < n_out ? o0 + 16 : n_out;
	u64 u = p_upper(offs_out, s_u[0], s_u[1] > s_u[0] ? s_u[1] : s_u[0], o0, ~0ULL);   // read u - 1 holds o0
	if (u < 1 || u > n_seqs) return;
	if (o1 - o0 == 16 && offs_out[u] >= o1) {
		const u64 h = home[u - 1];
		if ((h >> POLISH_HOME_SHIFT) > POLISH_MAX_PASSES) return;
		uint4 v;
		__builtin_memcpy(&v, hm.area[h >> POLISH_HOME_SHIFT] + (h & HOME_MASK) + (o0 - offs_out[u - 1]), 16);
		__builtin_memcpy(out + o0, &v, 16);
		return;
	}
	u64 cur = 0, s0 = 0;
	const unsigned char *src = nullptr;
	for (u64 o = o0; o < o1; o++) {
		while (u <= n_seqs && offs_out[u] <= o) u++;
		if (u > n_seqs) return;
		if (u != cur) {
			cur = u;
			const u64 h = home[u - 1];
			src = (h >> POLISH_HOME_SHIFT) > POLISH_MAX_PASSES ? nullptr : hm.area[h >> POLISH_HOME_SHIFT] + (h & HOME_MASK);
			s0 = offs_out[u - 1];
		}
		if (src) out[o] = src[o - s0];
	}
}

}   // namespace

namespace kmxk {

void polish_empty(SeqPolish *rec, u64 *offs_out, u64 n_seqs, hipStream_t st)
{
	hipLaunchKernelGGL(k_polish_empty, dim3(nblk(n_seqs + 1)), dim3(256), 0, st, rec, offs_out, n_seqs);
}

// after the sites of pass `pass` over the active reads: records folded, lengths and kinds written; tri[0, n_act] scanned into
// sc, sc[n_act] holds the totals (not on the last pass of max_passes: tri and sc are null)
hipError_t polish_fold(const SeqEdits *re, const u64 *offs, const u64 *ids, u64 n_act, u64 n_bytes, SeqPolish *rec, int pass, bool last, PolishTri *tri, PolishTri *sc,
                       unsigned char *kind, u64 *home, u64 *len, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	hipLaunchKernelGGL(k_polish_fold, dim3(nblk(n_act + 1)), dim3(256), 0, st, re, offs, ids, n_act, n_bytes, rec, pass, (int)last, tri, kind, home, len);
	if (!tri) return hipGetLastError();
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const PolishTri *)tri, sc, PolishTri{0, 0, 0}, (size_t)(n_act + 1), TriPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const PolishTri *)tri, sc, PolishTri{0, 0, 0}, (size_t)(n_act + 1), TriPlus(), st));
	return hipGetLastError();
}

// the pass's sorted list applied: escan has room for 2 (n_ed + 1) words; place: see k_polish_place (then park / park_cap are the output's)
hipError_t polish_apply(const unsigned char *in, const u64 *offs, const u64 *ids, u64 n_act, u64 n_bytes, const unsigned char *kind, const PolishTri *sc, const u64 *edits, u64 n_ed,
                        u64 *escan, int pass, const u64 *place, u64 *delta, unsigned char *next, u64 next_cap, u64 *offs_next, u64 *ids_next, unsigned char *park, u64 park_cap, u64 *home,
                        DevBuf<unsigned char> &tmp, hipStream_t st)
{
	u64 *ek = escan + (n_ed + 1);
	hipLaunchKernelGGL(k_polish_kinds, dim3(nblk(n_ed + 1)), dim3(256), 0, st, edits, n_ed, ek);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const u64 *)ek, escan, (u64)0, (size_t)(n_ed + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const u64 *)ek, escan, (u64)0, (size_t)(n_ed + 1), rocprim::plus<u64>(), st));
	hipLaunchKernelGGL(k_polish_place, dim3(nblk(n_act + 1)), dim3(256), 0, st, offs, ids, n_act, n_bytes, kind, sc, edits, n_ed, (const u64 *)escan, pass, place, delta, offs_next, ids_next, home);
	if (n_bytes) hipLaunchKernelGGL(k_polish_apply, dim3(nblk((n_bytes + 15) / 16)), dim3(256), 0, st, in, n_bytes, offs, n_act, kind, (const u64 *)delta, edits, n_ed, (const u64 *)escan, next, next_cap, park, park_cap);
	return hipGetLastError();
}

// offs_out[0, n_seqs] = the running sum of the lengths len[0, n_seqs] (len[n_seqs] = 0)
hipError_t polish_offsets(const u64 *len, u64 n_seqs, u64 *offs_out, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, len, offs_out, (u64)0, (size_t)(n_seqs + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, len, offs_out, (u64)0, (size_t)(n_seqs + 1), rocprim::plus<u64>(), st));
	return hipGetLastError();
}

void polish_gather(const PolishHomes &hm, const u64 *home, const u64 *offs_out, u64 n_seqs, unsigned char *out, u64 n_out, hipStream_t st)
{
	if (n_out) hipLaunchKernelGGL(k_polish_gather, dim3(nblk((n_out + 15) / 16)), dim3(256), 0, st, hm, home, offs_out, n_seqs, out, n_out);
}

}   // namespace kmxk
