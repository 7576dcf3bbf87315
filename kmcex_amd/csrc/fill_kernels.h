// fill_kernels.h -- kmx_unitig_scaffold_fill*: the scaffolds of kmx_unitig_scaffold spelled again with the gaps filled that
// kmx_unitig_pair_paths found a path for (the rule: include/kmx.h; the host side: fill_host.h; the launchers: unitig_device.hip).
// The kernels, in the order the host runs them:
//   k_fill_heads  one lane per scaffold: tot[first_step].n = 1 (tot is zero before);
//   k_fill_kind   one lane per step: the two lower-bound searches for its link's entry, the record, the kind, and what the step
//                 writes: bytes, pieces, piece bytes.  Its loop over a path is bounded by PP_MAX_STEPS.  The eight counters are
//                 summed in LDS, one global atomic per block and counter;
//   (one rocPRIM scan of tot into sc: per step the scaffolds, bytes, pieces and piece bytes in front of it and the last step in
//   front of it that starts a scaffold; sc[U] holds the totals the host waits for)
//   k_fill_place  one lane per step: fsteps, the ubase word of its unitig (CTG_FIRST on HEAD and N steps, so ctg_emit_tile with
//                 later_skip = k - 1 writes every step's own bytes), its pieces (oriented unitig, destination, exclusive piece-byte
//                 prefix) and its share of the scaffold's record by integer atomics (frec is zero before);
//   k_fill_step_emit   the steps' own bytes: the tile emit of the contigs over fseq, which holds 'N' before;
//   k_fill_emit   THE PATH PIECES.  A repeat unitig lies on many paths and is written many times, so this emit is tiled over the
//                 OUTPUT: a block takes FILL_TILE piece bytes, finds its first piece by one binary search in pc_pre, and takes the
//                 pieces of its tile FILL_NB at a time into LDS; a scan of the aligned 16-byte output words each of them covers,
//                 then one lane per word: it gathers from useq, forward or backwards and complemented (ctg_comp4).  Edge words are
//                 written byte by byte inside the piece only, so the N and the step bytes beside it stay.  No lane's work grows
//                 with the length of a unitig or of a path.
// Every index read from the caller's arrays is clamped or checked where it is read and every store is checked against its
// capacity: bad device input gives wrong strings, never an access outside a buffer.  A link beside a unitig shorter than k (only
// the device form lets one in) is an N step, so the start of a step's whole string never lies in front of its scaffold.
#pragma once
#include "contig_kernels.h"

static constexpr int FILL_TILE = 4096;                         // piece bytes per block of k_fill_emit
static constexpr int FILL_NB = 1024;                           // pieces taken into LDS at a time
static constexpr u32 FILL_NO_ENTRY = 0xFFFFFFFFu;

// the clamped start and bytes of unitig u < U
__device__ __forceinline__ u64 fill_len(const FillDev &D, u64 u, u64 *so)
{
	const u64 a = ctg_min(D.uoffs[u], D.n_ubases), b = ctg_min(D.uoffs[u + 1], D.n_ubases);
	*so = a;
	return b > a ? b - a : 0;
}
// the bytes of oriented unitig o, 0 for what is no unitig
__device__ __forceinline__ u64 fill_olen(const FillDev &D, u32 o)
{
	u64 so;
	return (u64)o < 2 * D.U ? fill_len(D, o >> 1, &so) : 0;
}
// the entry with (a, b), or FILL_NO_ENTRY: a lower-bound search on a << 32 | b
__device__ __forceinline__ u32 fill_find(const FillDev &D, u32 a, u32 b)
{
	const u64 key = (u64)a << 32 | b;
	u64 lo = 0, hi = D.n_plinks;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		const PairLink E = D.plinks[mid];
		if (((u64)E.a << 32 | E.b) < key) lo = mid + 1; else hi = mid;
	}
	if (lo >= D.n_plinks) return FILL_NO_ENTRY;
	const PairLink E = D.plinks[lo];
	return E.a == a && E.b == b ? (u32)lo : FILL_NO_ENTRY;
}

// what step i >= 1 that starts no scaffold is: its link's entry, whether that is the mirror, the kind, the steps of its path (t,
// from psteps[fs]) and the bytes of the path's pieces
struct FillLink {
	u32 entry, kind, t;
	bool mirror;
	u64 fs, front;
};
// step j < t of the link's path: as it stands through the entry, reversed and flipped through the mirror
__device__ __forceinline__ u32 fill_path_step(const FillDev &D, const FillLink &L, u32 j) { return L.mirror ? D.psteps[L.fs + (L.t - 1 - j)] ^ 1u : D.psteps[L.fs + j]; }

__device__ __forceinline__ FillLink fill_link(const FillDev &D, u32 p, u32 q)
{
	FillLink L{FILL_NO_ENTRY, FILL_N, 0, false, 0, 0};
	u32 e = fill_find(D, p, q);
	if (e == FILL_NO_ENTRY) {
		e = fill_find(D, q ^ 1u, p ^ 1u);
		L.mirror = e != FILL_NO_ENTRY;
	}
	L.entry = e;
	const u64 k = (u64)D.k;
	if (e == FILL_NO_ENTRY || fill_olen(D, p) < k || fill_olen(D, q) < k) return L;
	const PairPath R = D.precs[e];
	if (R.verdict == PP_ADJACENT && (D.kinds & 2)) { L.kind = FILL_ADJACENT; return L; }
	if (R.verdict != PP_PATH || !(D.kinds & 1) || R.n_steps < 1 || R.n_steps > PP_MAX_STEPS || R.first_step > D.n_psteps || (u64)R.n_steps > D.n_psteps - R.first_step) return L;
	L.t = R.n_steps;
	L.fs = R.first_step;
	bool ok = true;
	u64 front = 0;
	for (u32 j = 0; j < L.t; j++) {                                // (the steps' own order: the sum is the same either way)
		const u64 len = fill_olen(D, D.psteps[L.fs + j]);
		ok = ok && len >= k;
		front += len - (k - 1);
	}
	if (!ok) { L.t = 0; L.fs = 0; return L; }
	L.kind = FILL_PATH;
	L.front = front;
	return L;
}

// thread s < S (D.tot is zero before)
__global__ __launch_bounds__(256) void k_fill_heads(FillDev D)
{
	const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
	if (s >= D.S) return;
	const u64 f = D.srec[s].first_step;
	if (f < D.U) D.tot[f].n = 1;                                   // (every writer stores the same value)
}

// thread i < U; step 0 starts a scaffold whatever srec says
__global__ __launch_bounds__(256) void k_fill_kind(FillDev D)
{
	__shared__ unsigned long long s_cnt[FILL_C_N];
	if (threadIdx.x < FILL_C_N) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i < D.U) {
		const bool head = i == 0 || D.tot[i].n != 0;
		const ScfStep q = D.steps[i];
		const u64 len = fill_olen(D, q.o);
		FillTot t{head ? 1u : 0u, len, 0, 0, head ? i : 0};
		u32 kind = FILL_HEAD;
		if (!head) {
			const FillLink L = fill_link(D, D.steps[i - 1].o, q.o);
			kind = L.kind;
			if (kind == FILL_N) t.len = len + q.n_gap;
			else {
				t.len = L.front + (len - (u64)(D.k - 1));
				t.np = L.t;
				t.pb = L.front;
				atomicAdd(&s_cnt[FILL_C_REMOVED], (unsigned long long)q.n_gap);
				atomicAdd(&s_cnt[FILL_C_FILLED], (unsigned long long)L.front);
			}
			if (L.entry == FILL_NO_ENTRY) atomicAdd(&s_cnt[FILL_C_NO_ENTRY], 1ULL);
			if (L.mirror) atomicAdd(&s_cnt[FILL_C_MIRROR], 1ULL);
		}
		atomicAdd(&s_cnt[kind], 1ULL);
		D.tot[i] = t;
	}
	__syncthreads();
	if (threadIdx.x < FILL_C_N && s_cnt[threadIdx.x]) atomicAdd(D.cnt + threadIdx.x, s_cnt[threadIdx.x]);
}

// thread i <= U (D.sc: the scan of D.tot; D.frec is zero and D.ubase all ones before)
__global__ __launch_bounds__(256) void k_fill_place(FillDev D)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i > D.U) return;
	const FillTot at = D.sc[i];
	if (i == D.U) {
		if (at.n <= D.S) D.foffs[at.n] = at.len;
		if (at.np <= D.n_pc) D.pc_pre[at.np] = at.pb;
		return;
	}
	const FillTot me = D.tot[i];
	const bool head = me.n != 0;
	const u64 c = at.n + me.n - 1, soff = D.sc[head ? i : ctg_min(at.first, D.U)].len, pos = at.len - soff;
	const ScfStep q = D.steps[i];
	FillLink L{FILL_NO_ENTRY, FILL_HEAD, 0, false, 0, 0};
	if (!head) L = fill_link(D, D.steps[i - 1].o, q.o);
	const u64 km1 = (u64)(D.k - 1);
	const u64 n_front = head ? 0 : L.kind == FILL_N ? (u64)q.n_gap : L.front;
	const u64 off = head || L.kind == FILL_N ? pos + n_front : pos + n_front - km1;
	D.fsteps[i] = FillStep{q.o, L.kind, L.entry, L.t, off, n_front};
	if ((u64)q.o < 2 * D.U) D.ubase[q.o >> 1] = ((soff + off) & (CTG_FIRST - 1)) | ((q.o & 1u) ? CTG_REV : 0) | (head || L.kind == FILL_N ? CTG_FIRST : 0);
	u64 run = 0;
	for (u32 j = 0; j < L.t; j++) {
		const u32 v = fill_path_step(D, L, j);
		const u64 x = at.np + j;
		if (x < D.n_pc) {
			D.pc_o[x] = v;
			D.pc_dst[x] = soff + pos + run;
			D.pc_pre[x] = at.pb + run;
		}
		if (D.pieces && x < D.piece_cap) D.pieces[x] = v;
		run += fill_olen(D, v) - km1;
	}
	if (c >= D.S) return;
	ScfFill *R = D.frec + c;
	atomicAdd((unsigned long long *)&R->n_bases, (unsigned long long)me.len);
	if (head) {
		D.foffs[c] = soff;
		R->first_piece = at.np;                                    // (nothing adds to it)
		return;
	}
	if (L.kind == FILL_N) {
		atomicAdd((unsigned long long *)&R->n_gap_bases, (unsigned long long)q.n_gap);
		atomicAdd((unsigned long long *)&R->n_n_links, 1ULL);
		return;
	}
	atomicAdd((unsigned long long *)(L.kind == FILL_PATH ? &R->n_path_links : &R->n_adjacent_links), 1ULL);
	if (L.t) {
		atomicAdd((unsigned long long *)&R->n_fill_bases, (unsigned long long)L.front);
		atomicAdd((unsigned long long *)&R->n_pieces, (unsigned long long)L.t);
	}
}

// one block per tile of CTG_TILE input bytes; fseq[0, n_fbases) holds 'N' before
__global__ __launch_bounds__(256) void k_fill_step_emit(FillDev D)
{
	ctg_emit_tile(D.useq, D.uoffs, D.U, D.n_ubases, D.ubase, (u64)(D.k - 1), D.fseq, D.seq_cap);
}

// piece i of the LDS chunk inside the tile [t0, t1) of piece bytes: its bytes r in [ra, rb) go to out[d0, d1); the byte at d0 is
// useq[x0], the next one useq[x0 + 1] (forward) or useq[x0 - 1] complemented (rev).  A piece is the LAST m = len - (k - 1) bytes
// of its oriented string.
__device__ __forceinline__ bool fill_piece(const u64 *s_pre, const u64 *s_dst, const u64 *s_so, const u64 *s_m, const u32 *s_o, u32 i, u64 t0, u64 t1, u64 km1, u64 *d0, u64 *d1, u64 *x0, bool *rev)
{
	const u64 P = s_pre[i], m = s_m[i];
	const u64 a = ctg_max(P, t0), b = ctg_min(P + m, t1);
	if (b <= a) return false;
	const u64 ra = a - P, rb = b - P;
	*rev = (s_o[i] & 1u) != 0;
	*d0 = s_dst[i] + ra;
	*d1 = s_dst[i] + rb;
	*x0 = *rev ? s_so[i] + (m - 1 - ra) : s_so[i] + km1 + ra;
	return true;
}

// one block per tile of FILL_TILE piece bytes (D.pbytes of them over D.n_pc pieces)
__global__ __launch_bounds__(256) void k_fill_emit(FillDev D)
{
	__shared__ u64 s_pre[FILL_NB];
	__shared__ u64 s_dst[FILL_NB];
	__shared__ u64 s_so[FILL_NB];
	__shared__ u64 s_m[FILL_NB];
	__shared__ u32 s_o[FILL_NB];
	__shared__ u32 s_wpre[FILL_NB + 1];
	__shared__ u32 s_part[256];
	__shared__ u64 s_p0;
	const u32 tid = threadIdx.x;
	const u64 t0 = (u64)blockIdx.x * FILL_TILE, t1 = ctg_min(t0 + FILL_TILE, D.pbytes), km1 = (u64)(D.k - 1);
	if (tid == 0) {                                                // the tile's first piece: the last one that starts at or in front of t0
		u64 lo = 0, hi = D.n_pc;
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (D.pc_pre[mid] <= t0) lo = mid + 1; else hi = mid;
		}
		s_p0 = lo ? lo - 1 : 0;
	}
	__syncthreads();
	const bool wide = ((size_t)D.fseq & 15) == 0, wide_in = ((size_t)D.useq & 3) == 0;
	// a piece is at least one byte, so the tile ends within FILL_TILE + 1 pieces of its first one
	for (u64 p0 = s_p0; p0 < D.n_pc && p0 <= s_p0 + FILL_TILE; p0 += FILL_NB) {
		if (D.pc_pre[p0] >= t1) break;                               // (the same for every lane)
		for (u32 i = tid; i < FILL_NB; i += 256) {
			const u64 x = p0 + i;
			u64 so = 0, m = 0;
			u32 o = 0;
			if (x < D.n_pc) {
				o = D.pc_o[x];
				const u64 len = (u64)o < 2 * D.U ? fill_len(D, o >> 1, &so) : 0;
				m = len > km1 ? len - km1 : 0;
			}
			s_pre[i] = x < D.n_pc ? D.pc_pre[x] : D.pbytes;
			s_dst[i] = x < D.n_pc ? D.pc_dst[x] : 0;
			s_so[i] = so;
			s_m[i] = m;
			s_o[i] = o;
		}
		__syncthreads();
		u32 wn[4], sum = 0;                                          // the aligned 16-byte output words each of this lane's 4 pieces touches
#pragma unroll
		for (u32 j = 0; j < 4; j++) {
			u64 d0, d1, x0;
			bool rev;
			wn[j] = fill_piece(s_pre, s_dst, s_so, s_m, s_o, 4 * tid + j, t0, t1, km1, &d0, &d1, &x0, &rev) ? (u32)(((d1 + 15) >> 4) - (d0 >> 4)) : 0;
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
#pragma unroll
		for (u32 j = 0; j < 4; j++) { s_wpre[4 * tid + j] = run; run += wn[j]; }
		if (tid == 255) s_wpre[FILL_NB] = run;
		__syncthreads();
		const u32 total = s_wpre[FILL_NB];
		for (u32 w = tid; w < total; w += 256) {
			u32 lo = 0, hi = FILL_NB;                                  // the last piece with s_wpre[i] <= w: the one word w belongs to
			while (lo < hi) {
				const u32 mid = (lo + hi) >> 1;
				if (s_wpre[mid] <= w) lo = mid + 1; else hi = mid;
			}
			const u32 i = lo - 1;
			u64 d0, d1, x0;
			bool rev;
			if (!fill_piece(s_pre, s_dst, s_so, s_m, s_o, i, t0, t1, km1, &d0, &d1, &x0, &rev)) continue;
			const u64 A = ((d0 >> 4) + (w - s_wpre[i])) << 4;
			u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;
			u32 fullm = 0;
#pragma unroll
			for (u32 g = 0; g < 4; g++) {
				u32 v = 0;
				const u64 G = A + 4 * g;
				if (G >= d0 && G + 4 <= d1) {                            // four bytes of one unitig: [x, x + 4) forward, read backwards for rev
					fullm |= 1u << g;
					const u64 x = rev ? x0 - (G - d0) - 3 : x0 + (G - d0), y = x & ~3ULL;
					if (wide_in && y + 8 <= D.n_ubases) {
						const u64 two = (u64)*(const u32 *)(D.useq + y + 4) << 32 | *(const u32 *)(D.useq + y);
						v = (u32)(two >> (8 * (x & 3)));
					} else
						v = (u32)D.useq[x] | (u32)D.useq[x + 1] << 8 | (u32)D.useq[x + 2] << 16 | (u32)D.useq[x + 3] << 24;
					v = rev ? ctg_comp4(__builtin_bswap32(v)) : v;
				} else {
					for (u32 b = 0; b < 4; b++) {
						const u64 d = G + b;
						if (d >= d0 && d < d1) v |= (u32)D.useq[rev ? x0 - (d - d0) : x0 + (d - d0)] << (8 * b);
					}
					v = rev ? ctg_comp4(v) : v;
				}
				if (g == 0) w0 = v; else if (g == 1) w1 = v; else if (g == 2) w2 = v; else w3 = v;
			}
			if (wide && fullm == 15 && A + 16 <= D.seq_cap) {
				*(uint4 *)(D.fseq + A) = make_uint4(w0, w1, w2, w3);
				continue;
			}
#pragma unroll
			for (u32 g = 0; g < 4; g++) {
				const u32 v = g == 0 ? w0 : g == 1 ? w1 : g == 2 ? w2 : w3;
				const u64 G = A + 4 * g;
				if (wide && (fullm >> g & 1) && G + 4 <= D.seq_cap) { *(u32 *)(D.fseq + G) = v; continue; }
				for (u32 b = 0; b < 4; b++) {
					const u64 d = G + b;
					if (d >= d0 && d < d1 && d < D.seq_cap) D.fseq[d] = (unsigned char)(v >> (8 * b));
				}
			}
		}
		__syncthreads();
	}
}
