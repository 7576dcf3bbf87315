// correct_kernels.h -- kmx_correct_seqs: substitution errors of reads, corrected from the k-mer spectrum.
// Included at the end of kernels.hip (after count_kernels.h): it uses seq_tile_window / query_packed_one / astr_query_one
// and seq_off / seq_upper, so the windows, their answers and the sequence boundaries are those of kmx_query_seqs.
//
// The rule is in include/kmx.h; every decision is taken from the answers on the INPUT bases, so nothing here depends on
// the order of evaluation.  One piece = the windows [p0, p0 + n_win), in four launches on one stream:
//   k_correct_weak (+ k_correct_weak_ascii_at for the listed windows): one bit per window, answer < thr, for the piece and a
//     halo of KMX_CORR_HALO(k) windows on both sides (the halo is answered again by the neighbouring piece: 2 * (2k + 2)
//     windows per piece).  Bit d of `bits` is window w0 + d; a position where no window of a sequence starts holds 0.
//   k_correct_sites<W, false>: a lane per window of the piece looks at the bits around it, decides whether it is the first or
//     the last window of a run and which site that edge owns (at most one per lane), the workgroup keeps its sites in LDS and
//     its waves verify them, a wave per site and a lane per verification window.  Sites whose span holds another byte outside
//     ACGT are left to k_correct_sites<W, true>, which redoes the (cheap) edge pass of the workgroups that flagged one and
//     answers those windows through the byte-string body: an AStr per lane stays off the clean kernel's registers.
// No list grows with the input: the bits are one piece's, the sites never leave the workgroup.

static constexpr int CORR_RAW = SEQ_BT + 3 * 64;                   // bases a workgroup of k_correct_sites stages: k - 1 before its tile, 2k - 2 behind

// windows [w0, w0 + n_win): bits[(p - w0) / 64] bit (p - w0) % 64 = the window at p is valid, clean and answered < thr (the
// listed ones are OR-ed in by k_correct_weak_ascii_at).  Every word of the grid's tiles is written.  seq holds the bases
// [g0, g1) and the offsets are clamped to g1: a window of [w0, w0 + n_win) that fits in its sequence must fit below g1.
template <int W> __global__ __launch_bounds__(SEQ_BT) void k_correct_weak(ModelDev md, const unsigned char *seq, u64 g0, u64 g1, const u64 *offs, u64 n_seqs, u64 w0, u64 n_win, int thr, u64 *bits, u32 *dlist, u32 cap, u32 *dcnt)
{
	__shared__ unsigned char s_code[SEQ_TILE];
	__shared__ u64 s_u[2];
	const u64 t0 = w0 + (u64)blockIdx.x * SEQ_BT, p_end = w0 + n_win, p = t0 + threadIdx.x;
	u64 v[W];
	const SeqLane w = seq_tile_window<W>(md.k, seq, g0, g1, offs, n_seqs, t0, p_end, s_code, s_u, v);
	const bool dirty = w.valid && w.bad, act = w.valid && !w.bad;
	const u32 slot = wave_append_slot<u32>(dcnt, dirty);
	if (dirty && slot < cap) dlist[slot] = (u32)(p - w0);
	int ans = 0;
	if (act) query_packed_one<W, false>(md, v, nullptr, &ans);
	const u64 weak = __ballot(act && ans < thr);
	if ((threadIdx.x & 63) == 0) bits[(u64)blockIdx.x * (SEQ_BT / 64) + (threadIdx.x >> 6)] = weak;
}

template <int W> __global__ __launch_bounds__(256) void k_correct_weak_ascii_at(ModelDev md, StrGeom gf, StrGeom gb, const unsigned char *seq, u64 g0, u64 g1, u64 w0, u64 n_win, int thr, u64 *bits, const u32 *dlist, u32 cap, const u32 *dcnt, u32 *dcnt_next)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) *dcnt_next = 0;
	const u32 c = *dcnt, n = c < cap ? c : cap;
	const int L = md.k;
	for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
		const u64 d = dlist[i], p = w0 + d;
		if (d >= n_win || p < g0 || p + (u64)L > g1) continue;       // (never for a listed window)
		int ans = 0;
		astr_query_one<W>(md, gf, gb, L, astr_load(seq + (p - g0), L), &ans);
		if (ans < thr) atomicOr((unsigned long long *)bits + (d >> 6), 1ULL << (d & 63));
	}
}

// the weak bits of the windows [q0, q0 + 64) that lie in [lo, hi), bit j = window q0 + j; [lo, hi) is inside [w0, w0 + n_bits),
// the windows `bits` holds, so no word outside them is read
__device__ __forceinline__ u64 corr_bits(const u64 *bits, u64 w0, u64 lo, u64 hi, long long q0)
{
	const long long a = q0 < (long long)lo ? (long long)lo : q0, b = q0 + 64 > (long long)hi ? (long long)hi : q0 + 64;
	if (a >= b) return 0;
	const u64 d = (u64)a - w0, wi = d >> 6;
	const int sh = (int)(d & 63), n = (int)(b - a);
	u64 x = bits[wi] >> sh;
	if (sh && sh + n > 64) x |= bits[wi + 1] << (64 - sh);
	if (n < 64) x &= (1ULL << n) - 1;
	return x << (a - q0);
}
// the same after gap closing: a window between two weak ones counts as weak (both neighbours are windows of the sequence,
// so it is an inner one)
__device__ __forceinline__ u64 corr_closed(const u64 *bits, u64 w0, u64 lo, u64 hi, long long q0)
{
	return corr_bits(bits, w0, lo, hi, q0) | (corr_bits(bits, w0, lo, hi, q0 - 1) & corr_bits(bits, w0, lo, hi, q0 + 1));
}

// n_weak and n_runs of a wave's windows into the records: key = the lane's sequence (u, or ~0 for none), fw / fr = the
// ballots of the lanes that count.  The lanes of one key are one stretch of the wave; its first lane adds the stretch's
// counts.  Every lane of the wave calls it.
__device__ __forceinline__ void corr_fold_wave(SeqCorrection *rec, u64 key, u64 fw, u64 fr)
{
	const int lane = threadIdx.x & 63;
	const u64 prev = __shfl_up(key, 1, 64);
	const u64 heads = __ballot(lane == 0 || key != prev);
	if (!((heads >> lane) & 1) || key == ~0ULL) return;
	const u64 above = lane == 63 ? 0 : heads & (~0ULL << (lane + 1));
	const int e = above ? __ffsll((long long)above) - 2 : 63;
	const u64 seg = (~0ULL >> (63 - e)) & (~0ULL << lane);
	if (fw & seg) atomicAdd(&rec[key - 1].n_weak, (u64)__popcll(fw & seg));
	if (fr & seg) atomicAdd(&rec[key - 1].n_runs, (u64)__popcll(fr & seg));
}

__global__ __launch_bounds__(256) void k_seq_correction_init(SeqCorrection *rec, const u64 *offs, u64 n_seqs, u64 n_bases, int k)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_seqs) return;
	const u64 a = seq_off(offs, i, n_bases), b = seq_off(offs, i + 1, n_bases), len = b > a ? b - a : 0;
	rec[i] = SeqCorrection{len >= (u64)k ? len - (u64)k + 1 : 0, 0, 0, 0, 0, 0, 0, 0};
}

// The windows [p0, p0 + n_win) of the piece (positions of the offsets, which are clamped to n_total, the length of the whole
// input): seq holds the bases [g0, g1), bits the windows [w0, w0 + n_bits).  flags[blockIdx.x]: the clean kernel left a site
// to the DIRTY one.  n_weak and n_runs are counted by the clean kernel alone, the site counters by whichever verifies the site.
template <int W, bool DIRTY> __global__ __launch_bounds__(SEQ_BT) void k_correct_sites(ModelDev md, StrGeom gf, StrGeom gb, const unsigned char *seq, u64 g0, u64 g1, u64 n_total, const u64 *offs, u64 n_seqs, u64 p0, u64 n_win, u64 w0, u64 n_bits, const u64 *bits, CorrDev cd, unsigned char *flags)
{
	__shared__ unsigned char s_raw[CORR_RAW];
	__shared__ u64 s_u[2];
	__shared__ u64 s_b[SEQ_BT], s_v0[SEQ_BT], s_seq[SEQ_BT];
	__shared__ int s_nv[SEQ_BT];
	__shared__ int s_n, s_flag;
	if (DIRTY && !flags[blockIdx.x]) return;
	const int tid = threadIdx.x, lane = tid & 63, k = md.k;
	const u64 t0 = p0 + (u64)blockIdx.x * SEQ_BT, p_end = p0 + n_win, p = t0 + tid;
	const u64 t_last = (t0 + SEQ_BT < p_end ? t0 + SEQ_BT : p_end) - 1;
	const u64 r0 = t0 >= g0 + (u64)(k - 1) ? t0 - (u64)(k - 1) : g0;
	const u64 r1 = t0 + SEQ_BT + 2 * (u64)k - 2 < g1 ? t0 + SEQ_BT + 2 * (u64)k - 2 : g1;   // the bases staged: [r0, r1)
	if (tid == 0) { s_u[0] = seq_upper(offs, 0, n_seqs + 1, t0, n_total); s_n = 0; s_flag = 0; }
	if (tid == 64) s_u[1] = seq_upper(offs, 0, n_seqs + 1, t_last, n_total);
	for (u64 j = r0 + tid; j < r1; j += SEQ_BT) s_raw[j - r0] = seq[j - g0];
	__syncthreads();

	// ---- the lane's window: its sequence, the bits around it, the site its edge owns
	u64 key = ~0ULL;
	bool weak = false, first = false, tried = false;
	u64 b = 0, v0 = 0, v1 = 0;
	if (p < p_end) {
		const u64 u0 = s_u[0], u1 = s_u[1];
		const u64 u = seq_upper(offs, u0, u1 > u0 ? u1 : u0, p, n_total);
		if (u >= 1 && u <= n_seqs) {
			const u64 start = seq_off(offs, u - 1, n_total), end = seq_off(offs, u, n_total);
			const u64 len = end > start ? end - start : 0, nw = len >= (u64)k ? len - (u64)k + 1 : 0;
			if (start <= p && p < start + nw) {
				key = u;
				const u64 lo = start > w0 ? start : w0, hi = start + nw < w0 + n_bits ? start + nw : w0 + n_bits;
				const u64 x = corr_bits(bits, w0, lo, hi, (long long)p - 2);   // bit j: window p - 2 + j
				const bool c_prev = ((x >> 1) & 1) || ((x & 1) && ((x >> 2) & 1));
				const bool c_here = ((x >> 2) & 1) || (((x >> 1) & 1) && ((x >> 3) & 1));
				const bool c_next = ((x >> 3) & 1) || (((x >> 2) & 1) && ((x >> 4) & 1));
				weak = (x >> 2) & 1;
				first = c_here && !c_prev;
				const bool last = c_here && !c_next;
				const u64 w_last = start + nw - 1;
				bool has = false;
				if (first && p > start) {                                    // the run's first window, s = p; hasL
					u64 c = ~corr_closed(bits, w0, lo, hi, (long long)p + 1);
					int run = c ? __ffsll((long long)c) - 1 : 64;            // closed windows behind p, up to 128
					if (run == 64) { c = ~corr_closed(bits, w0, lo, hi, (long long)p + 65); run += c ? __ffsll((long long)c) - 1 : 64; }
					const u64 e = p + (u64)run;
					if (run >= 2 * k - 1 || e == w_last) { has = true; b = p + k - 1; v0 = p; v1 = e < b ? e : b; }   // a long run, or hasL only
					else if (run + 1 == k) { has = true; b = e; v0 = p; v1 = e; }
					else if (run + 1 > k) { has = true; b = p + k - 1; v0 = p; v1 = b < e - k ? b : e - k; }
				}
				if (last && p < w_last && !has) {                            // the run's last window, e = p; hasR
					u64 c = ~corr_closed(bits, w0, lo, hi, (long long)p - 64);
					int run = c ? __clzll((long long)c) : 64;                // closed windows before p, up to 128
					if (run == 64) { c = ~corr_closed(bits, w0, lo, hi, (long long)p - 128); run += c ? __clzll((long long)c) : 64; }
					const u64 s = p - (u64)run;
					if (run >= 2 * k - 1) { has = true; b = p; v0 = p - (k - 1); v1 = p; }
					else if (s == start) { has = true; b = p; v0 = s + (k - 1) > p ? s : p - (k - 1); v1 = p; }        // hasR only
					else if (run + 1 > k) { has = true; b = p; v0 = p - (k - 1) > s + k ? p - (k - 1) : s + k; v1 = p; }
				}
				// (the span's bases are staged: they lie within k - 1 before and 2k - 2 behind the lane, inside its sequence)
				tried = has && v1 >= v0 && v1 - v0 + 1 >= (u64)cd.min_support && v0 >= r0 && v1 + (u64)k <= r1;
			}
		}
	}
	if (!DIRTY && cd.rec) corr_fold_wave(cd.rec, key, __ballot(weak), __ballot(first));
	if (tried) {
		const int i = atomicAdd(&s_n, 1);
		s_b[i] = b; s_v0[i] = v0; s_seq[i] = key - 1; s_nv[i] = (int)(v1 - v0 + 1);
	}
	__syncthreads();

	// ---- a wave per site, a lane per verification window
	const int n_sites = s_n;
	for (int i = tid >> 6; i < n_sites; i += SEQ_BT / 64) {
		const u64 sb = s_b[i], sv0 = s_v0[i];
		const int nv = s_nv[i];
		const bool mine = lane < nv;
		const u64 wp = sv0 + (u64)lane;                                // the lane's window
		const int jb = (int)(sb - wp);                                  // where base b sits in it (0 .. k - 1 for a lane of V)
		const u32 orig = s_raw[sb - r0];
		u64 v[W];
		bool bad = false;
		if (mine) {
			u64 hi = 0, lo = 0;
			u32 any = 0;
			for (int j = 0; j < k; j++) {
				const u32 c = j == jb ? 0u : seq_code(s_raw[wp - r0 + j]);
				any |= c;
				if (W == 2) hi = (hi << 2) | (lo >> 62);
				lo = (lo << 2) | (c & 3u);
			}
			bad = (any & 4u) != 0;
			v[W - 1] = lo;
			if (W == 2) v[0] = hi;
		}
		const bool site_dirty = __ballot(mine && bad) != 0;
		if (site_dirty != DIRTY) {
			if (!DIRTY && lane == 0) s_flag = 1;
			continue;
		}
		const int sh = 2 * (k - 1 - jb);                                // the bit of base b in the packed window
		int n_pass = 0;
		u32 which = 0;
		for (u32 ci = 0; ci < 4 && n_pass < 2; ci++) {
			const u32 cb = (u32)"ACGT"[ci];
			if (cb == orig) continue;
			int ans = 0;
			if (mine) {
				if (DIRTY && bad) {
					AStr s = astr_load(s_raw + (wp - r0), k);
					astr_set(s, jb, cb);
					astr_query_one<W>(md, gf, gb, k, s, &ans);
				} else {
					u64 q[W];
#pragma unroll
					for (int j = 0; j < W; j++) q[j] = v[j];
					if (W == 2 && sh >= 64) q[0] |= (u64)ci << (sh - 64);
					else q[W - 1] |= (u64)ci << (sh & 63);
					query_packed_one<W, false>(md, q, nullptr, &ans);
				}
			}
			if (!__ballot(mine && ans < cd.thr)) { n_pass++; which = ci; }
		}
		if (lane != 0) continue;
		if (cd.rec) {
			SeqCorrection *r = cd.rec + s_seq[i];
			atomicAdd(&r->n_sites, 1ULL);
			atomicAdd(n_pass == 1 ? &r->n_corrected : (n_pass ? &r->n_ambiguous : &r->n_unfixable), 1ULL);
		}
		if (n_pass != 1) continue;
		if (cd.out) cd.out[sb] = (unsigned char)"ACGT"[which];
		if (cd.fix) {
			const u32 slot = atomicAdd(cd.fix, 1u);
			if (slot < cd.fix_cap) cd.fix[2 + slot] = ((u32)(sb - p0) << 2) | which;
		}
	}
	if (!DIRTY) {
		__syncthreads();
		if (tid == 0) flags[blockIdx.x] = (unsigned char)s_flag;
	}
}

namespace kmxk {

void seq_correction_init(SeqCorrection *rec, const u64 *offs, u64 n_seqs, u64 n_bases, int k, hipStream_t st, KernelProf *prof)
{
	if (!n_seqs || !rec) return;
	KPROF_BEGIN(prof, KC_QUERY, st);
	hipLaunchKernelGGL(k_seq_correction_init, dim3((unsigned)((n_seqs + 255) / 256)), dim3(256), 0, st, rec, offs, n_seqs, n_bases, k);
	KPROF_END(prof, st);
}

// one piece: the windows [p0, p0 + n_win) of the input v views.  bits: room for the windows [w0, w1) in whole tiles of SEQ_BT,
// where [w0, w1) = the piece and KMX_CORR_HALO(k) windows on both sides, cut to [0, n_total) and to the windows whose bases
// are on hand; d (kmx_types.h) has room for w1 - w0 entries; flags: one byte per SEQ_BT windows of the piece.
void correct_piece(const ModelDev &md, const SeqView &v, u64 p0, u64 n_win, u64 w0, u64 w1, u64 *bits, const CorrDev &cd, unsigned char *flags, const SeqDirty &d, hipStream_t st, KernelProf *prof)
{
	const unsigned char *seq = v.seq;
	const u64 g0 = v.g0, g1 = v.g1, n_total = v.n_total, *offs = v.offs, n_seqs = v.n_seqs;
	u32 *dlist = d.list, cap = d.cap, *dcnt = d.cnt, *dcnt_next = d.cnt_next;
	if (!n_win) return;
	KPROF_BEGIN(prof, KC_QUERY, st);
	const StrGeom gf = make_geom(md.k), gb = make_geom(md.k - 2);
	const unsigned gw = (unsigned)((w1 - w0 + SEQ_BT - 1) / SEQ_BT), gs = (unsigned)((n_win + SEQ_BT - 1) / SEQ_BT);
	DISPATCH_W(words(md), hipLaunchKernelGGL(k_correct_weak<W>, dim3(gw), dim3(SEQ_BT), 0, st, md, seq, g0, g1, offs, n_seqs, w0, w1 - w0, cd.thr, bits, dlist, cap, dcnt));
	DISPATCH_W(words(md), hipLaunchKernelGGL(k_correct_weak_ascii_at<W>, dim3(SEQ_DIRTY_WGS), dim3(256), 0, st, md, gf, gb, seq, g0, g1, w0, w1 - w0, cd.thr, bits, (const u32 *)dlist, cap, (const u32 *)dcnt, dcnt_next));
	DISPATCH_W(words(md), hipLaunchKernelGGL((k_correct_sites<W, false>), dim3(gs), dim3(SEQ_BT), 0, st, md, gf, gb, seq, g0, g1, n_total, offs, n_seqs, p0, n_win, w0, w1 - w0, (const u64 *)bits, cd, flags));
	DISPATCH_W(words(md), hipLaunchKernelGGL((k_correct_sites<W, true>), dim3(gs), dim3(SEQ_BT), 0, st, md, gf, gb, seq, g0, g1, n_total, offs, n_seqs, p0, n_win, w0, w1 - w0, (const u64 *)bits, cd, flags));
	KPROF_END(prof, st);
}

}   // namespace kmxk
