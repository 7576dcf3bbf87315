// edit_kernels.h -- kmx_edit_seqs: substitutions and single-base insertions / deletions of reads, found from the k-mer spectrum.
// Included at the end of kernels.hip (after correct_kernels.h): k_correct_weak / k_correct_weak_ascii_at, corr_bits /
// corr_closed, seq_upper / seq_off and the two query bodies are used as they are.
//
// The rule is in include/kmx.h.  Unlike kmx_correct_seqs' table, it is not local: a run that touches one end of its sequence
// takes all three kinds of candidates however long it is, so the window at one edge of a run has to know where the other edge
// lies.  The weak bits are therefore kept for the whole input (one bit per window, written piece by piece by k_correct_weak
// into one array) before the first site is decided, and the edge lanes scan that array as far as the run reaches.
//   k_edit_sites<W, false>: a lane per window of the piece; the run's first window owns a left-anchored site (hasL only, or
//     the left substitution site of a run longer than k), its last window a right-anchored or interior one.  The workgroup keeps
//     its sites in LDS and its waves verify them, a wave per site, a lane per verification window, the candidates one after
//     another (up to 8 at a read end, up to 5 inside) until a second one has passed.
//   k_edit_sites<W, true>: the sites whose span holds a byte outside ACGT, through the byte-string body (as k_correct_sites).

enum { EDIT_F_SUB = 1, EDIT_F_DEL = 2, EDIT_F_INS4 = 4, EDIT_F_INS1 = 8, EDIT_F_JNEXT = 16 };   // a site's candidates; JNEXT: junction = anchor + 1

__global__ __launch_bounds__(256) void k_seq_edits_init(SeqEdits *rec, const u64 *offs, u64 n_seqs, u64 n_bases, int k)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_seqs) return;
	const u64 a = seq_off(offs, i, n_bases), b = seq_off(offs, i + 1, n_bases), len = b > a ? b - a : 0;
	rec[i] = SeqEdits{len >= (u64)k ? len - (u64)k + 1 : 0, 0, 0, 0, 0, 0, 0, 0, 0, len};
}

// corr_fold_wave for the 80-byte records
__device__ __forceinline__ void edit_fold_wave(SeqEdits *rec, u64 key, u64 fw, u64 fr)
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

// where byte j of an edited window comes from: x[j] with the byte at jb replaced (SUB), x without the byte at jb (DEL), x with
// a byte placed before the one at jb (INS).  For SUB and INS position jb of the window is the candidate's base.
__device__ __forceinline__ u32 edit_base(u32 ci) { return (0x54474341u >> (8 * ci)) & 0xFFu; }   // "ACGT"[ci]
__device__ __forceinline__ int edit_src(int op, int jb, int j) { return op == 1 ? j : (op == 2 ? j + (j >= jb) : j - (j > jb)); }

// the lane's window packed, the candidate's position left 0; returns whether another byte of it is outside ACGT
template <int W> __device__ __forceinline__ bool edit_pack(const unsigned char *x, int k, int op, int jb, u64 *v)
{
	u64 hi = 0, lo = 0;
	u32 any = 0;
	for (int j = 0; j < k; j++) {
		const u32 c = (op != 2 && j == jb) ? 0u : seq_code(x[edit_src(op, jb, j)]);
		any |= c;
		if (W == 2) hi = (hi << 2) | (lo >> 62);
		lo = (lo << 2) | (c & 3u);
	}
	v[W - 1] = lo;
	if (W == 2) v[0] = hi;
	return (any & 4u) != 0;
}

__device__ __forceinline__ AStr edit_astr(const unsigned char *x, int k, int op, int jb, u32 cb)
{
	AStr s;
#pragma unroll
	for (int w = 0; w < 8; w++) {
		u64 word = 0;
#pragma unroll
		for (int j = 0; j < 8; j++)
			if (8 * w + j < k) word |= (u64)x[edit_src(op, jb, 8 * w + j)] << (8 * j);
		s.b[w] = word;
	}
	if (op != 2) astr_set(s, jb, cb);
	return s;
}

// one candidate: every lane of the wave calls it; true iff every window of V answers >= thr
template <int W, bool DIRTY> __device__ __forceinline__ bool edit_try(const ModelDev &md, const StrGeom gf, const StrGeom gb, int thr, const unsigned char *x, int op, int jb, u32 ci, bool mine, bool bad, const u64 *v)
{
	const int k = md.k;
	int ans = 0;
	if (mine) {
		if (DIRTY && bad) astr_query_one<W>(md, gf, gb, k, edit_astr(x, k, op, jb, edit_base(ci)), &ans);
		else {
			u64 q[W];
#pragma unroll
			for (int j = 0; j < W; j++) q[j] = v[j];
			if (op != 2) {
				const int sh = 2 * (k - 1 - jb);
				if (W == 2 && sh >= 64) q[0] |= (u64)ci << (sh - 64);
				else q[W - 1] |= (u64)ci << (sh & 63);
			}
			query_packed_one<W, false>(md, q, nullptr, &ans);
		}
	}
	return !__ballot(mine && ans < thr);
}

// The windows [p0, p0 + n_win) of the piece; seq holds the whole input [0, n_total), bits the weak bits of all its windows
// (bit p of the array = window p).  flags[blockIdx.x]: the clean kernel left a site to the DIRTY one.
template <int W, bool DIRTY> __global__ __launch_bounds__(SEQ_BT) void k_edit_sites(ModelDev md, StrGeom gf, StrGeom gb, const unsigned char *seq, u64 n_total, const u64 *offs, u64 n_seqs, u64 p0, u64 n_win, const u64 *bits, EditDev ed, unsigned char *flags)
{
	__shared__ unsigned char s_raw[CORR_RAW];
	__shared__ u64 s_u[2];
	__shared__ u64 s_a[SEQ_BT], s_v0[SEQ_BT], s_seq[SEQ_BT], s_start[SEQ_BT], s_end[SEQ_BT];
	__shared__ int s_nv[SEQ_BT], s_fl[SEQ_BT];
	__shared__ int s_n, s_flag;
	if (DIRTY && !flags[blockIdx.x]) return;
	const int tid = threadIdx.x, lane = tid & 63, k = md.k;
	const u64 t0 = p0 + (u64)blockIdx.x * SEQ_BT, p_end = p0 + n_win, p = t0 + tid;
	const u64 t_last = (t0 + SEQ_BT < p_end ? t0 + SEQ_BT : p_end) - 1;
	const u64 r0 = t0 >= (u64)(k - 1) ? t0 - (u64)(k - 1) : 0;
	const u64 r1 = t0 + SEQ_BT + 2 * (u64)k - 2 < n_total ? t0 + SEQ_BT + 2 * (u64)k - 2 : n_total;   // the bases staged: [r0, r1)
	if (tid == 0) { s_u[0] = seq_upper(offs, 0, n_seqs + 1, t0, n_total); s_n = 0; s_flag = 0; }
	if (tid == 64) s_u[1] = seq_upper(offs, 0, n_seqs + 1, t_last, n_total);
	for (u64 j = r0 + tid; j < r1; j += SEQ_BT) s_raw[j - r0] = seq[j];
	__syncthreads();

	// ---- the lane's window: its sequence, the bits around it, the site its edge owns
	u64 key = ~0ULL;
	bool weak = false, first = false;
	int fl = 0, nv = 0;
	u64 A = 0, v0 = 0, start = 0, end = 0;
	if (p < p_end) {
		const u64 u0 = s_u[0], u1 = s_u[1];
		const u64 u = seq_upper(offs, u0, u1 > u0 ? u1 : u0, p, n_total);
		if (u >= 1 && u <= n_seqs) {
			start = seq_off(offs, u - 1, n_total);
			end = seq_off(offs, u, n_total);
			const u64 len = end > start ? end - start : 0, nw = len >= (u64)k ? len - (u64)k + 1 : 0;
			if (start <= p && p < start + nw) {
				key = u;
				const u64 lo = start, hi = start + nw, w_last = hi - 1;
				const u64 x = corr_bits(bits, 0, lo, hi, (long long)p - 2);   // bit j: window p - 2 + j
				const bool c_prev = ((x >> 1) & 1) || ((x & 1) && ((x >> 2) & 1));
				const bool c_here = ((x >> 2) & 1) || (((x >> 1) & 1) && ((x >> 3) & 1));
				const bool c_next = ((x >> 3) & 1) || (((x >> 2) & 1) && ((x >> 4) & 1));
				weak = (x >> 2) & 1;
				first = c_here && !c_prev;
				const bool last = c_here && !c_next;
				u64 v1 = 0;
				if (first && p > start) {                                    // the run's first window, s = p; hasL
					u64 e = p;
					for (;;) {                                               // closed windows behind p, as far as they go
						const u64 c = ~corr_closed(bits, 0, lo, hi, (long long)e + 1);
						const int n = c ? __ffsll((long long)c) - 1 : 64;
						e += (u64)n;
						if (n < 64) break;
					}
					A = p + (u64)(k - 1);
					if (e == w_last) { fl = EDIT_F_SUB | EDIT_F_DEL | EDIT_F_INS4; v0 = p; v1 = e < A ? e : A; }        // hasL only
					else if (e - p + 1 > (u64)k) { fl = EDIT_F_SUB; v0 = p; v1 = A < e - k ? A : e - k; }
				}
				if (last && p < w_last && !fl) {                             // the run's last window, e = p; hasR
					u64 s = p;
					for (;;) {                                               // closed windows before p
						const u64 c = ~corr_closed(bits, 0, lo, hi, (long long)s - 64);
						const int n = c ? __clzll((long long)c) : 64;
						s -= (u64)n;
						if (n < 64) break;
					}
					const u64 rl = p - s + 1;
					A = p;
					v1 = p;
					if (s == start) { fl = EDIT_F_SUB | EDIT_F_DEL | EDIT_F_INS4 | EDIT_F_JNEXT; v0 = s + (u64)(k - 1) > p ? s : p - (u64)(k - 1); }   // hasR only
					else if (rl > (u64)k) { fl = EDIT_F_SUB; v0 = p - (u64)(k - 1) > s + k ? p - (u64)(k - 1) : s + k; }
					else if (p + (u64)k <= r1 && s >= r0) {                  // inside, len <= k: the core is x[e .. s + k - 1] (always staged)
						const int h = k - (int)rl + 1;
						const unsigned char *core = s_raw + (p - r0);
						fl = EDIT_F_JNEXT;
						if (h == 1) { fl |= EDIT_F_SUB; v0 = s; }
						bool eq = true;
						for (int j = 1; j < h; j++) eq = eq && core[j] == core[0];
						if (eq) fl |= EDIT_F_DEL;
						if (h == 2) fl |= EDIT_F_INS4;
						else if (h >= 3) {
							bool same = seq_code(core[1]) < 4u;
							for (int j = 2; j < h - 1; j++) same = same && core[j] == core[1];
							if (same) fl |= EDIT_F_INS1;
						}
					}
				}
				// which kinds are asked for and tried; their windows lie within k - 1 before and 2k - 2 behind the lane, inside
				// its sequence, so they are staged
				if (fl) {
					const long long L = (long long)len, a = (long long)(A - start), j = a + ((fl & EDIT_F_JNEXT) ? 1 : 0);
					const long long dlo = a - k + 1 > 0 ? a - k + 1 : 0, dhi = a - 1 < L - 1 - k ? a - 1 : L - 1 - k;
					const long long ilo = j - k + 1 > 0 ? j - k + 1 : 0, ihi = j < L + 1 - k ? j : L + 1 - k;
					nv = (fl & EDIT_F_SUB) ? (int)(v1 - v0 + 1) : 0;
					if (!(ed.ops & 1) || nv < ed.min_support) fl &= ~EDIT_F_SUB;
					if (!(ed.ops & 2) || dhi - dlo + 1 < ed.min_support) fl &= ~EDIT_F_DEL;
					if (!(ed.ops & 4) || ihi - ilo + 1 < ed.min_support) fl &= ~(EDIT_F_INS4 | EDIT_F_INS1);
					if (!(fl & (EDIT_F_SUB | EDIT_F_DEL | EDIT_F_INS4 | EDIT_F_INS1))) fl = 0;
					const u64 b0 = p >= start + (u64)(k - 1) ? p - (u64)(k - 1) : start, b1 = p + 2 * (u64)k - 1 < end ? p + 2 * (u64)k - 1 : end;
					if (b0 < r0 || b1 > r1) fl = 0;                          // (never: the staged span covers it)
				}
			}
		}
	}
	if (!DIRTY && ed.rec) edit_fold_wave(ed.rec, key, __ballot(weak), __ballot(first));
	if (fl) {
		const int i = atomicAdd(&s_n, 1);
		s_a[i] = A; s_v0[i] = v0; s_seq[i] = key - 1; s_start[i] = start; s_end[i] = end; s_nv[i] = nv; s_fl[i] = fl;
	}
	__syncthreads();

	// ---- a wave per site, a lane per verification window, the candidates in the rule's order
	const int n_sites = s_n;
	for (int i = tid >> 6; i < n_sites; i += SEQ_BT / 64) {
		const u64 sa = s_a[i], st = s_start[i];
		const int f = s_fl[i], nvs = (f & EDIT_F_SUB) ? s_nv[i] : 0;
		const long long L = (long long)(s_end[i] - st), a = (long long)(sa - st), jj = a + ((f & EDIT_F_JNEXT) ? 1 : 0);
		const long long dlo = a - k + 1 > 0 ? a - k + 1 : 0, dhi = a - 1 < L - 1 - k ? a - 1 : L - 1 - k;
		const long long ilo = jj - k + 1 > 0 ? jj - k + 1 : 0, ihi = jj < L + 1 - k ? jj : L + 1 - k;
		const int nvd = (f & EDIT_F_DEL) ? (int)(dhi - dlo + 1) : 0, nvi = (f & (EDIT_F_INS4 | EDIT_F_INS1)) ? (int)(ihi - ilo + 1) : 0;
		const u64 sj = st + (u64)jj;
		// the bytes any of its windows reads; the anchor itself only when an insertion keeps it
		u64 lo = ~0ULL, hi = 0;
		if (nvs) { lo = s_v0[i]; hi = s_v0[i] + (u64)(nvs - 1 + k); }
		if (nvd) { lo = st + (u64)dlo < lo ? st + (u64)dlo : lo; hi = st + (u64)(dhi + k + 1) > hi ? st + (u64)(dhi + k + 1) : hi; }
		if (nvi) { lo = st + (u64)ilo < lo ? st + (u64)ilo : lo; hi = st + (u64)(ihi + k - 1) > hi ? st + (u64)(ihi + k - 1) : hi; }
		bool off_acgt = false;
		for (u64 q = lo + (u64)lane; q < hi; q += 64) off_acgt = off_acgt || (seq_code(s_raw[q - r0]) > 3u && (nvi || q != sa));
		const bool site_dirty = __ballot(off_acgt) != 0;
		if (site_dirty != DIRTY) {
			if (!DIRTY && lane == 0) s_flag = 1;
			continue;
		}
		// candidate c: 0 .. 3 SUB of "ACGT"[c], 4 DEL, 5 .. 8 INS of "ACGT"[c - 5]; a kind's windows are packed when its first
		// candidate comes up (one loop, so that each query body is inlined once)
		int n_pass = 0, cur = 0, jb = 0;
		u32 won = 0;                                                   // op << 4 | code of the candidate that passed
		u64 v[W];
		bool mine = false, bad = false;
		const unsigned char *x = s_raw;
		const u32 orig = s_raw[sa - r0], only = s_raw[sj - r0];
		for (int c = 0; c < 9 && n_pass < 2; c++) {
			const int op = c < 4 ? 1 : (c == 4 ? 2 : 3);
			const u32 ci = op == 1 ? (u32)c : (op == 2 ? 0u : (u32)(c - 5));
			const int nvk = op == 1 ? nvs : (op == 2 ? nvd : nvi);
			if (!nvk) continue;
			if (op == 1 && edit_base(ci) == orig) continue;
			if (op == 3 && (f & EDIT_F_INS1) && edit_base(ci) != only) continue;
			if (op != cur) {
				cur = op;
				mine = lane < nvk;
				const u64 wp = (op == 1 ? s_v0[i] : st + (u64)(op == 2 ? dlo : ilo)) + (mine ? (u64)lane : 0);
				jb = (int)((op == 3 ? sj : sa) - wp);
				x = s_raw + (wp - r0);
				bad = edit_pack<W>(x, k, op, jb, v);
			}
			if (edit_try<W, DIRTY>(md, gf, gb, ed.thr, x, op, jb, ci, mine, bad, v)) { n_pass++; won = (u32)op << 4 | ci; }
		}
		if (lane != 0) continue;
		const u32 op = won >> 4;
		if (ed.rec) {
			SeqEdits *r = ed.rec + s_seq[i];
			atomicAdd(&r->n_sites, 1ULL);
			atomicAdd(n_pass == 1 ? (op == 1 ? &r->n_sub : (op == 2 ? &r->n_del : &r->n_ins)) : (n_pass ? &r->n_ambiguous : &r->n_unfixable), 1ULL);
			if (n_pass == 1 && op != 1) atomicAdd(&r->out_len, op == 3 ? 1ULL : ~0ULL);
		}
		if (n_pass != 1) continue;
		const u64 slot = atomicAdd(ed.count, 1ULL);
		if (slot < ed.cap) ed.edits[slot] = (op == 3 ? sj : sa) << 8 | won;
	}
	if (!DIRTY) {
		__syncthreads();
		if (tid == 0) flags[blockIdx.x] = (unsigned char)s_flag;
	}
}

namespace kmxk {

void seq_edits_init(SeqEdits *rec, const u64 *offs, u64 n_seqs, u64 n_bases, int k, hipStream_t st, KernelProf *prof)
{
	if (!n_seqs || !rec) return;
	KPROF_BEGIN(prof, KC_QUERY, st);
	hipLaunchKernelGGL(k_seq_edits_init, dim3((unsigned)((n_seqs + 255) / 256)), dim3(256), 0, st, rec, offs, n_seqs, n_bases, k);
	KPROF_END(prof, st);
}

// the weak bits of the windows [w0, w0 + n_win) of the input v holds whole, w0 a multiple of SEQ_BT: whole words of bits
// (bit p = window p) are written, up to the end of the piece's last tile.  d (kmx_types.h) has room for n_win entries.
void edit_weak_piece(const ModelDev &md, const SeqView &v, u64 w0, u64 n_win, int thr, u64 *bits, const SeqDirty &d, hipStream_t st, KernelProf *prof)
{
	const unsigned char *seq = v.seq;
	const u64 *offs = v.offs, n_seqs = v.n_seqs;
	u32 *dlist = d.list, cap = d.cap, *dcnt = d.cnt, *dcnt_next = d.cnt_next;
	if (!n_win) return;
	KPROF_BEGIN(prof, KC_QUERY, st);
	const StrGeom gf = make_geom(md.k), gb = make_geom(md.k - 2);
	const unsigned gw = (unsigned)((n_win + SEQ_BT - 1) / SEQ_BT);
	u64 *b = bits + w0 / 64;
	DISPATCH_W(words(md), hipLaunchKernelGGL(k_correct_weak<W>, dim3(gw), dim3(SEQ_BT), 0, st, md, seq, v.g0, v.g1, offs, n_seqs, w0, n_win, thr, b, dlist, cap, dcnt));
	DISPATCH_W(words(md), hipLaunchKernelGGL(k_correct_weak_ascii_at<W>, dim3(SEQ_DIRTY_WGS), dim3(256), 0, st, md, gf, gb, seq, v.g0, v.g1, w0, n_win, thr, b, (const u32 *)dlist, cap, (const u32 *)dcnt, dcnt_next));
	KPROF_END(prof, st);
}

// the sites of the windows [p0, p0 + n_win), once the bits of the whole input are written; flags: one byte per SEQ_BT windows
void edit_sites_piece(const ModelDev &md, const SeqView &v, u64 p0, u64 n_win, const u64 *bits, const EditDev &ed, unsigned char *flags, hipStream_t st, KernelProf *prof)
{
	const unsigned char *seq = v.seq;
	const u64 n_total = v.n_total, *offs = v.offs, n_seqs = v.n_seqs;
	if (!n_win) return;
	KPROF_BEGIN(prof, KC_QUERY, st);
	const StrGeom gf = make_geom(md.k), gb = make_geom(md.k - 2);
	const unsigned gs = (unsigned)((n_win + SEQ_BT - 1) / SEQ_BT);
	DISPATCH_W(words(md), hipLaunchKernelGGL((k_edit_sites<W, false>), dim3(gs), dim3(SEQ_BT), 0, st, md, gf, gb, seq, n_total, offs, n_seqs, p0, n_win, bits, ed, flags));
	DISPATCH_W(words(md), hipLaunchKernelGGL((k_edit_sites<W, true>), dim3(gs), dim3(SEQ_BT), 0, st, md, gf, gb, seq, n_total, offs, n_seqs, p0, n_win, bits, ed, flags));
	KPROF_END(prof, st);
}

}   // namespace kmxk
