// extend_kernels.h -- kmx_extend_seqs: seeds extended to the right along unique k-mer paths of the model's de Bruijn graph.
// Included at the end of kernels.hip (after correct_kernels.h): it uses query_packed_one, seq_off / seq_code and
// wave_append_slot.  Every k-mer a walk asks about is uppercase ACGT, so every answer is that of the packed body.
//
// The rule is in include/kmx.h.  A walk is a dependent chain: step t + 1 asks about the k-mer step t chose.  What one step
// asks does not depend on its own choice, though: the four successors cur[1:] + c and the four predecessors d + cur[1:] of
// whichever of them is chosen are known from cur.  So a group of 8 lanes owns a walk (lanes 0-3: the successors, lanes 4-7:
// the predecessors), a wave holds 8 walks and one ballot per step gives every group its sets S and P as a byte.  A tie goes
// to the lookahead:
// each half of the group keeps the frontier of its direction as a 64-bit mask (level l: nodes of l + 1 bases, at most 4, 16,
// 64), takes one surviving node per pass and asks its four children; the last level keeps only "some child is solid".
//
//   k_extend_init: a lane per seed packs its last k bytes, asks seed_occ, writes the walk's state and lists it as live.
//   k_extend_step: at most `steps` steps of every live walk; a walk that stops writes its record, one that does not goes to
//     the next launch's list, so finished walks stop occupying lanes and no launch runs longer than `steps` steps.
// The lists alternate between two buffers and three counters: a launch reads one counter, appends under the next and
// zeroes the third for the launch after it, so the host neither waits nor clears anything between launches.

static constexpr int EXT_GROUP = 8, EXT_BT = 256, EXT_WALKS = EXT_BT / EXT_GROUP;

// a node of the step at cur, `nd` bases (1 ... 4) deep: forward, cur[nd:] + the digits of dig (first appended base most
// significant); backward, the digits of dig in reverse (the base prepended last comes first) + cur[1 : k - nd + 1] -- the
// first backward digit REPLACES cur[0]: d + cur[1:] is a predecessor of the k-mer the walk would move to
template <int W> __device__ __forceinline__ void ext_node(const u64 *cur, int k, bool back, u32 dig, int nd, u64 *q)
{
	const int s = 2 * nd;
	if (!back) {
		if (W == 1) q[0] = ((cur[0] << s) | dig) & (k == 32 ? ~0ULL : (1ULL << (2 * k)) - 1);
		else {
			q[0] = ((cur[0] << s) | (cur[W - 1] >> (64 - s))) & (k == 64 ? ~0ULL : (1ULL << (2 * k - 64)) - 1);
			q[W - 1] = (cur[W - 1] << s) | dig;
		}
		return;
	}
	u64 r = 0;
	for (int i = 0; i < nd; i++) { r = (r << 2) | (dig & 3u); dig >>= 2; }
	const int pos = 2 * k - s, sh = s - 2;                          // (k >= 4 >= nd)
	if (W == 1) q[0] = ((cur[0] & ((1ULL << (2 * (k - 1))) - 1)) >> sh) | (r << pos);
	else {
		const u64 t = cur[0] & ((1ULL << (2 * (k - 1) - 64)) - 1);  // cur[1:], whose last nd - 1 bases go
		u64 lo = sh ? (cur[W - 1] >> sh) | (t << (64 - sh)) : cur[W - 1], hi = t >> sh;
		if (pos >= 64) hi |= r << (pos - 64);
		else { lo |= r << pos; hi |= r >> (64 - pos); }             // (k >= 33: 58 <= pos < 64)
		q[0] = hi;
		q[W - 1] = lo;
	}
}

// seeds [0, n) of the chunk: seq holds n_bases bases, offs the chunk's n + 1 offsets (clamped to n_bases where they are read)
template <int W> __global__ __launch_bounds__(256) void k_extend_init(ModelDev md, const unsigned char *seq, u64 n_bases, const u64 *offs, u32 n, ExtDev xd, u32 *live, u32 *cnt)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	const int k = md.k;
	bool ok = false;
	u64 v[W];
#pragma unroll
	for (int j = 0; j < W; j++) v[j] = 0;
	if (i < n) {
		const u64 a = seq_off(offs, i, n_bases), b = seq_off(offs, (u64)i + 1, n_bases);
		if (b >= a && b - a >= (u64)k) {
			u64 hi = 0, lo = 0;
			u32 any = 0;
			for (int j = 0; j < k; j++) {
				const u32 c = seq_code(seq[b - (u64)k + j]);
				any |= c;
				if (W == 2) hi = (hi << 2) | (lo >> 62);
				lo = (lo << 2) | (c & 3u);
			}
			ok = !(any & 4u);
			v[W - 1] = lo;
			if (W == 2) v[0] = hi;
		}
	}
	int occ = -1;
	if (ok) {
		u64 q[W];
#pragma unroll
		for (int j = 0; j < W; j++) q[j] = v[j];
		query_packed_one<W, false>(md, q, nullptr, &occ);
	}
	if (i < n) {
		ExtWalk w;
		w.cur[0] = w.first[0] = v[0];
		w.cur[1] = w.first[1] = v[W - 1];
		w.r = SeqExtension{0, ok ? 0u : (u32)EXT_BAD_SEED, occ, -1, -1, 0, 0};
		xd.walk[i] = w;
		if (!ok && xd.rec) xd.rec[i] = w.r;
	}
	const u32 slot = wave_append_slot<u32>(cnt, ok);               // (every lane of the wave takes part)
	if (ok) live[slot] = i;
}

template <int W> __global__ __launch_bounds__(EXT_BT) void k_extend_step(ModelDev md, ExtDev xd, const u32 *live, const u32 *cnt, u32 *live_next, u32 *cnt_next, u32 *cnt_zero, int steps)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) *cnt_zero = 0;
	const u32 n_live = *cnt;
	if ((u64)blockIdx.x * EXT_WALKS >= n_live) return;
	const int lane = threadIdx.x & 63, j = lane & 7, c_me = j & 3, k = md.k;
	const bool back = j >= 4;
	const int g_sh = lane & 56, h_sh = lane & 60;                  // where the group's byte and the half's nibble sit in a ballot
	const u32 wi = blockIdx.x * EXT_WALKS + threadIdx.x / EXT_GROUP;
	const bool mine = wi < n_live;
	const u32 id = mine ? live[wi] : 0;
	u64 cur[W], first[W];
	SeqExtension r = SeqExtension{0, 0, 0, -1, -1, 0, 0};
	if (mine) {
		const ExtWalk w = xd.walk[id];
		cur[0] = w.cur[0]; first[0] = w.first[0];
		cur[W - 1] = w.cur[W - 1]; first[W - 1] = w.first[W - 1];
		r = w.r;
	} else {
#pragma unroll
		for (int x = 0; x < W; x++) cur[x] = first[x] = 0;
	}
	bool active = mine;
	// (every branch that holds a ballot or a shuffle is taken by the whole wave)
	for (int s = 0; s < steps && __any(active); s++) {
		u64 q[W];
		ext_node<W>(cur, k, back, (u32)c_me, 1, q);
		int ans = 0;
		if (active) query_packed_one<W, false>(md, q, nullptr, &ans);
		const u32 c0 = (u32)(W == 1 ? cur[0] >> (2 * (k - 1)) : cur[0] >> (2 * (k - 1) - 64)) & 3u;
		const u32 B = (u32)(__ballot(active && ans >= xd.thr && !(back && (u32)c_me == c0)) >> g_sh) & 0xFFu;
		u32 S = B & 15u, P = B >> 4;
		const bool lf = active && xd.depth > 0 && (S & (S - 1)) != 0, lb = active && xd.depth > 0 && P != 0;
		if (__any(lf || lb)) {
			u64 fr = back ? (lb ? P : 0) : (lf ? S : 0);                // my half's frontier
			for (int L = 1; L <= xd.depth; L++) {
				const bool last = L == xd.depth;
				u64 rem = fr, nxt = 0;
				while (__any(rem != 0)) {
					const int p = rem ? __ffsll((long long)rem) - 1 : -1;
					int a2 = 0;
					if (p >= 0) {
						ext_node<W>(cur, k, back, (u32)p * 4u + (u32)c_me, L + 1, q);
						query_packed_one<W, false>(md, q, nullptr, &a2);
					}
					const u64 nib = (__ballot(p >= 0 && a2 >= xd.thr) >> h_sh) & 15u;
					if (p >= 0) nxt |= last ? (u64)(nib != 0) << p : nib << (4 * p);
					rem &= rem - 1;
				}
				fr = nxt;
			}
			// fr: the nodes of `depth` bases with a solid child; lane c_me looks at those whose first base is c_me
			const int width = 1 << (2 * (xd.depth - 1));
			const u32 B2 = (u32)(__ballot(((fr >> (c_me * width)) & ((1ULL << width) - 1)) != 0) >> g_sh) & 0xFFu;
			if (lf) S = B2 & 15u;
			if (lb) P = B2 >> 4;
		}
		u32 stop = 0;
		if (!S) stop = EXT_DEAD_END;
		else if (S & (S - 1)) stop = EXT_BRANCH;
		else if (P) stop = EXT_JOIN;
		const int c = S ? __ffs((int)S) - 1 : 0;
		const int a_c = __shfl(ans, g_sh + c, 64);
		if (active && !stop) {
			ext_node<W>(cur, k, false, (u32)c, 1, q);
			if (q[0] == first[0] && q[W - 1] == first[W - 1]) stop = EXT_CYCLE;
			else {
				if (j == 0) xd.ext[(u64)id * xd.max_ext + r.n_ext] = (unsigned char)"ACGT"[c];
				r.min_occ = r.n_ext && r.min_occ < a_c ? r.min_occ : a_c;
				r.max_occ = r.n_ext && r.max_occ > a_c ? r.max_occ : a_c;
				r.n_ext++;
				r.sum_occ += (u64)(long long)a_c;
				r.n_lookahead += (lf || lb) ? 1u : 0u;
#pragma unroll
				for (int x = 0; x < W; x++) cur[x] = q[x];
				if (r.n_ext == xd.max_ext) stop = EXT_MAX_EXT;
			}
		}
		if (active && stop) { r.stop = stop; active = false; }
	}
	if (!mine || j != 0) return;
	if (r.stop) {
		if (xd.rec) xd.rec[id] = r;
		return;
	}
	ExtWalk w;
	w.cur[0] = cur[0]; w.first[0] = first[0];
	w.cur[1] = cur[W - 1]; w.first[1] = first[W - 1];
	w.r = r;
	xd.walk[id] = w;
	live_next[atomicAdd(cnt_next, 1u)] = id;
}

namespace kmxk {

// a chunk of n = v.n_seqs seeds (v.offs is the chunk's first offset; seq, offs as k_extend_init takes them): xd.walk holds
// n states, lists 2 n entries, cnt 3 counters.
// ceil(max_ext / steps) launches of k_extend_step finish every walk: a step appends a base or stops the walk.
void extend_walks(const ModelDev &md, const SeqView &v, const ExtDev &xd, u32 *lists, u32 *cnt, int steps, hipStream_t st, KernelProf *prof)
{
	const unsigned char *seq = v.seq;
	const u64 n_bases = v.g1, *offs = v.offs;                      // (where k_extend_init clamps the offsets: the end of the bases on hand)
	const u32 n = (u32)v.n_seqs;
	if (!n) return;
	(void)hipMemsetAsync(cnt, 0, 3 * sizeof(u32), st);
	KPROF_BEGIN(prof, KC_QUERY, st);
	DISPATCH_W(words(md), hipLaunchKernelGGL(k_extend_init<W>, dim3((n + 255) / 256), dim3(256), 0, st, md, seq, n_bases, offs, n, xd, lists, cnt));
	const u32 rounds = (xd.max_ext + (u32)steps - 1) / (u32)steps;
	for (u32 r = 0; r < rounds; r++)
		DISPATCH_W(words(md), hipLaunchKernelGGL(k_extend_step<W>, dim3((n + EXT_WALKS - 1) / EXT_WALKS), dim3(EXT_BT), 0, st, md, xd, (const u32 *)(lists + (u64)(r & 1) * n), (const u32 *)(cnt + r % 3),
		                                         lists + (u64)((r + 1) & 1) * n, cnt + (r + 1) % 3, cnt + (r + 2) % 3, steps));
	KPROF_END(prof, st);
}

}   // namespace kmxk
