// map_host.h -- kmx_unitig_map_*: a session that maps the windows of reads onto the unitigs of a listing (the rule: include/kmx.h;
// the kernels: map_kernels.h).  Included into kmx_api.hip after unitig_host.h, whose argument check and bucket index it shares.
// The host forms stage their buffers in a Staging and validate offsets and CSR with graph_checks.h (both: graph_host.h).
//
// begin validates the listing and builds its bucket index (k_uni_index, into the session's own array: a kmx_unitigs call on the
// handle rebuilds the other one), then the place table and m_u from the unitig set, and waits once for the two error words.
// A batch runs chunk by chunk on the model's stream (kmxk::map_chunk: codes, scan, starts, ends, advance), with no wait between
// the chunks; the records and the CSR are finished behind the last one, and one wait brings the number of segments to the host.
// The host variant sends the bases through the pinned slots of the query feed, one slot per chunk: a chunk needs no halo in
// front, because the code of the window before it is what the previous chunk left on the device.
static_assert(sizeof(kmx_map_segment) == 24 && sizeof(MapSeg) == 24 && sizeof(kmx_seq_map) == 64 && sizeof(SeqMap) == 64, "kmx_map_segment is 24 bytes, kmx_seq_map 64");
static_assert(offsetof(kmx_map_segment, n_windows) == offsetof(MapSeg, n_windows) && offsetof(kmx_map_segment, off) == offsetof(MapSeg, off) &&
              offsetof(kmx_seq_map, first_mapped) == offsetof(SeqMap, first_mapped) && offsetof(kmx_seq_map, longest) == offsetof(SeqMap, longest),
              "MapSeg and SeqMap (kmx_types.h) are the layouts of kmx_map_segment and kmx_seq_map");

static const u64 kMapChunk = u64(1) << 22;                     // windows per chunk: 20 bytes of work arrays each

// KMX_MAP_PIECE (test hook): device chunks and the host variant's pieces of this many windows, so a small test crosses many
// of their boundaries.  Read at every call.
static u64 map_chunk_size()
{
	const char *e = hook_env("KMX_MAP_PIECE");
	const long long x = e ? atoll(e) : 0;
	return x > 0 ? std::min<u64>((u64)x, kMapChunk) : kMapChunk;
}

static const char *const kMapWhat = "the unitig map";
static int map_nomem() { return graph_nomem(kMapWhat); }

static int map_session(kmx_model *m, const char *who)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!m->map.on) return fail(KMX_E_STATE, "%s outside a map session (kmx_unitig_map_begin first)", who);
	return KMX_OK;
}

// the index of a session on a device-resident listing and unitig set
static int map_begin_core(kmx_model *m, int k, const u64 *d_km, u64 n, const unsigned char *d_useq, const u64 *d_uoffs, u64 U, u64 n_ubases, bool from_count)
{
	auto &S = m->map;
	const hipStream_t st = m->stream;
	TRY(check_unitig_count(U));
	int lg = 0;
	while ((u64(1) << lg) < n) lg++;
	UniDev d{};
	d.km = d_km; d.n = n; d.k = k; d.W = (k + 31) / 32;
	d.bits = std::min({2 * k, std::max(lg, 1), kUniMaxBits});
	d.shift = 2 * k - d.bits;
	const size_t n_start = (size_t(1) << d.bits) + 1;
	if (S.d_start.ensure(n_start, st) != hipSuccess || S.d_place.ensure(n, st) != hipSuccess || S.d_mu.ensure(U, st) != hipSuccess || S.d_err.ensure(2, st) != hipSuccess) {
		map_drop(m);
		return map_nomem();
	}
	d.start = S.d_start; d.err = S.d_err;
	HIPCHK(hipMemsetAsync(S.d_err, 0, 8, st));
	HIPCHK(hipMemsetAsync(S.d_start, 0, n_start * 4, st));
	if (n) HIPCHK(hipMemsetAsync(S.d_place, 0xFF, n * 8, st));
	kmxk::unitig_index(d, st);
	d.err = S.d_err.get() + 1;
	S.dev = MapDev{d, S.d_place, S.d_mu, U};
	kmxk::map_index(S.dev, d_useq, d_uoffs, n_ubases, st);
	HIPCHK(hipGetLastError());
	u32 bad[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(bad, S.d_err, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the session's one wait
	if (bad[0]) { map_drop(m); return fail(KMX_E_ARG, "the listing is not strictly ascending, not canonical, or holds bits above 2k"); }
	if (bad[1]) {
		map_drop(m);
		return fail(KMX_E_ARG, "the unitig set is no valid set for this listing: a byte outside ACGT, a unitig shorter than k, a window that is not listed, or a k-mer that occurs twice");
	}
	S.on = true;
	S.from_count = from_count;
	return KMX_OK;
}

static int map_begin_args(kmx_model *m, int k, u64 n, const void *km, const void *useq, const void *uoffs, u64 U)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(unitig_args(k, n));
	if ((n && !km) || (U && (!useq || !uoffs))) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	map_drop(m);                                                   // a session that was open ends here
	return KMX_OK;
}

static int kmx_unitig_map_begin_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, uint64_t n, const char *d_useq, const uint64_t *d_uoffsets, uint64_t U, uint64_t n_ubases)
{
	TRY(map_begin_args(m, k, n, d_kmers, d_useq, d_uoffsets, U));
	return map_begin_core(m, k, (const u64 *)d_kmers, n, (const unsigned char *)d_useq, (const u64 *)d_uoffsets, U, n_ubases, false);
}

// the unitig set of a host variant, staged for the length of begin
static int map_set_upload(Staging &G, const char *useq, const uint64_t *uoffsets, u64 U, const unsigned char **d_useq, const u64 **d_uoffs)
{
	*d_useq = nullptr; *d_uoffs = nullptr;
	if (!U) return KMX_OK;
	TRY(check_offsets(uoffsets, U));
	*d_useq = G.in<unsigned char>(useq, uoffsets[U]);
	*d_uoffs = G.in<u64>(uoffsets, U + 1);
	return G.status();
}

static int kmx_unitig_map_begin_impl(kmx_model *m, int k, const uint64_t *kmers, uint64_t n, const char *useq, const uint64_t *uoffsets, uint64_t U)
{
	TRY(map_begin_args(m, k, n, kmers, useq, uoffsets, U));
	Staging G(m, kMapWhat);
	const unsigned char *d_useq;
	const u64 *d_uoffs;
	TRY(map_set_upload(G, useq, uoffsets, U, &d_useq, &d_uoffs));
	auto &S = m->map;
	const u64 W = (u64)(k + 31) / 32;
	if (n) {
		if (S.d_km.ensure(n * W, m->stream) != hipSuccess) { map_drop(m); return map_nomem(); }
		HIPCHK(hipMemcpyAsync(S.d_km, kmers, n * W * 8, hipMemcpyHostToDevice, m->stream));
	}
	return map_begin_core(m, k, S.d_km, n, d_useq, d_uoffs, U, U ? uoffsets[U] : 0, false);
}

static int kmx_count_unitig_map_begin_dev_impl(kmx_model *m, const char *d_useq, const uint64_t *d_uoffsets, uint64_t U, uint64_t n_ubases)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitig_map_begin_dev"));
	auto &C = m->cnt;
	TRY(map_begin_args(m, C.k, C.n_list, C.d_run[1].get(), d_useq, d_uoffsets, U));
	return map_begin_core(m, C.k, C.d_run[1], C.n_list, (const unsigned char *)d_useq, (const u64 *)d_uoffsets, U, n_ubases, true);
}

static int kmx_count_unitig_map_begin_impl(kmx_model *m, const char *useq, const uint64_t *uoffsets, uint64_t U)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitig_map_begin"));
	auto &C = m->cnt;
	TRY(map_begin_args(m, C.k, C.n_list, C.d_run[1].get(), useq, uoffsets, U));
	Staging G(m, kMapWhat);
	const unsigned char *d_useq;
	const u64 *d_uoffs;
	TRY(map_set_upload(G, useq, uoffsets, U, &d_useq, &d_uoffs));
	return map_begin_core(m, C.k, C.d_run[1], C.n_list, d_useq, d_uoffs, U, U ? uoffsets[U] : 0, true);
}

static int kmx_unitig_map_end_impl(kmx_model *m)
{
	TRY(map_session(m, "kmx_unitig_map_end"));
	HIPCHK(hipSetDevice(m->device));
	map_drop(m);
	return KMX_OK;
}

// the work arrays of chunks of `chunk` windows, and the state in front of a batch's first chunk
static int map_batch_begin(kmx_model *m, u64 chunk, MapChunk *C, const MapOut &O, u64 n_seqs)
{
	auto &S = m->map;
	const hipStream_t st = m->stream;
	if (S.d_code.ensure(chunk + 1, st) != hipSuccess || S.d_ex.ensure(chunk + 1, st) != hipSuccess || S.d_spos.ensure(chunk, st) != hipSuccess || S.d_state.ensure(2, st) != hipSuccess)
		return map_nomem();
	*C = MapChunk{S.d_code, S.d_ex, S.d_spos, S.d_state};
	HIPCHK(hipMemsetAsync(S.d_state, 0, 16, st));
	HIPCHK(hipMemsetAsync(S.d_code, 0xFF, 8, st));                 // no window in front of the first chunk
	HIPCHK(hipMemsetAsync(O.so, 0, (n_seqs + 1) * 8, st));
	kmxk::map_rec_init(O.rec, n_seqs, st);
	return KMX_OK;
}

static int map_dev_fail(hipError_t e)
{
	if (e == hipErrorOutOfMemory) return map_nomem();
	return fail(KMX_E_NODEVICE, "the unitig map failed: %s", hipGetErrorString(e));
}

static int map_range(u64 need, u64 cap) { return fail(KMX_E_RANGE, "%llu segments, the buffer holds %llu", (unsigned long long)need, (unsigned long long)cap); }

static int kmx_unitig_map_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, kmx_map_segment *d_segs, uint64_t capacity,
                                        uint64_t *n_segs, uint64_t *d_seg_offsets, kmx_seq_map *d_rec, uint64_t *d_hits)
{
	TRY(map_session(m, "kmx_unitig_map_seqs_dev"));
	if (!n_segs) return fail(KMX_E_ARG, "null argument");
	*n_segs = 0;
	if (!n_seqs) return KMX_OK;
	if (!d_offsets || !d_seg_offsets || (n_bases && !d_seq)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	auto &S = m->map;
	const hipStream_t st = m->stream;
	const u64 chunk = std::min<u64>(map_chunk_size(), std::max<u64>(n_bases, 1));
	const MapOut O{(MapSeg *)d_segs, d_segs ? capacity : 0, (u64 *)d_seg_offsets, (SeqMap *)d_rec};
	MapChunk C{};
	TRY(map_batch_begin(m, chunk, &C, O, n_seqs));
	const SeqView v{(const unsigned char *)d_seq, 0, n_bases, n_bases, (const u64 *)d_offsets, n_seqs};
	for (u64 p0 = 0; p0 < n_bases; p0 += chunk) {
		const hipError_t e = kmxk::map_chunk(S.dev, v, p0, std::min<u64>(chunk, n_bases - p0), C, O, (unsigned long long *)d_hits, S.d_tmp, st);
		if (e != hipSuccess) return map_dev_fail(e);
	}
	const hipError_t e = kmxk::map_finish(O, v.offs, n_seqs, n_bases, S.dev.d.k, S.d_tmp, st);
	if (e != hipSuccess) return map_dev_fail(e);
	u64 ns = 0;
	HIPCHK(hipMemcpyAsync(&ns, S.d_state, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait
	*n_segs = ns;
	if (d_segs && ns > capacity) return map_range(ns, capacity);
	return KMX_OK;
}

static int kmx_unitig_map_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, kmx_map_segment *segs, uint64_t capacity, uint64_t *n_segs,
                                    uint64_t *seg_offsets, kmx_seq_map *rec, uint64_t *hits)
{
	TRY(map_session(m, "kmx_unitig_map_seqs"));
	if (!n_segs) return fail(KMX_E_ARG, "null argument");
	*n_segs = 0;
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	if (!seg_offsets) return fail(KMX_E_ARG, "null argument");
	const u64 n_bases = offsets[n_seqs];
	if (!n_bases) {
		for (u64 i = 0; i <= n_seqs; i++) seg_offsets[i] = 0;
		if (rec) for (u64 i = 0; i < n_seqs; i++) rec[i] = kmx_seq_map{0, 0, 0, 0, 0, 0, 0, 0};
		return KMX_OK;
	}
	if (!seq) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	auto &S = m->map;
	const hipStream_t st = m->stream;
	std::lock_guard<std::mutex> lk(m->query_mu);                  // the pinned slots of m->qfeed
	Staging G(m, kMapWhat);
	const u64 U = S.dev.U, seg_cap = segs ? std::min<u64>(capacity, n_bases) : 0;
	const u64 *d_offs = G.in<u64>(offsets, n_seqs + 1);
	const MapOut O{segs ? G.out<MapSeg>(seg_cap) : nullptr, seg_cap, G.out<u64>(n_seqs + 1), rec ? G.out<SeqMap>(n_seqs) : nullptr};
	unsigned long long *d_hits = hits && U ? G.zeroed<unsigned long long>(U) : nullptr;
	TRY(G.status());
	SeqChunks sc(seq, offsets, n_seqs, (u64)S.dev.d.k, map_chunk_size());
	const SlotShape shape = sc.bases_shape();
	MapChunk C{};
	TRY(map_batch_begin(m, sc.C, &C, O, n_seqs));
	if (ensure_query_feed(m, shape.slot_bytes, 0) != KMX_OK) return map_nomem();
	auto &F = m->qfeed;
	hipError_t le = hipSuccess;
	TRY(query_pipeline(m, n_bases, 1, seq_workers(n_bases),
		[&](int, u64 lo, u64 hi, unsigned char *dst) { sc.stage_bases(lo, hi, dst); },
		[&](int s, u64 cn, u64 c) {
			if (le != hipSuccess) return;
			le = kmxk::map_chunk(S.dev, SeqView{F.d_in[s], c * sc.C, c * sc.C + sc.nbytes_of(c), n_bases, d_offs, n_seqs}, c * sc.C, cn, C, O, d_hits, S.d_tmp, st);
		}, (int32_t *)nullptr, &shape));
	if (le != hipSuccess) return map_dev_fail(le);
	const hipError_t e = kmxk::map_finish(O, d_offs, n_seqs, n_bases, S.dev.d.k, S.d_tmp, st);
	if (e != hipSuccess) return map_dev_fail(e);
	u64 ns = 0;
	G.down(&ns, S.d_state.get(), 1);
	G.down(seg_offsets, O.so, n_seqs + 1);
	if (rec) G.down(rec, O.rec, n_seqs);
	if (d_hits) G.down_add(hits, d_hits, U);
	TRY(G.finish());
	*n_segs = ns;
	if (!segs) return KMX_OK;
	if (ns > capacity) return map_range(ns, capacity);
	G.down(segs, O.segs, ns);
	return G.finish();
}

// ---- kmx_unitig_walk_segs*: the walks of a batch's segments (the rule: include/kmx.h; the kernels: walk_kernels.h).  A post-pass
// inside the session: the work arrays grow with n_segs and stay on the handle, everything is enqueued on the model's stream, and
// one wait brings the two totals and the five counters to the host.  The entry point fills a WalkArgs, walk_args checks it for both
// forms and walk_dev_of fills the kernel block's sizes: the forms differ in what the host one validates, stages and downloads.
static_assert(sizeof(kmx_walk) == 80 && sizeof(Walk) == 80 && sizeof(kmx_walk_stats) == 64 && sizeof(kmx_walk_params) == 16 && sizeof(WalkTot) == 16, "kmx_walk is 80 bytes, kmx_walk_stats 64, kmx_walk_params 16");
static_assert(offsetof(kmx_walk, first_seg) == offsetof(Walk, first_seg) && offsetof(kmx_walk, n_segs) == offsetof(Walk, n_segs) && offsetof(kmx_walk, off_last) == offsetof(Walk, off_last) &&
              offsetof(kmx_walk, n_across) == offsetof(Walk, n_across) && offsetof(kmx_walk, indel) == offsetof(Walk, indel), "Walk (kmx_types.h) is the layout of kmx_walk");

// the buffers of one call: what both forms check before anything runs
struct WalkArgs {
	const kmx_map_segment *segs; u64 n_segs;
	const uint64_t *so; u64 n_seqs;
	const uint64_t *loffs; const uint32_t *links; u64 n_links;
	const kmx_walk_params *params;
	kmx_walk *walks; u64 walk_cap; uint64_t *wo; uint32_t *steps; u64 step_cap;
	uint64_t *link_hits;
	kmx_walk_stats *stats;
};

static int walk_args(kmx_model *m, const char *who, const WalkArgs &A)
{
	TRY(map_session(m, who));
	const kmx_walk_params *p = A.params;
	if (!p || !A.stats) return fail(KMX_E_ARG, "null argument");
	if (p->max_indel > 255) return fail(KMX_E_ARG, "max_indel = %u: at most 255", p->max_indel);
	if (p->reserved[0] || p->reserved[1]) return fail(KMX_E_ARG, "kmx_walk_params.reserved is not 0");
	*A.stats = kmx_walk_stats{0, 0, 0, 0, 0, 0, 0, 0};
	if (!A.n_seqs) return KMX_OK;
	if (!A.so || !A.wo || (A.n_segs && !A.segs) || !A.loffs || (A.n_links && !A.links) || (A.walks && !A.steps)) return fail(KMX_E_ARG, "null argument");
	return KMX_OK;
}

static int walk_range(const kmx_walk_stats &s, u64 walk_cap, u64 step_cap)
{
	return fail(KMX_E_RANGE, "%llu walks and %llu steps, the buffers hold %llu and %llu", (unsigned long long)s.n_walks, (unsigned long long)s.n_steps, (unsigned long long)walk_cap, (unsigned long long)step_cap);
}

// the pass on device buffers (D: input, parameters and output; the session's part and the work arrays are filled in here)
static int walk_core(kmx_model *m, WalkDev D, kmx_walk_stats *stats)
{
	auto &S = m->map;
	const hipStream_t st = m->stream;
	if (!D.n_segs) {
		HIPCHK(hipMemsetAsync(D.wo, 0, (D.n_seqs + 1) * 8, st));
		HIPCHK(hipStreamSynchronize(st));
		return KMX_OK;
	}
	if (S.d_wflag.ensure(D.n_segs, st) != hipSuccess || S.d_wjoin.ensure(D.n_segs, st) != hipSuccess || S.d_wsc.ensure(D.n_segs + 1, st) != hipSuccess || S.d_wcnt.ensure(WALK_C_N, st) != hipSuccess)
		return map_nomem();
	D.mu = S.dev.mu; D.U = S.dev.U; D.k = S.dev.d.k;
	D.flag = S.d_wflag; D.join = S.d_wjoin; D.sc = S.d_wsc; D.cnt = S.d_wcnt;
	const hipError_t e = kmxk::walk_segs(D, S.d_tmp, st);
	if (e != hipSuccess) return map_dev_fail(e);
	WalkTot tot{0, 0};
	unsigned long long c[WALK_C_N] = {0, 0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&tot, D.sc + D.n_segs, sizeof tot, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait
	*stats = kmx_walk_stats{tot.w, tot.s, c[WALK_C_EDGE], c[WALK_C_INSIDE], c[WALK_C_ACROSS], c[WALK_C_UNLINKED], c[WALK_C_BREAKS], 0};
	return D.walks && (tot.w > D.walk_cap || tot.s > D.step_cap) ? walk_range(*stats, D.walk_cap, D.step_cap) : KMX_OK;
}

// the sizes and parameters of the kernel block; the pointers are the form's own
static WalkDev walk_dev_of(const WalkArgs &A)
{
	WalkDev D{};
	D.n_segs = A.n_segs; D.n_seqs = A.n_seqs; D.n_links = A.n_links;
	D.max_gap = A.params->max_gap; D.max_indel = A.params->max_indel;
	D.walk_cap = A.walks ? A.walk_cap : 0; D.step_cap = A.walks ? A.step_cap : 0;
	return D;
}

static int kmx_unitig_walk_segs_dev_impl(kmx_model *m, const WalkArgs &A)
{
	TRY(walk_args(m, "kmx_unitig_walk_segs_dev", A));
	if (!A.n_seqs) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	WalkDev D = walk_dev_of(A);
	D.segs = (const MapSeg *)A.segs; D.so = (const u64 *)A.so; D.loffs = (const u64 *)A.loffs; D.links = A.links;
	D.walks = (Walk *)A.walks; D.wo = (u64 *)A.wo; D.steps = A.walks ? A.steps : nullptr; D.link_hits = (unsigned long long *)A.link_hits;
	return walk_core(m, D, A.stats);
}

static int kmx_unitig_walk_segs_impl(kmx_model *m, const WalkArgs &A)
{
	TRY(walk_args(m, "kmx_unitig_walk_segs", A));
	if (!A.n_seqs) return KMX_OK;
	const u64 n_segs = A.n_segs, n_seqs = A.n_seqs, n_links = A.n_links;
	TRY(check_offsets(A.so, n_seqs));
	if (A.so[n_seqs] != n_segs) return fail(KMX_E_ARG, "seg_offsets end at %llu, not at n_segs = %llu", (unsigned long long)A.so[n_seqs], (unsigned long long)n_segs);
	TRY(check_link_csr(A.loffs, A.links, n_links, m->map.dev.U, false));
	HIPCHK(hipSetDevice(m->device));
	Staging G(m, kMapWhat);
	WalkDev D = walk_dev_of(A);
	D.walk_cap = std::min<u64>(D.walk_cap, n_segs); D.step_cap = std::min<u64>(D.step_cap, n_segs);   // a segment starts at most one walk and one step
	D.segs = G.in<MapSeg>(A.segs, n_segs); D.so = G.in<u64>(A.so, n_seqs + 1); D.loffs = G.in<u64>(A.loffs, 2 * m->map.dev.U + 1); D.links = G.in<u32>(A.links, n_links);
	D.wo = G.out<u64>(n_seqs + 1);
	if (A.walks) { D.walks = G.out<Walk>(D.walk_cap); D.steps = G.out<u32>(D.step_cap); }
	if (A.link_hits && n_links) D.link_hits = G.zeroed<unsigned long long>(n_links);
	TRY(G.status());
	const int rc = walk_core(m, D, A.stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	const kmx_walk_stats &s = *A.stats;
	const bool short_cap = A.walks && (s.n_walks > A.walk_cap || s.n_steps > A.step_cap);
	G.down(A.wo, D.wo, n_seqs + 1);
	G.down_add(A.link_hits, D.link_hits, D.link_hits ? n_links : 0);
	if (A.walks && !short_cap) { G.down(A.walks, D.walks, s.n_walks); G.down(A.steps, D.steps, s.n_steps); }
	TRY(G.finish());
	return short_cap ? walk_range(s, A.walk_cap, A.step_cap) : KMX_OK;
}
