// map_host.h -- kmx_unitig_map_*: a session that maps the windows of reads onto the unitigs of a listing (the rule: include/kmx.h;
// the kernels: map_kernels.h).  Included into kmx_api.hip after unitig_host.h, whose argument check and bucket index it shares.
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

static int map_nomem() { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of the unitig map could not be allocated"); }

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
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: a map takes fewer than 2^31", (unsigned long long)U);
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

// the unitig set of a host variant, on the device for the length of begin
struct MapSetOnDevice {
	kmx_model *m;
	DevBuf<unsigned char> seq;
	DevBuf<u64> offs;
	~MapSetOnDevice() { (void)hipStreamSynchronize(m->stream); }
	int upload(const char *useq, const uint64_t *uoffsets, u64 U)
	{
		if (!U) return KMX_OK;
		TRY(check_offsets(uoffsets, U));
		if (seq.alloc(uoffsets[U]) != hipSuccess || offs.alloc(U + 1) != hipSuccess) return map_nomem();
		if (uoffsets[U]) HIPCHK(hipMemcpyAsync(seq, useq, uoffsets[U], hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(offs, uoffsets, (U + 1) * 8, hipMemcpyHostToDevice, m->stream));
		return KMX_OK;
	}
};

static int kmx_unitig_map_begin_impl(kmx_model *m, int k, const uint64_t *kmers, uint64_t n, const char *useq, const uint64_t *uoffsets, uint64_t U)
{
	TRY(map_begin_args(m, k, n, kmers, useq, uoffsets, U));
	MapSetOnDevice set{m};
	TRY(set.upload(useq, uoffsets, U));
	auto &S = m->map;
	const u64 W = (u64)(k + 31) / 32;
	if (n) {
		if (S.d_km.ensure(n * W, m->stream) != hipSuccess) { map_drop(m); return map_nomem(); }
		HIPCHK(hipMemcpyAsync(S.d_km, kmers, n * W * 8, hipMemcpyHostToDevice, m->stream));
	}
	return map_begin_core(m, k, S.d_km, n, set.seq, set.offs, U, U ? uoffsets[U] : 0, false);
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
	MapSetOnDevice set{m};
	TRY(set.upload(useq, uoffsets, U));
	return map_begin_core(m, C.k, C.d_run[1], C.n_list, set.seq, set.offs, U, U ? uoffsets[U] : 0, true);
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
	struct Staged {                                                // the call's own device buffers; the stream is drained before they go
		kmx_model *m;
		DevBuf<u64> offs, so, hits;
		DevBuf<MapSeg> segs;
		DevBuf<SeqMap> rec;
		~Staged() { (void)hipStreamSynchronize(m->stream); }
	} D{m};
	const u64 U = S.dev.U, seg_cap = segs ? std::min<u64>(capacity, n_bases) : 0;
	if (D.offs.alloc(n_seqs + 1) != hipSuccess || D.so.alloc(n_seqs + 1) != hipSuccess || (rec && D.rec.alloc(n_seqs) != hipSuccess) || (segs && D.segs.alloc(seg_cap) != hipSuccess) ||
	    (hits && U && D.hits.alloc(U) != hipSuccess))
		return map_nomem();
	HIPCHK(hipMemcpyAsync(D.offs, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
	unsigned long long *d_hits = hits && U ? (unsigned long long *)D.hits.get() : nullptr;
	if (d_hits) HIPCHK(hipMemsetAsync(d_hits, 0, U * 8, st));
	SeqChunks sc(seq, offsets, n_seqs, (u64)S.dev.d.k, map_chunk_size());
	const SlotShape shape = sc.bases_shape();
	const MapOut O{segs ? D.segs.get() : nullptr, seg_cap, D.so, rec ? D.rec.get() : nullptr};
	MapChunk C{};
	TRY(map_batch_begin(m, sc.C, &C, O, n_seqs));
	if (ensure_query_feed(m, shape.slot_bytes, 0) != KMX_OK) return map_nomem();
	auto &F = m->qfeed;
	hipError_t le = hipSuccess;
	TRY(query_pipeline(m, n_bases, 1, seq_workers(n_bases),
		[&](int, u64 lo, u64 hi, unsigned char *dst) { sc.stage_bases(lo, hi, dst); },
		[&](int s, u64 cn, u64 c) {
			if (le != hipSuccess) return;
			le = kmxk::map_chunk(S.dev, SeqView{F.d_in[s], c * sc.C, c * sc.C + sc.nbytes_of(c), n_bases, D.offs, n_seqs}, c * sc.C, cn, C, O, d_hits, S.d_tmp, st);
		}, (int32_t *)nullptr, &shape));
	if (le != hipSuccess) return map_dev_fail(le);
	const hipError_t e = kmxk::map_finish(O, D.offs, n_seqs, n_bases, S.dev.d.k, S.d_tmp, st);
	if (e != hipSuccess) return map_dev_fail(e);
	u64 ns = 0;
	std::vector<uint64_t> h;
	if (d_hits) h.resize(U);
	HIPCHK(hipMemcpyAsync(&ns, S.d_state, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(seg_offsets, D.so, (n_seqs + 1) * 8, hipMemcpyDeviceToHost, st));
	if (rec) HIPCHK(hipMemcpyAsync(rec, D.rec, n_seqs * sizeof(SeqMap), hipMemcpyDeviceToHost, st));
	if (d_hits) HIPCHK(hipMemcpyAsync(h.data(), d_hits, U * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	for (u64 u = 0; u < h.size(); u++) hits[u] += h[u];
	*n_segs = ns;
	if (!segs) return KMX_OK;
	if (ns > capacity) return map_range(ns, capacity);
	if (ns) HIPCHK(hipMemcpyAsync(segs, D.segs, ns * sizeof(MapSeg), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

// ---- kmx_unitig_walk_segs*: the walks of a batch's segments (the rule: include/kmx.h; the kernels: walk_kernels.h).  A post-pass
// inside the session: the work arrays grow with n_segs and stay on the handle, everything is enqueued on the model's stream, and
// one wait brings the two totals and the five counters to the host.
static_assert(sizeof(kmx_walk) == 80 && sizeof(Walk) == 80 && sizeof(kmx_walk_stats) == 64 && sizeof(kmx_walk_params) == 16 && sizeof(WalkTot) == 16, "kmx_walk is 80 bytes, kmx_walk_stats 64, kmx_walk_params 16");
static_assert(offsetof(kmx_walk, first_seg) == offsetof(Walk, first_seg) && offsetof(kmx_walk, n_segs) == offsetof(Walk, n_segs) && offsetof(kmx_walk, off_last) == offsetof(Walk, off_last) &&
              offsetof(kmx_walk, n_across) == offsetof(Walk, n_across) && offsetof(kmx_walk, indel) == offsetof(Walk, indel), "Walk (kmx_types.h) is the layout of kmx_walk");

static int walk_args(kmx_model *m, const char *who, const kmx_walk_params *p, kmx_walk_stats *stats)
{
	TRY(map_session(m, who));
	if (!p || !stats) return fail(KMX_E_ARG, "null argument");
	if (p->max_indel > 255) return fail(KMX_E_ARG, "max_indel = %u: at most 255", p->max_indel);
	if (p->reserved[0] || p->reserved[1]) return fail(KMX_E_ARG, "kmx_walk_params.reserved is not 0");
	*stats = kmx_walk_stats{0, 0, 0, 0, 0, 0, 0, 0};
	return KMX_OK;
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
	if (D.walks && (tot.w > D.walk_cap || tot.s > D.step_cap))
		return fail(KMX_E_RANGE, "%llu walks and %llu steps, the buffers hold %llu and %llu", (unsigned long long)tot.w, (unsigned long long)tot.s, (unsigned long long)D.walk_cap, (unsigned long long)D.step_cap);
	return KMX_OK;
}

static int kmx_unitig_walk_segs_dev_impl(kmx_model *m, const kmx_map_segment *d_segs, uint64_t n_segs, const uint64_t *d_seg_offsets, uint64_t n_seqs, const uint64_t *d_link_offsets,
                                         const uint32_t *d_links, uint64_t n_links, const kmx_walk_params *params, kmx_walk *d_walks, uint64_t walk_capacity, uint64_t *d_walk_offsets,
                                         uint32_t *d_steps, uint64_t step_capacity, uint64_t *d_link_hits, kmx_walk_stats *stats)
{
	TRY(walk_args(m, "kmx_unitig_walk_segs_dev", params, stats));
	if (!n_seqs) return KMX_OK;
	if (!d_seg_offsets || !d_walk_offsets || (n_segs && !d_segs) || !d_link_offsets || (n_links && !d_links) || (d_walks && !d_steps)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	WalkDev D{};
	D.segs = (const MapSeg *)d_segs; D.n_segs = n_segs; D.so = (const u64 *)d_seg_offsets; D.n_seqs = n_seqs;
	D.loffs = (const u64 *)d_link_offsets; D.links = d_links; D.n_links = n_links;
	D.max_gap = params->max_gap; D.max_indel = params->max_indel;
	D.walks = (Walk *)d_walks; D.walk_cap = d_walks ? walk_capacity : 0; D.wo = (u64 *)d_walk_offsets;
	D.steps = d_walks ? d_steps : nullptr; D.step_cap = d_walks ? step_capacity : 0;
	D.link_hits = (unsigned long long *)d_link_hits;
	return walk_core(m, D, stats);
}

static int kmx_unitig_walk_segs_impl(kmx_model *m, const kmx_map_segment *segs, uint64_t n_segs, const uint64_t *seg_offsets, uint64_t n_seqs, const uint64_t *link_offsets,
                                     const uint32_t *links, uint64_t n_links, const kmx_walk_params *params, kmx_walk *walks, uint64_t walk_capacity, uint64_t *walk_offsets,
                                     uint32_t *steps, uint64_t step_capacity, uint64_t *link_hits, kmx_walk_stats *stats)
{
	TRY(walk_args(m, "kmx_unitig_walk_segs", params, stats));
	if (!n_seqs) return KMX_OK;
	auto &S = m->map;
	const u64 U = S.dev.U;
	TRY(check_offsets(seg_offsets, n_seqs));
	if (seg_offsets[n_seqs] != n_segs) return fail(KMX_E_ARG, "seg_offsets end at %llu, not at n_segs = %llu", (unsigned long long)seg_offsets[n_seqs], (unsigned long long)n_segs);
	TRY(check_offsets(link_offsets, 2 * U));
	if (link_offsets[2 * U] != n_links) return fail(KMX_E_ARG, "link_offsets end at %llu, not at n_links = %llu", (unsigned long long)link_offsets[2 * U], (unsigned long long)n_links);
	if (!walk_offsets || (n_segs && !segs) || (n_links && !links) || (walks && !steps)) return fail(KMX_E_ARG, "null argument");
	for (u64 e = 0; e < n_links; e++)
		if ((u64)links[e] >= 2 * U) return fail(KMX_E_ARG, "links[%llu] = %u is no oriented unitig of the session's %llu", (unsigned long long)e, links[e], (unsigned long long)U);
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	struct Staged {                                                // the call's own device buffers; the stream is drained before they go
		kmx_model *m;
		DevBuf<MapSeg> segs;
		DevBuf<u64> so, loffs, wo, hits;
		DevBuf<u32> links, steps;
		DevBuf<Walk> walks;
		~Staged() { (void)hipStreamSynchronize(m->stream); }
	} G{m};
	const u64 wcap = walks ? std::min<u64>(walk_capacity, n_segs) : 0, scap = walks ? std::min<u64>(step_capacity, n_segs) : 0;
	if (G.segs.alloc(n_segs) != hipSuccess || G.so.alloc(n_seqs + 1) != hipSuccess || G.loffs.alloc(2 * U + 1) != hipSuccess || G.links.alloc(n_links) != hipSuccess ||
	    G.wo.alloc(n_seqs + 1) != hipSuccess || (walks && (G.walks.alloc(wcap) != hipSuccess || G.steps.alloc(scap) != hipSuccess)) || (link_hits && n_links && G.hits.alloc(n_links) != hipSuccess))
		return map_nomem();
	if (n_segs) HIPCHK(hipMemcpyAsync(G.segs, segs, n_segs * sizeof(MapSeg), hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.so, seg_offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.loffs, link_offsets, (2 * U + 1) * 8, hipMemcpyHostToDevice, st));
	if (n_links) HIPCHK(hipMemcpyAsync(G.links, links, n_links * 4, hipMemcpyHostToDevice, st));
	unsigned long long *d_hits = link_hits && n_links ? (unsigned long long *)G.hits.get() : nullptr;
	if (d_hits) HIPCHK(hipMemsetAsync(d_hits, 0, n_links * 8, st));
	WalkDev D{};
	D.segs = G.segs; D.n_segs = n_segs; D.so = G.so; D.n_seqs = n_seqs;
	D.loffs = G.loffs; D.links = G.links; D.n_links = n_links;
	D.max_gap = params->max_gap; D.max_indel = params->max_indel;
	D.walks = walks ? G.walks.get() : nullptr; D.walk_cap = wcap; D.wo = G.wo;
	D.steps = walks ? G.steps.get() : nullptr; D.step_cap = scap;
	D.link_hits = d_hits;
	const int rc = walk_core(m, D, stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	const bool short_cap = walks && (stats->n_walks > walk_capacity || stats->n_steps > step_capacity);
	std::vector<uint64_t> h;
	if (d_hits) h.resize(n_links);
	HIPCHK(hipMemcpyAsync(walk_offsets, G.wo, (n_seqs + 1) * 8, hipMemcpyDeviceToHost, st));
	if (d_hits) HIPCHK(hipMemcpyAsync(h.data(), d_hits, n_links * 8, hipMemcpyDeviceToHost, st));
	if (walks && !short_cap) {
		if (stats->n_walks) HIPCHK(hipMemcpyAsync(walks, G.walks, stats->n_walks * sizeof(Walk), hipMemcpyDeviceToHost, st));
		if (stats->n_steps) HIPCHK(hipMemcpyAsync(steps, G.steps, stats->n_steps * 4, hipMemcpyDeviceToHost, st));
	}
	HIPCHK(hipStreamSynchronize(st));
	for (u64 e = 0; e < h.size(); e++) link_hits[e] += h[e];
	if (short_cap)
		return fail(KMX_E_RANGE, "%llu walks and %llu steps, the buffers hold %llu and %llu", (unsigned long long)stats->n_walks, (unsigned long long)stats->n_steps, (unsigned long long)walk_capacity,
		            (unsigned long long)step_capacity);
	return KMX_OK;
}
