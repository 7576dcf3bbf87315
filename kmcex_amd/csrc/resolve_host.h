// resolve_host.h -- kmx_unitig_walk_through[_dev]: the through hits of a batch's walks (the rule: include/kmx.h; the kernels:
// resolve_kernels.h; the launcher: unitig_device.hip).  Included into kmx_api.hip after contig_host.h.
//
// through_core runs the count on device buffers: the marks and the three counters stay on the handle by capacity
// (kmx_model::res), everything is enqueued on the model's stream, and ONE wait brings the counters to the host.  The _dev form
// checks what can be checked without reading a buffer and hands the caller's pointers over; the host form validates the walks and
// the CSR, stages its input and a zeroed through of its own for the length of the call, downloads it and adds.
static_assert(sizeof(kmx_through_stats) == 64, "kmx_through_stats is 64 bytes");

static int thr_nomem() { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of the through hits could not be allocated"); }

// what both forms check before anything runs
static int through_args(kmx_model *m, const void *walks, u64 n_walks, const void *steps, u64 n_steps, const void *link_offsets, const void *links, u64 n_links, u64 U, const void *through,
                        kmx_through_stats *stats)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!stats || !link_offsets || (n_walks && !walks) || (n_steps && !steps) || (n_links && !links) || (U && !through)) return fail(KMX_E_ARG, "null argument");
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: the through hits take fewer than 2^31", (unsigned long long)U);
	*stats = kmx_through_stats{n_walks, n_steps, 0, 0, 0, {0, 0, 0}};
	return KMX_OK;
}

// the count on device buffers (D: input and output; the work arrays are filled in here); D.n_steps > 0 and D.U > 0
static int through_core(kmx_model *m, ThroughDev D, kmx_through_stats *stats)
{
	auto &S = m->res;
	const hipStream_t st = m->stream;
	if (S.d_mark.ensure(D.n_steps + 1, st) != hipSuccess || S.d_cnt.ensure(THR_C_N, st) != hipSuccess) return thr_nomem();
	D.mark = S.d_mark; D.cnt = S.d_cnt;
	HIPCHK(kmxk::walk_through(D, st));
	unsigned long long c[THR_C_N] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait
	HIPCHK(hipGetLastError());
	stats->n_interior = c[THR_C_INTERIOR];
	stats->n_added = c[THR_C_ADDED];
	stats->n_missing = c[THR_C_MISSING];
	return KMX_OK;
}

static int kmx_unitig_walk_through_dev_impl(kmx_model *m, const kmx_walk *d_walks, uint64_t n_walks, const uint32_t *d_steps, uint64_t n_steps, const uint64_t *d_link_offsets, const uint32_t *d_links,
                                            uint64_t n_links, uint64_t U, uint64_t *d_through, kmx_through_stats *stats)
{
	TRY(through_args(m, d_walks, n_walks, d_steps, n_steps, d_link_offsets, d_links, n_links, U, d_through, stats));
	if (!n_steps || !U) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	ThroughDev D{};
	D.walks = (const Walk *)d_walks; D.n_walks = n_walks; D.steps = d_steps; D.n_steps = n_steps;
	D.loffs = (const u64 *)d_link_offsets; D.links = d_links; D.n_links = n_links; D.U = U;
	D.through = (unsigned long long *)d_through;
	return through_core(m, D, stats);
}

static int kmx_unitig_walk_through_impl(kmx_model *m, const kmx_walk *walks, uint64_t n_walks, const uint32_t *steps, uint64_t n_steps, const uint64_t *link_offsets, const uint32_t *links,
                                        uint64_t n_links, uint64_t U, uint64_t *through, kmx_through_stats *stats)
{
	TRY(through_args(m, walks, n_walks, steps, n_steps, link_offsets, links, n_links, U, through, stats));
	u64 at = 0;
	for (u64 w = 0; w < n_walks; w++) {
		if (walks[w].first_step != at) return fail(KMX_E_ARG, "walk %llu starts at step %llu, not at %llu", (unsigned long long)w, (unsigned long long)walks[w].first_step, (unsigned long long)at);
		at += walks[w].n_steps;
	}
	if (at != n_steps) return fail(KMX_E_ARG, "the walks hold %llu steps, not n_steps = %llu", (unsigned long long)at, (unsigned long long)n_steps);
	TRY(check_offsets(link_offsets, 2 * U));
	if (link_offsets[2 * U] != n_links) return fail(KMX_E_ARG, "link_offsets end at %llu, not at n_links = %llu", (unsigned long long)link_offsets[2 * U], (unsigned long long)n_links);
	for (u64 e = 0; e < n_links; e++)
		if ((u64)links[e] >= 2 * U) return fail(KMX_E_ARG, "links[%llu] = %u is no oriented unitig of %llu", (unsigned long long)e, links[e], (unsigned long long)U);
	if (!n_steps || !U) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	struct Staged {                                                // the call's own device buffers; the stream is drained before they go
		kmx_model *m;
		DevBuf<Walk> walks;
		DevBuf<u32> steps, links;
		DevBuf<u64> loffs;
		DevBuf<unsigned long long> through;
		~Staged() { (void)hipStreamSynchronize(m->stream); }
	} G{m};
	if (G.walks.alloc(n_walks) != hipSuccess || G.steps.alloc(n_steps) != hipSuccess || G.links.alloc(n_links) != hipSuccess || G.loffs.alloc(2 * U + 1) != hipSuccess ||
	    G.through.alloc(16 * U) != hipSuccess)
		return thr_nomem();
	HIPCHK(hipMemcpyAsync(G.walks, walks, n_walks * sizeof(Walk), hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.steps, steps, n_steps * 4, hipMemcpyHostToDevice, st));
	if (n_links) HIPCHK(hipMemcpyAsync(G.links, links, n_links * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.loffs, link_offsets, (2 * U + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemsetAsync(G.through, 0, 16 * U * 8, st));
	ThroughDev D{};
	D.walks = G.walks; D.n_walks = n_walks; D.steps = G.steps; D.n_steps = n_steps;
	D.loffs = G.loffs; D.links = G.links; D.n_links = n_links; D.U = U;
	D.through = G.through;
	TRY(through_core(m, D, stats));
	std::vector<uint64_t> h(16 * U);
	HIPCHK(hipMemcpyAsync(h.data(), G.through, 16 * U * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	for (u64 i = 0; i < h.size(); i++) through[i] += h[i];
	return KMX_OK;
}

// ---- kmx_unitig_resolve[_dev]: the graph with every resolved unitig split into one copy per way in.  resolve_core runs the
// transform on device buffers: the unmirrored edges, the verdicts and their scan, ONE wait for the two counts and the counters,
// the check of the capacities, then records, links and the bytes.  The work arrays stay on the handle by capacity.
static_assert(sizeof(kmx_resolve_params) == 16 && sizeof(kmx_resolve_place) == 8 && sizeof(ResPlace) == 8 && sizeof(kmx_resolve_stats) == 64,
              "kmx_resolve_params is 16 bytes, kmx_resolve_place 8, kmx_resolve_stats 64");

static int res_nomem() { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of the resolution could not be allocated"); }

// what both forms check before anything runs
static int resolve_args(kmx_model *m, int k, u64 U, const kmx_resolve_params *p, const CtgSpan *spans, int n_spans, uint64_t *n_unitigs_out, uint64_t *n_bases_out, kmx_resolve_stats *stats)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (k < 5 || k > 63 || !(k & 1)) return fail(KMX_E_ARG, "the resolution needs an odd k in [5, 63], not %d", k);
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: the resolution takes fewer than 2^31", (unsigned long long)U);
	if (!p || !n_unitigs_out || !n_bases_out || !stats) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < n_spans; i++)
		if (!spans[i].p && spans[i].bytes) return fail(KMX_E_ARG, "null argument (buffer %d of the call)", i);
	for (int i = 0; i < n_spans; i++)
		for (int j = i + 1; j < n_spans; j++)
			if ((spans[i].out || spans[j].out) && ctg_overlap(spans[i].p, spans[i].bytes, spans[j].p, spans[j].bytes))
				return fail(KMX_E_ARG, "an output buffer overlaps another buffer of the call (buffers %d and %d)", i, j);
	*n_unitigs_out = *n_bases_out = 0;
	*stats = kmx_resolve_stats{0, 0, 0, 0, 0, 0, 0, 0};
	return KMX_OK;
}

struct ResClock {
	kmx_model *m;
	std::chrono::steady_clock::time_point t0;
	explicit ResClock(kmx_model *mm) : m(mm) { if (m->prof.on) { hipStreamSynchronize(m->stream); t0 = std::chrono::steady_clock::now(); } }
	void lap(int phase)
	{
		if (!m->prof.on) return;
		hipStreamSynchronize(m->stream);
		const auto t1 = std::chrono::steady_clock::now();
		m->res.phase_s[phase] += std::chrono::duration<double>(t1 - t0).count();
		t0 = t1;
	}
};

// the transform on device buffers (D: input, parameters and output; the work arrays are filled in here); D.U > 0.  D.rseq == null:
// the sizing call
static int resolve_core(kmx_model *m, ResDev D, uint64_t *n_unitigs_out, uint64_t *n_bases_out, kmx_resolve_stats *stats)
{
	auto &S = m->res;
	const hipStream_t st = m->stream;
	const u64 U = D.U;
	for (double &s : S.phase_s) s = 0;
	if (S.d_bad.ensure(U, st) != hipSuccess || S.d_ver.ensure(U, st) != hipSuccess || S.d_tot.ensure(U + 1, st) != hipSuccess || S.d_sc.ensure(U + 1, st) != hipSuccess ||
	    S.d_rcnt.ensure(RES_C_N, st) != hipSuccess)
		return res_nomem();
	D.bad = S.d_bad; D.ver = S.d_ver; D.sc = S.d_sc; D.cnt = S.d_rcnt;
	ResClock clk(m);
	HIPCHK(kmxk::resolve_verdicts(D, S.d_tot, st));
	clk.lap(0);
	const hipError_t e = kmxk::resolve_scan(D, S.d_tot, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return res_nomem();
	HIPCHK(e);
	CtgTot tot{0, 0, 0};
	unsigned long long c[RES_C_N] = {0, 0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&tot, D.sc + U, sizeof tot, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait: the counts and the counters
	HIPCHK(hipGetLastError());
	*n_unitigs_out = tot.n;
	*n_bases_out = tot.len;
	*stats = kmx_resolve_stats{c[RES_C_CANDIDATES], c[RES_C_RESOLVED], c[RES_C_CROSSED], c[RES_C_UNSUPPORTED], c[RES_C_AMBIGUOUS], tot.n - U, tot.n, 0};
	if (tot.n >> 31) return fail(KMX_E_RANGE, "%llu unitigs out: a unitig set holds fewer than 2^31", (unsigned long long)tot.n);
	if (!D.rseq) return KMX_OK;                                    // the sizing call
	if (tot.n > D.rec_cap || tot.len > D.seq_cap)
		return fail(KMX_E_RANGE, "%llu unitigs of %llu bytes, the buffers hold %llu and %llu", (unsigned long long)tot.n, (unsigned long long)tot.len, (unsigned long long)D.rec_cap, (unsigned long long)D.seq_cap);
	kmxk::resolve_records(D, st);
	clk.lap(1);
	kmxk::resolve_links(D, st);
	clk.lap(2);
	kmxk::resolve_bytes(D, st);
	clk.lap(3);
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

static int kmx_unitig_resolve_dev_impl(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t U, uint64_t n_ubases, const kmx_unitig *d_urec, const uint64_t *d_link_offsets,
                                       const uint32_t *d_links, uint64_t n_links, const uint64_t *d_link_hits, const uint64_t *d_through, const kmx_resolve_params *params, char *d_rseq,
                                       uint64_t seq_capacity, uint64_t *d_roffsets, uint64_t rec_capacity, kmx_unitig *d_rrec, uint32_t *d_origin, kmx_resolve_place *d_rplace, uint64_t *d_rlink_offsets,
                                       uint32_t *d_rlinks, uint64_t *d_link_origin, uint64_t *d_rlink_hits, uint64_t *n_unitigs_out, uint64_t *n_bases_out, kmx_resolve_stats *stats)
{
	const u64 U1 = (U >> 31) ? 0 : U, rc = d_rseq ? rec_capacity : 0, sc = d_rseq ? seq_capacity : 0, nl = d_rseq ? n_links : 0, up = d_rseq ? U1 : 0;
	if (d_rseq && U && !!d_urec != !!d_rrec) return fail(KMX_E_ARG, "rrec is NULL exactly when urec is");
	if (d_rseq && n_links && !!d_link_hits != !!d_rlink_hits) return fail(KMX_E_ARG, "rlink_hits is NULL exactly when link_hits is");
	if (d_rseq && (rec_capacity >> 32)) return fail(KMX_E_ARG, "rec_capacity = %llu: at most 2^32 - 1", (unsigned long long)rec_capacity);
	const CtgSpan spans[] = {{d_useq, n_ubases, false}, {d_uoffsets, (U1 + 1) * 8, false}, {d_link_offsets, (2 * U1 + 1) * 8, false}, {d_links, n_links * 4, false}, {d_through, 16 * U1 * 8, false},
	                         {d_urec, d_urec ? U1 * sizeof(Unitig) : 0, false}, {d_link_hits, d_link_hits ? n_links * 8 : 0, false},
	                         {d_rseq, sc, true}, {d_roffsets, d_rseq ? (rc + 1) * 8 : 0, true}, {d_rrec, d_rrec ? rc * sizeof(Unitig) : 0, true}, {d_origin, rc * 4, true}, {d_rplace, up * 8, true},
	                         {d_rlink_offsets, d_rseq ? (2 * rc + 1) * 8 : 0, true}, {d_rlinks, nl * 4, true}, {d_link_origin, nl * 8, true}, {d_rlink_hits, d_rlink_hits ? nl * 8 : 0, true}};
	TRY(resolve_args(m, k, U, params, spans, 16, n_unitigs_out, n_bases_out, stats));
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!U) {
		if (d_rseq) {
			HIPCHK(hipMemsetAsync(d_roffsets, 0, 8, st));
			HIPCHK(hipMemsetAsync(d_rlink_offsets, 0, 8, st));
			HIPCHK(hipStreamSynchronize(st));
		}
		return KMX_OK;
	}
	ResDev D{};
	D.k = k; D.U = U; D.n_ubases = n_ubases; D.n_links = n_links;
	D.useq = (const unsigned char *)d_useq; D.uoffs = (const u64 *)d_uoffsets; D.urec = (const Unitig *)d_urec; D.loffs = (const u64 *)d_link_offsets; D.links = d_links; D.hits = (const u64 *)d_link_hits;
	D.through = (const u64 *)d_through; D.min_reads = params->min_reads; D.max_cross = params->max_cross;
	D.rseq = (unsigned char *)d_rseq; D.seq_cap = seq_capacity; D.rec_cap = rec_capacity; D.roffs = (u64 *)d_roffsets; D.rrec = (Unitig *)d_rrec; D.origin = d_origin; D.rplace = (ResPlace *)d_rplace;
	D.rloffs = (u64 *)d_rlink_offsets; D.rlinks = d_rlinks; D.lorigin = (u64 *)d_link_origin; D.rhits = (u64 *)d_rlink_hits;
	return resolve_core(m, D, n_unitigs_out, n_bases_out, stats);
}

static int kmx_unitig_resolve_impl(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets, uint64_t U, const kmx_unitig *urec, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links,
                                   const uint64_t *link_hits, const uint64_t *through, const kmx_resolve_params *params, char *rseq, uint64_t seq_capacity, uint64_t *roffsets, uint64_t rec_capacity,
                                   kmx_unitig *rrec, uint32_t *origin, kmx_resolve_place *rplace, uint64_t *rlink_offsets, uint32_t *rlinks, uint64_t *link_origin, uint64_t *rlink_hits,
                                   uint64_t *n_unitigs_out, uint64_t *n_bases_out, kmx_resolve_stats *stats)
{
	if (!uoffsets || !link_offsets) return fail(KMX_E_ARG, "null argument");
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: the resolution takes fewer than 2^31", (unsigned long long)U);
	if (k < 5 || k > 63 || !(k & 1)) return fail(KMX_E_ARG, "the resolution needs an odd k in [5, 63], not %d", k);
	if (rseq && U && !!urec != !!rrec) return fail(KMX_E_ARG, "rrec is NULL exactly when urec is");
	if (rseq && n_links && !!link_hits != !!rlink_hits) return fail(KMX_E_ARG, "rlink_hits is NULL exactly when link_hits is");
	if (rseq && (rec_capacity >> 32)) return fail(KMX_E_ARG, "rec_capacity = %llu: at most 2^32 - 1", (unsigned long long)rec_capacity);
	TRY(check_offsets(uoffsets, U));
	const u64 n_ubases = uoffsets[U];
	const u64 rc = rseq ? rec_capacity : 0, sc = rseq ? seq_capacity : 0, nl = rseq ? n_links : 0, up = rseq ? U : 0;
	const CtgSpan spans[] = {{useq, n_ubases, false}, {uoffsets, (U + 1) * 8, false}, {link_offsets, (2 * U + 1) * 8, false}, {links, n_links * 4, false}, {through, 16 * U * 8, false},
	                         {urec, urec ? U * sizeof(Unitig) : 0, false}, {link_hits, link_hits ? n_links * 8 : 0, false},
	                         {rseq, sc, true}, {roffsets, rseq ? (rc + 1) * 8 : 0, true}, {rrec, rrec ? rc * sizeof(Unitig) : 0, true}, {origin, rc * 4, true}, {rplace, up * 8, true},
	                         {rlink_offsets, rseq ? (2 * rc + 1) * 8 : 0, true}, {rlinks, nl * 4, true}, {link_origin, nl * 8, true}, {rlink_hits, rlink_hits ? nl * 8 : 0, true}};
	TRY(resolve_args(m, k, U, params, spans, 16, n_unitigs_out, n_bases_out, stats));
	for (u64 u = 0; u < U; u++)
		if (uoffsets[u + 1] - uoffsets[u] < (u64)k) return fail(KMX_E_ARG, "unitig %llu has %llu bytes, fewer than k = %d", (unsigned long long)u, (unsigned long long)(uoffsets[u + 1] - uoffsets[u]), k);
	TRY(check_offsets(link_offsets, 2 * U));
	if (link_offsets[2 * U] != n_links) return fail(KMX_E_ARG, "link_offsets end at %llu, not at n_links = %llu", (unsigned long long)link_offsets[2 * U], (unsigned long long)n_links);
	for (u64 o = 0; o < 2 * U; o++)
		if (link_offsets[o + 1] - link_offsets[o] > 4) return fail(KMX_E_ARG, "the row of oriented unitig %llu has %llu entries, more than 4", (unsigned long long)o, (unsigned long long)(link_offsets[o + 1] - link_offsets[o]));
	for (u64 e = 0; e < n_links; e++)
		if ((u64)links[e] >= 2 * U) return fail(KMX_E_ARG, "links[%llu] = %u is no oriented unitig of %llu", (unsigned long long)e, links[e], (unsigned long long)U);
	for (u64 a = 0; a < 2 * U; a++)
		for (u64 e = link_offsets[a]; e < link_offsets[a + 1]; e++) {
			const u64 b1 = (u64)links[e] ^ 1;
			bool found = false;
			for (u64 f = link_offsets[b1]; f < link_offsets[b1 + 1]; f++) found = found || links[f] == (u32)(a ^ 1);
			if (!found) return fail(KMX_E_ARG, "the edge %llu -> %u has no mirror %llu -> %llu", (unsigned long long)a, links[e], (unsigned long long)b1, (unsigned long long)(a ^ 1));
		}
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!U) {
		if (rseq) roffsets[0] = rlink_offsets[0] = 0;
		return KMX_OK;
	}
	struct Staged {                                                // the call's own device buffers; the stream is drained before they go
		kmx_model *m;
		DevBuf<unsigned char> useq, rseq;
		DevBuf<u64> uoffs, loffs, hits, through, roffs, rloffs, lorigin, rhits;
		DevBuf<u32> links, origin, rlinks;
		DevBuf<Unitig> urec, rrec;
		DevBuf<ResPlace> rplace;
		~Staged() { (void)hipStreamSynchronize(m->stream); }
	} G{m};
	if (G.useq.alloc(n_ubases) != hipSuccess || G.uoffs.alloc(U + 1) != hipSuccess || G.loffs.alloc(2 * U + 1) != hipSuccess || G.links.alloc(n_links) != hipSuccess || G.through.alloc(16 * U) != hipSuccess ||
	    (urec && G.urec.alloc(U) != hipSuccess) || (link_hits && G.hits.alloc(n_links) != hipSuccess))
		return res_nomem();
	HIPCHK(hipMemcpyAsync(G.useq, useq, n_ubases, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.uoffs, uoffsets, (U + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.loffs, link_offsets, (2 * U + 1) * 8, hipMemcpyHostToDevice, st));
	if (n_links) HIPCHK(hipMemcpyAsync(G.links, links, n_links * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.through, through, 16 * U * 8, hipMemcpyHostToDevice, st));
	if (urec) HIPCHK(hipMemcpyAsync(G.urec, urec, U * sizeof(Unitig), hipMemcpyHostToDevice, st));
	if (link_hits && n_links) HIPCHK(hipMemcpyAsync(G.hits, link_hits, n_links * 8, hipMemcpyHostToDevice, st));
	ResDev D{};
	D.k = k; D.U = U; D.n_ubases = n_ubases; D.n_links = n_links;
	D.useq = G.useq; D.uoffs = G.uoffs; D.urec = urec ? G.urec.get() : nullptr; D.loffs = G.loffs; D.links = G.links; D.hits = link_hits ? G.hits.get() : nullptr;
	D.through = G.through; D.min_reads = params->min_reads; D.max_cross = params->max_cross;
	if (!rseq) return resolve_core(m, D, n_unitigs_out, n_bases_out, stats);   // the sizing call
	// the output is staged at what 4 U and 4 n_ubases bound, never beyond the caller's capacities
	const u64 rcap = std::min<u64>(rec_capacity, 4 * U), scap = std::min<u64>(seq_capacity, 4 * n_ubases);
	if (G.rseq.alloc(scap) != hipSuccess || G.roffs.alloc(rcap + 1) != hipSuccess || G.rloffs.alloc(2 * rcap + 1) != hipSuccess || G.lorigin.alloc(n_links) != hipSuccess ||
	    (link_hits && G.rhits.alloc(n_links) != hipSuccess) || G.origin.alloc(rcap) != hipSuccess || G.rlinks.alloc(n_links) != hipSuccess || (urec && G.rrec.alloc(rcap) != hipSuccess) ||
	    G.rplace.alloc(U) != hipSuccess)
		return res_nomem();
	D.rseq = G.rseq; D.seq_cap = scap; D.rec_cap = rcap; D.roffs = G.roffs; D.rrec = urec ? G.rrec.get() : nullptr; D.origin = G.origin; D.rplace = G.rplace;
	D.rloffs = G.rloffs; D.rlinks = G.rlinks; D.lorigin = G.lorigin; D.rhits = link_hits ? G.rhits.get() : nullptr;
	TRY(resolve_core(m, D, n_unitigs_out, n_bases_out, stats));
	const u64 N = *n_unitigs_out, B = *n_bases_out;
	if (B) HIPCHK(hipMemcpyAsync(rseq, G.rseq, B, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(roffsets, G.roffs, (N + 1) * 8, hipMemcpyDeviceToHost, st));
	if (urec) HIPCHK(hipMemcpyAsync(rrec, G.rrec, N * sizeof(Unitig), hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(origin, G.origin, N * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(rplace, G.rplace, U * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(rlink_offsets, G.rloffs, (2 * N + 1) * 8, hipMemcpyDeviceToHost, st));
	if (n_links) HIPCHK(hipMemcpyAsync(rlinks, G.rlinks, n_links * 4, hipMemcpyDeviceToHost, st));
	if (n_links) HIPCHK(hipMemcpyAsync(link_origin, G.lorigin, n_links * 8, hipMemcpyDeviceToHost, st));
	if (n_links && link_hits) HIPCHK(hipMemcpyAsync(rlink_hits, G.rhits, n_links * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

static int kmx_unitig_resolve_last_phases_impl(kmx_model *m, double *seconds)
{
	if (!m || !seconds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 4; i++) seconds[i] = m->res.phase_s[i];
	return KMX_OK;
}
