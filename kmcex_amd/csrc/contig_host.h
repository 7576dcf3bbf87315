// contig_host.h -- kmx_unitig_contigs[_dev]: contigs from the read-supported edges between unitigs (the rule: include/kmx.h; the
// kernels: contig_kernels.h; the launchers: unitig_device.hip).  Included into kmx_api.hip after map_host.h.
//
// contig_core runs the construction on device buffers: supports and verdicts, the chain links, the ranking of the 2 U oriented
// unitigs by pointer doubling (one stream wait per round: a word says whether anything moved), the cut of what is left on
// cycles and its ranking, the marks and their scan, then records, steps, places, the bytes and the contig graph, and ONE wait for
// the totals and the counters.  The work arrays stay on the handle by capacity (kmx_model::ctg).  The _dev form checks what
// can be checked without reading a buffer and hands the caller's pointers over; the host form validates offsets and CSR, stages
// input and output in buffers of its own for the length of the call, and downloads.
static_assert(sizeof(kmx_contig) == 64 && sizeof(Contig) == 64 && sizeof(kmx_contig_place) == 8 && sizeof(CtgPlace) == 8 && sizeof(kmx_contig_stats) == 64 && sizeof(kmx_contig_params) == 16,
              "kmx_contig is 64 bytes, kmx_contig_place 8, kmx_contig_stats 64, kmx_contig_params 16");
static_assert(offsetof(kmx_contig, min_count) == offsetof(Contig, min_count) && offsetof(kmx_contig, first_step) == offsetof(Contig, first_step) && offsetof(kmx_contig, n_steps) == offsetof(Contig, n_steps) &&
              offsetof(kmx_contig, circular) == offsetof(Contig, circular) && offsetof(kmx_contig, min_support) == offsetof(Contig, min_support) && offsetof(kmx_contig, reserved2) == offsetof(Contig, reserved2),
              "Contig (kmx_types.h) is the layout of kmx_contig");
static_assert(sizeof(CtgRank) == 16 && sizeof(CtgTot) == 24, "the rank state is 16 bytes per oriented unitig, a mark 24 per unitig");

static int ctg_nomem() { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of the contig construction could not be allocated"); }

// [a, a + na) and [b, b + nb) share a byte
static bool ctg_overlap(const void *a, u64 na, const void *b, u64 nb)
{
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	return a && b && na && nb && x < y + nb && y < x + na;
}

struct CtgSpan {
	const void *p;
	u64 bytes;
	bool out;
};

// what both forms check before anything runs
static int contig_args(kmx_model *m, int k, u64 U, const kmx_contig_params *p, const CtgSpan *spans, int n_spans, uint64_t *n_contigs, uint64_t *n_cbases, uint64_t *n_clinks, kmx_contig_stats *stats)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (k < 5 || k > 63 || !(k & 1)) return fail(KMX_E_ARG, "contigs need an odd k in [5, 63], not %d", k);
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: contigs take fewer than 2^31", (unsigned long long)U);
	if (!p || !n_contigs || !n_cbases || !n_clinks || !stats) return fail(KMX_E_ARG, "null argument");
	if (p->ratio > 65536) return fail(KMX_E_ARG, "ratio = %u: at most 65536", p->ratio);
	if (p->reserved) return fail(KMX_E_ARG, "kmx_contig_params.reserved is not 0");
	for (int i = 0; i < n_spans; i++)                              // a buffer of no element may be null; the offset arrays always hold one
		if (!spans[i].p && spans[i].bytes) return fail(KMX_E_ARG, "null argument (buffer %d of the call)", i);
	for (int i = 0; i < n_spans; i++)
		for (int j = i + 1; j < n_spans; j++)
			if ((spans[i].out || spans[j].out) && ctg_overlap(spans[i].p, spans[i].bytes, spans[j].p, spans[j].bytes))
				return fail(KMX_E_ARG, "an output buffer overlaps another buffer of the call (buffers %d and %d)", i, j);
	*n_contigs = *n_cbases = *n_clinks = 0;
	*stats = kmx_contig_stats{0, 0, 0, 0, 0, 0, 0, 0};
	return KMX_OK;
}

// a lap of the phase clock, only under kmx_set_profile(m, 1), where every phase waits for the stream
struct CtgClock {
	kmx_model *m;
	std::chrono::steady_clock::time_point t0;
	explicit CtgClock(kmx_model *mm) : m(mm) { if (m->prof.on) { hipStreamSynchronize(m->stream); t0 = std::chrono::steady_clock::now(); } }
	void lap(int phase)
	{
		if (!m->prof.on) return;
		hipStreamSynchronize(m->stream);
		const auto t1 = std::chrono::steady_clock::now();
		m->ctg.phase_s[phase] += std::chrono::duration<double>(t1 - t0).count();
		t0 = t1;
	}
};

// the construction on device buffers (D: input, parameters and output; the work arrays are filled in here); D.U > 0
static int contig_core(kmx_model *m, CtgDev D, uint64_t *n_contigs, uint64_t *n_cbases, uint64_t *n_clinks, kmx_contig_stats *stats)
{
	auto &S = m->ctg;
	const hipStream_t st = m->stream;
	const u64 U = D.U, nl = D.n_links;
	int lg = 0;
	while ((u64(1) << lg) < 2 * U) lg++;                           // ceil(log2 2U)
	const int T = lg + 1;
	for (double &s : S.phase_s) s = 0;
	S.rounds = 0;
	if (S.d_esup.ensure(nl, st) != hipSuccess || S.d_ekeep.ensure(nl, st) != hipSuccess || S.d_best.ensure(2 * U, st) != hipSuccess || S.d_nk.ensure(2 * U, st) != hipSuccess ||
	    S.d_only.ensure(2 * U, st) != hipSuccess || S.d_supo.ensure(2 * U, st) != hipSuccess || S.d_circ.ensure(U, st) != hipSuccess || S.d_rank[0].ensure(2 * U + 2, st) != hipSuccess ||
	    S.d_rank[1].ensure(2 * U + 2, st) != hipSuccess || S.d_mn.ensure(4 * U, st) != hipSuccess || S.d_sc.ensure(U + 1, st) != hipSuccess || S.d_ubase.ensure(U, st) != hipSuccess ||
	    S.d_clc.ensure(4 * U + 2, st) != hipSuccess || S.d_last.ensure(2 * U, st) != hipSuccess || S.d_cnt.ensure(CTG_C_N, st) != hipSuccess || S.d_flag.ensure(2 * (size_t)T + 2, st) != hipSuccess)
		return ctg_nomem();
	D.esup = S.d_esup; D.ekeep = S.d_ekeep; D.best = S.d_best; D.nk = S.d_nk; D.only = S.d_only; D.supo = S.d_supo; D.circ = S.d_circ;
	D.sc = S.d_sc; D.ubase = S.d_ubase; D.clc = S.d_clc; D.clsc = S.d_clc.get() + 2 * U + 1; D.last = S.d_last; D.cnt = S.d_cnt;
	HIPCHK(hipMemsetAsync(S.d_flag, 0, (2 * (size_t)T + 2) * 4, st));
	HIPCHK(hipMemsetAsync(S.d_cnt, 0, CTG_C_N * sizeof(unsigned long long), st));
	HIPCHK(hipMemsetAsync(S.d_circ, 0, U, st));
	auto word = [&](int i, u32 *v) {                               // one stream wait
		HIPCHK(hipMemcpyAsync(v, S.d_flag.get() + i, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		return (int)KMX_OK;
	};
	CtgClock clk(m);
	u32 *mn[2] = {S.d_mn.get(), S.d_mn.get() + 2 * U};
	kmxk::contig_links(D, S.d_rank[0], mn[0], st);
	clk.lap(0);
	int c = 0;
	bool cycles = false;
	for (int t = 1; t <= T; t++) {
		kmxk::contig_round(S.d_rank[c], mn[c], S.d_rank[c ^ 1], mn[c ^ 1], U, S.d_flag.get() + t, st);
		c ^= 1;
		S.rounds++;
		u32 moved = 0;
		TRY(word(t, &moved));
		if (!moved) break;
		cycles = t == T;                                           // every path has settled by now: what still moves goes round
	}
	if (cycles) {
		kmxk::contig_cut(D, S.d_rank[c], mn[c], S.d_rank[c ^ 1], st);
		c ^= 1;
		u32 moved = 1;
		for (int t = 1; t <= T && moved; t++) {
			kmxk::contig_round(S.d_rank[c], nullptr, S.d_rank[c ^ 1], nullptr, U, S.d_flag.get() + T + t, st);
			c ^= 1;
			S.rounds++;
			TRY(word(T + t, &moved));
		}
		if (moved) return fail(KMX_E_ARG, "internal error: the cut cycles did not settle");
	}
	clk.lap(1);
	hipError_t e = kmxk::contig_mark(D, S.d_rank[c], (CtgTot *)S.d_rank[c ^ 1].get(), S.d_tmp, st);   // the marks: 24 (U + 1) bytes in the spare copy's 16 (2 U + 2)
	if (e == hipErrorOutOfMemory) return ctg_nomem();
	HIPCHK(e);
	clk.lap(2);
	e = kmxk::contig_place(D, S.d_rank[c], S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return ctg_nomem();
	HIPCHK(e);
	clk.lap(3);
	kmxk::contig_bytes(D, st);
	CtgTot tot{0, 0, 0};
	unsigned long long cn[CTG_C_N] = {0, 0, 0, 0, 0, 0, 0};
	u64 ncl = 0;
	HIPCHK(hipMemcpyAsync(&tot, D.sc + U, sizeof tot, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(cn, D.cnt, sizeof cn, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(&ncl, D.clsc + 2 * U, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the wait for the counts; nothing is left in flight
	HIPCHK(hipGetLastError());
	clk.lap(4);
	*n_contigs = tot.n;
	*n_cbases = tot.len;
	*n_clinks = ncl;
	*stats = kmx_contig_stats{cn[CTG_C_LINKS], cn[CTG_C_KEPT], cn[CTG_C_BELOW_MIN], cn[CTG_C_BELOW_RATIO], cn[CTG_C_CHAIN], tot.n, cn[CTG_C_CIRCULAR], cn[CTG_C_MULTI]};
	return KMX_OK;
}

static int kmx_unitig_contigs_dev_impl(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t U, uint64_t n_ubases, const kmx_unitig *d_urec, const uint64_t *d_link_offsets,
                                       const uint32_t *d_links, uint64_t n_links, const uint64_t *d_link_hits, const kmx_contig_params *params, char *d_cseq, uint64_t *d_coffsets, kmx_contig *d_crec,
                                       uint32_t *d_steps, kmx_contig_place *d_place, uint64_t *d_clink_offsets, uint32_t *d_clinks, uint64_t *d_csupport, uint64_t *n_contigs, uint64_t *n_cbases,
                                       uint64_t *n_clinks, kmx_contig_stats *stats)
{
	const u64 U1 = (U >> 31) ? 0 : U;                              // (sizes for the overlap check only; a U that large is refused first)
	const CtgSpan spans[] = {{d_useq, n_ubases, false}, {d_uoffsets, (U1 + 1) * 8, false}, {d_urec, U1 * sizeof(Unitig), false}, {d_link_offsets, (2 * U1 + 1) * 8, false}, {d_links, n_links * 4, false},
	                         {d_link_hits, n_links * 8, false}, {d_cseq, n_ubases, true}, {d_coffsets, (U1 + 1) * 8, true}, {d_crec, U1 * sizeof(Contig), true}, {d_steps, U1 * 4, true}, {d_place, U1 * 8, true},
	                         {d_clink_offsets, (2 * U1 + 1) * 8, true}, {d_clinks, n_links * 4, true}, {d_csupport, n_links * 8, true}};
	CtgSpan checked[14];
	for (int i = 0; i < 14; i++) checked[i] = spans[i];
	checked[2].bytes = d_urec ? checked[2].bytes : 0;              // urec may be NULL
	TRY(contig_args(m, k, U, params, checked, 14, n_contigs, n_cbases, n_clinks, stats));
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!U) {
		HIPCHK(hipMemsetAsync(d_coffsets, 0, 8, st));
		HIPCHK(hipMemsetAsync(d_clink_offsets, 0, 8, st));
		HIPCHK(hipStreamSynchronize(st));
		return KMX_OK;
	}
	CtgDev D{};
	D.k = k; D.U = U; D.n_ubases = n_ubases; D.n_links = n_links;
	D.useq = (const unsigned char *)d_useq; D.uoffs = (const u64 *)d_uoffsets; D.urec = (const Unitig *)d_urec; D.loffs = (const u64 *)d_link_offsets; D.links = d_links; D.hits = (const u64 *)d_link_hits;
	D.min_reads = params->min_reads; D.ratio = params->ratio;
	D.cseq = (unsigned char *)d_cseq; D.coffs = (u64 *)d_coffsets; D.crec = (Contig *)d_crec; D.steps = d_steps; D.place = (CtgPlace *)d_place; D.cloffs = (u64 *)d_clink_offsets; D.clinks = d_clinks;
	D.csup = (u64 *)d_csupport;
	return contig_core(m, D, n_contigs, n_cbases, n_clinks, stats);
}

static int kmx_unitig_contigs_impl(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets, uint64_t U, const kmx_unitig *urec, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links,
                                   const uint64_t *link_hits, const kmx_contig_params *params, char *cseq, uint64_t *coffsets, kmx_contig *crec, uint32_t *steps, kmx_contig_place *place,
                                   uint64_t *clink_offsets, uint32_t *clinks, uint64_t *csupport, uint64_t *n_contigs, uint64_t *n_cbases, uint64_t *n_clinks, kmx_contig_stats *stats)
{
	if (!uoffsets || !coffsets || !clink_offsets || !link_offsets) return fail(KMX_E_ARG, "null argument");
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: contigs take fewer than 2^31", (unsigned long long)U);
	if (k < 5 || k > 63 || !(k & 1)) return fail(KMX_E_ARG, "contigs need an odd k in [5, 63], not %d", k);
	TRY(check_offsets(uoffsets, U));
	const u64 n_ubases = uoffsets[U];
	const CtgSpan spans[] = {{useq, n_ubases, false}, {uoffsets, (U + 1) * 8, false}, {urec, urec ? U * sizeof(Unitig) : 0, false}, {link_offsets, (2 * U + 1) * 8, false}, {links, n_links * 4, false},
	                         {link_hits, n_links * 8, false}, {cseq, n_ubases, true}, {coffsets, (U + 1) * 8, true}, {crec, U * sizeof(Contig), true}, {steps, U * 4, true}, {place, U * 8, true},
	                         {clink_offsets, (2 * U + 1) * 8, true}, {clinks, n_links * 4, true}, {csupport, n_links * 8, true}};
	TRY(contig_args(m, k, U, params, spans, 14, n_contigs, n_cbases, n_clinks, stats));
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
		coffsets[0] = clink_offsets[0] = 0;
		return KMX_OK;
	}
	struct Staged {                                                // the call's own device buffers; the stream is drained before they go
		kmx_model *m;
		DevBuf<unsigned char> useq, cseq;
		DevBuf<u64> uoffs, loffs, hits, coffs, cloffs, csup;
		DevBuf<u32> links, steps, clinks;
		DevBuf<Unitig> urec;
		DevBuf<Contig> crec;
		DevBuf<CtgPlace> place;
		~Staged() { (void)hipStreamSynchronize(m->stream); }
	} G{m};
	if (G.useq.alloc(n_ubases) != hipSuccess || G.cseq.alloc(n_ubases) != hipSuccess || G.uoffs.alloc(U + 1) != hipSuccess || G.loffs.alloc(2 * U + 1) != hipSuccess || G.hits.alloc(n_links) != hipSuccess ||
	    G.coffs.alloc(U + 1) != hipSuccess || G.cloffs.alloc(2 * U + 1) != hipSuccess || G.csup.alloc(n_links) != hipSuccess || G.links.alloc(n_links) != hipSuccess || G.steps.alloc(U) != hipSuccess ||
	    G.clinks.alloc(n_links) != hipSuccess || (urec && G.urec.alloc(U) != hipSuccess) || G.crec.alloc(U) != hipSuccess || G.place.alloc(U) != hipSuccess)
		return ctg_nomem();
	HIPCHK(hipMemcpyAsync(G.useq, useq, n_ubases, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.uoffs, uoffsets, (U + 1) * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(G.loffs, link_offsets, (2 * U + 1) * 8, hipMemcpyHostToDevice, st));
	if (n_links) HIPCHK(hipMemcpyAsync(G.links, links, n_links * 4, hipMemcpyHostToDevice, st));
	if (n_links) HIPCHK(hipMemcpyAsync(G.hits, link_hits, n_links * 8, hipMemcpyHostToDevice, st));
	if (urec) HIPCHK(hipMemcpyAsync(G.urec, urec, U * sizeof(Unitig), hipMemcpyHostToDevice, st));
	CtgDev D{};
	D.k = k; D.U = U; D.n_ubases = n_ubases; D.n_links = n_links;
	D.useq = G.useq; D.uoffs = G.uoffs; D.urec = urec ? G.urec.get() : nullptr; D.loffs = G.loffs; D.links = G.links; D.hits = G.hits;
	D.min_reads = params->min_reads; D.ratio = params->ratio;
	D.cseq = G.cseq; D.coffs = G.coffs; D.crec = G.crec; D.steps = G.steps; D.place = G.place; D.cloffs = G.cloffs; D.clinks = G.clinks; D.csup = G.csup;
	TRY(contig_core(m, D, n_contigs, n_cbases, n_clinks, stats));
	const u64 C = *n_contigs, ncl = *n_clinks;
	if (C > U || *n_cbases > n_ubases || ncl > n_links) return fail(KMX_E_ARG, "internal error: the contigs exceed the input's sizes");
	if (*n_cbases) HIPCHK(hipMemcpyAsync(cseq, G.cseq, *n_cbases, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(coffsets, G.coffs, (C + 1) * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(crec, G.crec, C * sizeof(Contig), hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(steps, G.steps, U * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(place, G.place, U * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(clink_offsets, G.cloffs, (2 * C + 1) * 8, hipMemcpyDeviceToHost, st));
	if (ncl) HIPCHK(hipMemcpyAsync(clinks, G.clinks, ncl * 4, hipMemcpyDeviceToHost, st));
	if (ncl) HIPCHK(hipMemcpyAsync(csupport, G.csup, ncl * 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

static int kmx_unitig_contigs_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 5; i++) seconds[i] = m->ctg.phase_s[i];
	*rounds = m->ctg.rounds;
	return KMX_OK;
}
