// resolve_host.h -- kmx_unitig_walk_through[_dev]: the through hits of a batch's walks (the rule: include/kmx.h; the kernels:
// resolve_kernels.h; the launcher: unitig_device.hip).  Included into kmx_api.hip after contig_host.h.
//
// through_core runs the count on device buffers: the marks and the three counters stay on the handle by capacity
// (kmx_model::res), everything is enqueued on the model's stream, and ONE wait brings the counters to the host.  The _dev form
// checks what can be checked without reading a buffer and hands the caller's pointers over; the host form validates the walks and
// the CSR, stages its input and a zeroed through of its own for the length of the call, downloads it and adds.  Both calls of this
// file take their arguments as a struct (ThroughArgs, ResArgs) that one *_args function checks for both forms; the checks of k,
// offsets, unitig lengths, CSR and buffers, the staging owner (Staging) and the phase clock are shared: graph_host.h.
static_assert(sizeof(kmx_through_stats) == 64, "kmx_through_stats is 64 bytes");

static const char *const kThrWhat = "the through hits";
static int thr_nomem() { return graph_nomem(kThrWhat); }

// the buffers of one call: what both forms check before anything runs
struct ThroughArgs {
	const kmx_walk *walks; u64 n_walks;
	const uint32_t *steps; u64 n_steps;
	const uint64_t *loffs; const uint32_t *links; u64 n_links, U;
	uint64_t *through;
	kmx_through_stats *stats;
};

static int through_args(kmx_model *m, const ThroughArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!A.stats || !A.loffs || (A.n_walks && !A.walks) || (A.n_steps && !A.steps) || (A.n_links && !A.links) || (A.U && !A.through)) return fail(KMX_E_ARG, "null argument");
	TRY(check_unitig_count(A.U));
	*A.stats = kmx_through_stats{A.n_walks, A.n_steps, 0, 0, 0, {0, 0, 0}};
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

static ThroughDev through_dev_of(const ThroughArgs &A)
{
	ThroughDev D{};
	D.n_walks = A.n_walks; D.n_steps = A.n_steps; D.n_links = A.n_links; D.U = A.U;
	return D;
}

static int kmx_unitig_walk_through_dev_impl(kmx_model *m, const ThroughArgs &A)
{
	TRY(through_args(m, A));
	if (!A.n_steps || !A.U) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	ThroughDev D = through_dev_of(A);
	D.walks = (const Walk *)A.walks; D.steps = A.steps; D.loffs = (const u64 *)A.loffs; D.links = A.links; D.through = (unsigned long long *)A.through;
	return through_core(m, D, A.stats);
}

static int kmx_unitig_walk_through_impl(kmx_model *m, const ThroughArgs &A)
{
	TRY(through_args(m, A));
	u64 at = 0;
	for (u64 w = 0; w < A.n_walks; w++) {
		if (A.walks[w].first_step != at) return fail(KMX_E_ARG, "walk %llu starts at step %llu, not at %llu", (unsigned long long)w, (unsigned long long)A.walks[w].first_step, (unsigned long long)at);
		at += A.walks[w].n_steps;
	}
	if (at != A.n_steps) return fail(KMX_E_ARG, "the walks hold %llu steps, not n_steps = %llu", (unsigned long long)at, (unsigned long long)A.n_steps);
	TRY(check_link_csr(A.loffs, A.links, A.n_links, A.U, false));
	if (!A.n_steps || !A.U) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	Staging G(m, kThrWhat);
	ThroughDev D = through_dev_of(A);
	D.walks = G.in<Walk>(A.walks, A.n_walks); D.steps = G.in<u32>(A.steps, A.n_steps); D.links = G.in<u32>(A.links, A.n_links); D.loffs = G.in<u64>(A.loffs, 2 * A.U + 1);
	D.through = G.zeroed<unsigned long long>(16 * A.U);
	TRY(G.status());
	TRY(through_core(m, D, A.stats));
	G.down_add(A.through, D.through, 16 * A.U);
	return G.finish();
}

// ---- kmx_unitig_resolve[_dev]: the graph with every resolved unitig split into one copy per way in.  resolve_core runs the
// transform on device buffers: the unmirrored edges, the verdicts and their scan, ONE wait for the two counts and the counters,
// the check of the capacities, then records, links and the bytes.  The work arrays stay on the handle by capacity.
static_assert(sizeof(kmx_resolve_params) == 16 && sizeof(kmx_resolve_place) == 8 && sizeof(ResPlace) == 8 && sizeof(kmx_resolve_stats) == 64,
              "kmx_resolve_params is 16 bytes, kmx_resolve_place 8, kmx_resolve_stats 64");

static const char *const kResWhat = "the resolution";
static int res_nomem() { return graph_nomem(kResWhat); }

// the buffers of one call (n_ubases: the host form fills it in from uoffsets; rseq == null: the sizing call): what both forms
// check before anything runs
struct ResArgs {
	int k;
	const char *useq; const uint64_t *uoffs; u64 U, n_ubases; const kmx_unitig *urec;
	const uint64_t *loffs; const uint32_t *links; u64 n_links; const uint64_t *hits, *through;
	const kmx_resolve_params *params;
	char *rseq; u64 seq_cap; uint64_t *roffs; u64 rec_cap; kmx_unitig *rrec; uint32_t *origin; kmx_resolve_place *rplace;
	uint64_t *rloffs; uint32_t *rlinks; uint64_t *lorigin, *rhits;
	uint64_t *n_out, *n_bases_out;
	kmx_resolve_stats *stats;
};

static int resolve_args(kmx_model *m, const ResArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	if (!A.params || !A.n_out || !A.n_bases_out || !A.stats) return fail(KMX_E_ARG, "null argument");
	if (A.rseq && A.U && !!A.urec != !!A.rrec) return fail(KMX_E_ARG, "rrec is NULL exactly when urec is");
	if (A.rseq && A.n_links && !!A.hits != !!A.rhits) return fail(KMX_E_ARG, "rlink_hits is NULL exactly when link_hits is");
	if (A.rseq && (A.rec_cap >> 32)) return fail(KMX_E_ARG, "rec_capacity = %llu: at most 2^32 - 1", (unsigned long long)A.rec_cap);
	const u64 U = A.U, rc = A.rseq ? A.rec_cap : 0, nl = A.rseq ? A.n_links : 0;   // the sizing call takes no output buffer
	const Span spans[] = {{A.useq, A.n_ubases, false}, {A.uoffs, (U + 1) * 8, false}, {A.loffs, (2 * U + 1) * 8, false}, {A.links, A.n_links * 4, false}, {A.through, 16 * U * 8, false},
	                      opt_span(A.urec, U * sizeof(Unitig), false), opt_span(A.hits, A.n_links * 8, false),
	                      {A.rseq, A.rseq ? A.seq_cap : 0, true}, {A.roffs, A.rseq ? (rc + 1) * 8 : 0, true}, opt_span(A.rrec, rc * sizeof(Unitig), true), {A.origin, rc * 4, true},
	                      {A.rplace, A.rseq ? U * 8 : 0, true}, {A.rloffs, A.rseq ? (2 * rc + 1) * 8 : 0, true}, {A.rlinks, nl * 4, true}, {A.lorigin, nl * 8, true}, opt_span(A.rhits, nl * 8, true)};
	TRY(check_spans(spans, 16));
	*A.n_out = *A.n_bases_out = 0;
	*A.stats = kmx_resolve_stats{0, 0, 0, 0, 0, 0, 0, 0};
	return KMX_OK;
}

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
	PhaseClock clk(m, S.phase_s);
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

// the sizes and parameters of the kernel block; the pointers and the capacities are the form's own
static ResDev resolve_dev_of(const ResArgs &A)
{
	ResDev D{};
	D.k = A.k; D.U = A.U; D.n_ubases = A.n_ubases; D.n_links = A.n_links;
	D.min_reads = A.params->min_reads; D.max_cross = A.params->max_cross;
	return D;
}

static int kmx_unitig_resolve_dev_impl(kmx_model *m, const ResArgs &A)
{
	TRY(resolve_args(m, A));
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!A.U) {
		if (A.rseq) {
			HIPCHK(hipMemsetAsync(A.roffs, 0, 8, st));
			HIPCHK(hipMemsetAsync(A.rloffs, 0, 8, st));
			HIPCHK(hipStreamSynchronize(st));
		}
		return KMX_OK;
	}
	ResDev D = resolve_dev_of(A);
	D.useq = (const unsigned char *)A.useq; D.uoffs = (const u64 *)A.uoffs; D.urec = (const Unitig *)A.urec; D.loffs = (const u64 *)A.loffs; D.links = A.links; D.hits = (const u64 *)A.hits;
	D.through = (const u64 *)A.through;
	D.rseq = (unsigned char *)A.rseq; D.seq_cap = A.seq_cap; D.rec_cap = A.rec_cap; D.roffs = (u64 *)A.roffs; D.rrec = (Unitig *)A.rrec; D.origin = A.origin; D.rplace = (ResPlace *)A.rplace;
	D.rloffs = (u64 *)A.rloffs; D.rlinks = A.rlinks; D.lorigin = (u64 *)A.lorigin; D.rhits = (u64 *)A.rhits;
	return resolve_core(m, D, A.n_out, A.n_bases_out, A.stats);
}

static int kmx_unitig_resolve_impl(kmx_model *m, ResArgs A)
{
	TRY(check_unitig_count(A.U));
	TRY(check_offsets(A.uoffs, A.U));
	A.n_ubases = A.uoffs[A.U];
	TRY(resolve_args(m, A));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_link_csr(A.loffs, A.links, A.n_links, A.U, true));
	HIPCHK(hipSetDevice(m->device));
	const u64 U = A.U, n_ubases = A.n_ubases, n_links = A.n_links;
	if (!U) {
		if (A.rseq) A.roffs[0] = A.rloffs[0] = 0;
		return KMX_OK;
	}
	Staging G(m, kResWhat);
	ResDev D = resolve_dev_of(A);
	D.useq = G.in<unsigned char>(A.useq, n_ubases); D.uoffs = G.in<u64>(A.uoffs, U + 1); D.loffs = G.in<u64>(A.loffs, 2 * U + 1); D.links = G.in<u32>(A.links, n_links);
	D.through = G.in<u64>(A.through, 16 * U); D.urec = A.urec ? G.in<Unitig>(A.urec, U) : nullptr; D.hits = A.hits ? G.in<u64>(A.hits, n_links) : nullptr;
	TRY(G.status());
	if (!A.rseq) return resolve_core(m, D, A.n_out, A.n_bases_out, A.stats);   // the sizing call: the inputs only
	// the output is staged at what 4 U and 4 n_ubases bound, never beyond the caller's capacities
	D.rec_cap = std::min<u64>(A.rec_cap, 4 * U); D.seq_cap = std::min<u64>(A.seq_cap, 4 * n_ubases);
	D.rseq = G.out<unsigned char>(D.seq_cap); D.roffs = G.out<u64>(D.rec_cap + 1); D.rloffs = G.out<u64>(2 * D.rec_cap + 1); D.lorigin = G.out<u64>(n_links);
	D.rhits = A.hits ? G.out<u64>(n_links) : nullptr; D.origin = G.out<u32>(D.rec_cap); D.rlinks = G.out<u32>(n_links); D.rrec = A.urec ? G.out<Unitig>(D.rec_cap) : nullptr;
	D.rplace = G.out<ResPlace>(U);
	TRY(G.status());
	TRY(resolve_core(m, D, A.n_out, A.n_bases_out, A.stats));
	const u64 N = *A.n_out;
	G.down(A.rseq, D.rseq, *A.n_bases_out);
	G.down(A.roffs, D.roffs, N + 1);
	if (A.urec) G.down(A.rrec, D.rrec, N);
	G.down(A.origin, D.origin, N);
	G.down(A.rplace, D.rplace, U);
	G.down(A.rloffs, D.rloffs, 2 * N + 1);
	G.down(A.rlinks, D.rlinks, n_links);
	G.down(A.lorigin, D.lorigin, n_links);
	if (A.hits) G.down(A.rhits, D.rhits, n_links);
	return G.finish();
}

static int kmx_unitig_resolve_last_phases_impl(kmx_model *m, double *seconds)
{
	if (!m || !seconds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 4; i++) seconds[i] = m->res.phase_s[i];
	return KMX_OK;
}
