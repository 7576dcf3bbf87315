// pair_path_host.h -- kmx_unitig_pair_paths[_dev]: the graph path every entry of a pair list stands for, credited to through and
// path_hits (the rule: include/kmx.h; the kernels: pair_path_kernels.h; the launchers: unitig_device.hip).  Included into
// kmx_api.hip after scaffold_host.h.
//
// pair_path_core runs the call on device buffers: the search, the scan of the PATH entries' steps, the additions, and ONE wait
// that brings the total and the counters to the host.  The steps are stored by the last launch only where they fit, so
// KMX_E_RANGE needs no second wait.  The work arrays stay on the handle by capacity (kmx_model::ppath).  The _dev form checks what
// can be checked without reading a buffer and hands the caller's pointers over; the host form validates offsets, CSR and the
// list's order, stages input and output in buffers of its own for the length of the call (through and path_hits zeroed, then
// added), and downloads.  The checks, the staging owner and the phase clock are shared: graph_host.h.
static_assert(sizeof(kmx_pair_path) == 32 && sizeof(PairPath) == 32 && sizeof(kmx_pair_path_params) == 32 && sizeof(kmx_pair_path_stats) == 80,
              "kmx_pair_path is 32 bytes, kmx_pair_path_params 32, kmx_pair_path_stats 80");
static_assert(offsetof(kmx_pair_path, n_steps) == offsetof(PairPath, n_steps) && offsetof(kmx_pair_path, first_step) == offsetof(PairPath, first_step) &&
              offsetof(kmx_pair_path, windows) == offsetof(PairPath, windows) && offsetof(kmx_pair_path, n_hits) == offsetof(PairPath, n_hits) &&
              offsetof(kmx_pair_path, n_visited) == offsetof(PairPath, n_visited) && offsetof(kmx_pair_path, n_visited) == 28,
              "PairPath (kmx_types.h) is the layout of kmx_pair_path");
static_assert(KMX_PATH_IGNORED == PP_IGNORED && KMX_PATH_BELOW_MIN == PP_BELOW_MIN && KMX_PATH_NO_PATH == PP_NO_PATH && KMX_PATH_ADJACENT == PP_ADJACENT && KMX_PATH_PATH == PP_PATH &&
              KMX_PATH_AMBIGUOUS == PP_AMBIGUOUS && KMX_PATH_COMPLEX == PP_COMPLEX && KMX_PATH_MAX_STEPS == PP_MAX_STEPS,
              "the verdicts of kmx_types.h are KMX_PATH_*");

static const char *const kPpWhat = "the pair paths";
static int pp_nomem() { return graph_nomem(kPpWhat); }
static int pp_range(u64 need, u64 cap) { return fail(KMX_E_RANGE, "%llu path steps, the buffer holds %llu", (unsigned long long)need, (unsigned long long)cap); }

// the buffers of one call: what both forms check before anything runs
struct PathArgs {
	int k;
	const uint64_t *uoffs; u64 U;
	const uint64_t *loffs; const uint32_t *links; u64 n_links;
	const kmx_pair_link *plinks; u64 n_plinks;
	const kmx_pair_path_params *params;
	kmx_pair_path *precs; uint32_t *psteps; u64 cap; uint64_t *n_psteps;
	uint64_t *through, *path_hits;
	kmx_pair_path_stats *stats;
};

static int pair_path_args(kmx_model *m, const PathArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	if (A.n_plinks >> 31) return fail(KMX_E_ARG, "%llu pair links: a path call takes fewer than 2^31", (unsigned long long)A.n_plinks);
	const kmx_pair_path_params *p = A.params;
	if (!p || !A.stats || (A.psteps && !A.n_psteps)) return fail(KMX_E_ARG, "null argument");
	if (p->max_steps < 1 || p->max_steps > KMX_PATH_MAX_STEPS) return fail(KMX_E_ARG, "max_steps = %u: in [1, %d]", p->max_steps, KMX_PATH_MAX_STEPS);
	if (p->max_visits < 1 || p->max_visits > 65536) return fail(KMX_E_ARG, "max_visits = %u: in [1, 65536]", p->max_visits);
	if (p->reserved) return fail(KMX_E_ARG, "kmx_pair_path_params.reserved is not 0");
	const u64 U = A.U;
	const Span spans[] = {{A.uoffs, (U + 1) * 8, false}, {A.loffs, (2 * U + 1) * 8, false}, {A.links, A.n_links * 4, false}, {A.plinks, A.n_plinks * sizeof(PairLink), false},
	                      {A.precs, A.n_plinks * sizeof(PairPath), true}, opt_span(A.psteps, A.cap * 4, true), opt_span(A.through, 16 * U * 8, true), opt_span(A.path_hits, A.n_links * 8, true)};
	TRY(check_spans(spans, 8));
	if (A.n_psteps) *A.n_psteps = 0;
	*A.stats = kmx_pair_path_stats{A.n_plinks, U ? 0 : A.n_plinks, 0, 0, 0, 0, 0, 0, 0, 0};   // without a unitig no entry is a pair link
	return KMX_OK;
}

// the call on device buffers (D: input, parameters and output; the work arrays are filled in here); D.U > 0 and D.n_plinks > 0.
// KMX_E_RANGE when the steps do not fit D.cap: everything but them is complete
static int pair_path_core(kmx_model *m, PathDev D, uint64_t *n_psteps, kmx_pair_path_stats *stats)
{
	auto &S = m->ppath;
	const hipStream_t st = m->stream;
	for (double &s : S.phase_s) s = 0;
	if (S.d_work.ensure(D.n_plinks * D.max_steps, st) != hipSuccess || S.d_sc.ensure(D.n_plinks + 1, st) != hipSuccess || S.d_cnt.ensure(PP_C_N, st) != hipSuccess) return pp_nomem();
	D.work = S.d_work; D.sc = S.d_sc; D.cnt = S.d_cnt;
	PhaseClock clk(m, S.phase_s);
	HIPCHK(kmxk::pair_path_search(D, st));
	clk.lap(0);
	const hipError_t e = kmxk::pair_path_scan(D, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return pp_nomem();
	HIPCHK(e);
	clk.lap(1);
	HIPCHK(kmxk::pair_path_apply(D, st));
	u64 total = 0;
	unsigned long long c[PP_C_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&total, D.sc + D.n_plinks, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait: the total and the counters
	HIPCHK(hipGetLastError());
	clk.lap(2);
	if (n_psteps) *n_psteps = total;
	*stats = kmx_pair_path_stats{D.n_plinks, c[PP_IGNORED], c[PP_BELOW_MIN], c[PP_NO_PATH], c[PP_ADJACENT], c[PP_PATH], c[PP_AMBIGUOUS], c[PP_COMPLEX], c[PP_C_ADDED], c[PP_C_MISSING]};
	if (D.psteps && total > D.cap) return pp_range(total, D.cap);
	return KMX_OK;
}

// the sizes and parameters of the kernel block; the pointers are the form's own
static PathDev pair_path_dev_of(const PathArgs &A)
{
	PathDev D{};
	D.k = A.k; D.U = A.U; D.n_links = A.n_links; D.n_plinks = A.n_plinks; D.cap = A.cap;
	D.min_pairs = A.params->min_pairs; D.inner = A.params->inner; D.tol = A.params->tol; D.max_steps = A.params->max_steps; D.max_visits = A.params->max_visits;
	return D;
}

static int kmx_unitig_pair_paths_dev_impl(kmx_model *m, const PathArgs &A)
{
	TRY(pair_path_args(m, A));
	if (!A.n_plinks) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	if (!A.U) {                                                    // every entry is ignored
		HIPCHK(hipMemsetAsync(A.precs, 0, A.n_plinks * sizeof(PairPath), m->stream));
		HIPCHK(hipStreamSynchronize(m->stream));
		return KMX_OK;
	}
	PathDev D = pair_path_dev_of(A);
	D.uoffs = (const u64 *)A.uoffs; D.loffs = (const u64 *)A.loffs; D.links = A.links; D.plinks = (const PairLink *)A.plinks;
	D.precs = (PairPath *)A.precs; D.psteps = A.psteps; D.through = (unsigned long long *)A.through; D.path_hits = (unsigned long long *)A.path_hits;
	return pair_path_core(m, D, A.n_psteps, A.stats);
}

static int kmx_unitig_pair_paths_impl(kmx_model *m, const PathArgs &A)
{
	TRY(check_unitig_count(A.U));
	TRY(pair_path_args(m, A));
	TRY(check_offsets(A.uoffs, A.U));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_link_csr(A.loffs, A.links, A.n_links, A.U, false));
	TRY(check_pair_list(A.plinks, A.n_plinks));
	const u64 U = A.U, np = A.n_plinks;
	if (!np) return KMX_OK;
	if (!U) {
		memset(A.precs, 0, np * sizeof(PairPath));
		return KMX_OK;
	}
	HIPCHK(hipSetDevice(m->device));
	Staging G(m, kPpWhat);
	PathDev D = pair_path_dev_of(A);
	D.cap = std::min<u64>(A.cap, np * A.params->max_steps);        // the steps are staged at what always suffices, never beyond the caller's capacity
	D.uoffs = G.in<u64>(A.uoffs, U + 1); D.loffs = G.in<u64>(A.loffs, 2 * U + 1); D.links = G.in<u32>(A.links, A.n_links); D.plinks = G.in<PairLink>(A.plinks, np);
	D.precs = G.out<PairPath>(np); D.psteps = A.psteps ? G.out<u32>(D.cap) : nullptr;
	D.through = A.through ? G.zeroed<unsigned long long>(16 * U) : nullptr; D.path_hits = A.path_hits ? G.zeroed<unsigned long long>(A.n_links) : nullptr;
	TRY(G.status());
	const int rc = pair_path_core(m, D, A.n_psteps, A.stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	G.down(A.precs, D.precs, np);
	if (A.psteps) G.down(A.psteps, D.psteps, std::min<u64>(*A.n_psteps, D.cap));
	if (A.through) G.down_add(A.through, D.through, 16 * U);
	if (A.path_hits) G.down_add(A.path_hits, D.path_hits, A.n_links);
	TRY(G.finish());
	return rc == KMX_OK ? KMX_OK : pp_range(*A.n_psteps, A.cap);
}

static int kmx_unitig_pair_paths_last_phases_impl(kmx_model *m, double *seconds)
{
	if (!m || !seconds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 3; i++) seconds[i] = m->ppath.phase_s[i];
	return KMX_OK;
}
