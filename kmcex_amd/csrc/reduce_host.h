// reduce_host.h -- kmx_unitig_pair_reduce[_dev]: a pair list without the entries that skip a unitig (the rule: include/kmx.h; the
// kernels: reduce_kernels.h; the launchers: unitig_device.hip).  Included into kmx_api.hip after fill_host.h.
//
// reduce_core runs the call on device buffers: the rows and their sort, the verdicts with the keep flags, the scan of the flags,
// and ONE wait that brings n_out and the counters to the host.  Only when that wait has shown that the list fits are the entries
// that stay written; a last wait leaves nothing in flight.  The work arrays stay on the handle by capacity (kmx_model::red).
// The _dev form checks what can be checked without reading a buffer and hands the caller's pointers over; the host form
// validates offsets and the list's order, stages input and output in buffers of its own for the length of the call, and
// downloads.  The checks, the staging owner and the phase clock are shared: graph_host.h.
static_assert(sizeof(kmx_pair_reduce) == 32 && sizeof(PairReduce) == 32 && sizeof(kmx_pair_reduce_params) == 24 && sizeof(kmx_pair_reduce_stats) == 80,
              "kmx_pair_reduce is 32 bytes, kmx_pair_reduce_params 24, kmx_pair_reduce_stats 80");
static_assert(offsetof(kmx_pair_reduce, via) == offsetof(PairReduce, via) && offsetof(kmx_pair_reduce, n_via) == offsetof(PairReduce, n_via) && offsetof(kmx_pair_reduce, side) == offsetof(PairReduce, side) &&
              offsetof(kmx_pair_reduce, g) == offsetof(PairReduce, g) && offsetof(kmx_pair_reduce, delta) == offsetof(PairReduce, delta) && offsetof(kmx_pair_reduce, delta) == 24,
              "PairReduce (kmx_types.h) is the layout of kmx_pair_reduce");
static_assert(KMX_REDUCE_IGNORED == RED_IGNORED && KMX_REDUCE_BELOW_MIN == RED_BELOW_MIN && KMX_REDUCE_KEPT == RED_KEPT && KMX_REDUCE_TRANSITIVE == RED_TRANSITIVE && KMX_REDUCE_COMPLEX == RED_COMPLEX,
              "the verdicts of kmx_types.h are KMX_REDUCE_*");

static const char *const kRedWhat = "the pair list reduction";
static int red_nomem() { return graph_nomem(kRedWhat); }
static int red_range(u64 need, u64 cap) { return fail(KMX_E_RANGE, "%llu pair links stay, the buffer holds %llu", (unsigned long long)need, (unsigned long long)cap); }

// the buffers of one call (n_ubases: the host form fills it in from uoffsets): what both forms check before anything runs
struct RedArgs {
	int k;
	const uint64_t *uoffs; u64 U, n_ubases;
	const kmx_pair_link *plinks; u64 n_plinks;
	const kmx_pair_reduce_params *params;
	kmx_pair_reduce *rrecs; kmx_pair_link *lout; uint32_t *origin; u64 cap;
	uint64_t *n_out;
	kmx_pair_reduce_stats *stats;
};

static int reduce_args(kmx_model *m, const RedArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	if (A.n_plinks >> 31) return fail(KMX_E_ARG, "%llu pair links: a reduce call takes fewer than 2^31", (unsigned long long)A.n_plinks);
	const kmx_pair_reduce_params *p = A.params;
	if (!p || !A.n_out || !A.stats) return fail(KMX_E_ARG, "null argument");
	if (p->max_row < 1 || p->max_row > 65536) return fail(KMX_E_ARG, "max_row = %u: in [1, 65536]", p->max_row);
	if (p->reserved) return fail(KMX_E_ARG, "kmx_pair_reduce_params.reserved is not 0");
	const Span spans[] = {{A.uoffs, (A.U + 1) * 8, false}, {A.plinks, A.n_plinks * sizeof(PairLink), false}, {A.rrecs, A.n_plinks * sizeof(PairReduce), true},
	                      opt_span(A.lout, A.cap * sizeof(PairLink), true), opt_span(A.origin, A.cap * 4, true)};
	TRY(check_spans(spans, 5));
	*A.n_out = 0;
	*A.stats = kmx_pair_reduce_stats{A.n_plinks, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	return KMX_OK;
}

// the call on device buffers (D: input, parameters and output; the work arrays are filled in here); D.n_plinks > 0.
// KMX_E_RANGE when a list is asked for and the entries that stay do not fit D.cap: records, stats and *n_out are complete and
// nothing is written to the list
static int reduce_core(kmx_model *m, RedDev D, uint64_t *n_out, kmx_pair_reduce_stats *stats)
{
	auto &S = m->red;
	const hipStream_t st = m->stream;
	const u64 E = D.n_plinks;
	for (double &s : S.phase_s) s = 0;
	if (S.d_key.ensure(4 * E, st) != hipSuccess || S.d_val.ensure(4 * E, st) != hipSuccess || S.d_flag.ensure(E, st) != hipSuccess || S.d_sc.ensure(E + 1, st) != hipSuccess ||
	    S.d_cnt.ensure(RED_C_N, st) != hipSuccess)
		return red_nomem();
	D.key = S.d_key; D.skey = S.d_key.get() + 2 * E; D.val = S.d_val; D.sval = S.d_val.get() + 2 * E; D.flag = S.d_flag; D.sc = S.d_sc; D.cnt = S.d_cnt;
	PhaseClock clk(m, S.phase_s);
	HIPCHK(kmxk::reduce_rows(D, st));
	clk.lap(0);
	hipError_t e = kmxk::reduce_sort(D, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return red_nomem();
	HIPCHK(e);
	clk.lap(1);
	HIPCHK(kmxk::reduce_verdicts(D, st));
	clk.lap(2);
	e = kmxk::reduce_scan(D, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return red_nomem();
	HIPCHK(e);
	u64 total = 0;
	unsigned long long c[RED_C_N] = {0, 0, 0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&total, D.sc + E, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait for a result: n_out and the counters
	HIPCHK(hipGetLastError());
	*n_out = total;
	*stats = kmx_pair_reduce_stats{E, c[RED_IGNORED], c[RED_BELOW_MIN], c[RED_KEPT], c[RED_TRANSITIVE], c[RED_COMPLEX], total, 2 * (E - c[RED_IGNORED] - c[RED_BELOW_MIN]), c[RED_C_EXAMINED], 0};
	const bool list = D.lout || D.origin;
	if (list && total > D.cap) { clk.lap(3); return red_range(total, D.cap); }
	if (list) {
		HIPCHK(kmxk::reduce_compact(D, st));
		HIPCHK(hipStreamSynchronize(st));                          // nothing is left in flight
		HIPCHK(hipGetLastError());
	}
	clk.lap(3);
	return KMX_OK;
}

// the sizes and parameters of the kernel block; the pointers are the form's own
static RedDev reduce_dev_of(const RedArgs &A)
{
	RedDev D{};
	D.k = A.k; D.U = A.U; D.n_ubases = A.n_ubases; D.n_plinks = A.n_plinks; D.cap = A.cap;
	D.min_pairs = A.params->min_pairs; D.inner = A.params->inner; D.tol = A.params->tol; D.max_row = A.params->max_row;
	return D;
}

static int kmx_unitig_pair_reduce_dev_impl(kmx_model *m, const RedArgs &A)
{
	TRY(reduce_args(m, A));
	if (!A.n_plinks) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	RedDev D = reduce_dev_of(A);
	D.uoffs = (const u64 *)A.uoffs; D.plinks = (const PairLink *)A.plinks;
	D.rrecs = (PairReduce *)A.rrecs; D.lout = (PairLink *)A.lout; D.origin = A.origin;
	return reduce_core(m, D, A.n_out, A.stats);
}

static int kmx_unitig_pair_reduce_impl(kmx_model *m, RedArgs A)
{
	TRY(check_unitig_count(A.U));
	TRY(check_offsets(A.uoffs, A.U));
	A.n_ubases = A.uoffs[A.U];
	TRY(reduce_args(m, A));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_pair_list(A.plinks, A.n_plinks));
	const u64 U = A.U, np = A.n_plinks;
	if (!np) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	Staging G(m, kRedWhat);
	RedDev D = reduce_dev_of(A);
	D.cap = std::min<u64>(A.cap, np);                              // the list is staged at what always suffices, never beyond the caller's capacity
	D.uoffs = G.in<u64>(A.uoffs, U + 1); D.plinks = G.in<PairLink>(A.plinks, np);
	D.rrecs = G.out<PairReduce>(np); D.lout = A.lout ? G.out<PairLink>(D.cap) : nullptr; D.origin = A.origin ? G.out<u32>(D.cap) : nullptr;
	TRY(G.status());
	const int rc = reduce_core(m, D, A.n_out, A.stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	G.down(A.rrecs, D.rrecs, np);
	if (rc == KMX_OK) {
		if (A.lout) G.down(A.lout, D.lout, *A.n_out);
		if (A.origin) G.down(A.origin, D.origin, *A.n_out);
	}
	TRY(G.finish());
	return rc == KMX_OK ? KMX_OK : red_range(*A.n_out, A.cap);
}

static int kmx_unitig_pair_reduce_last_phases_impl(kmx_model *m, double *seconds)
{
	if (!m || !seconds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 4; i++) seconds[i] = m->red.phase_s[i];
	return KMX_OK;
}
