// lift_host.h -- kmx_unitig_pair_lift[_dev]: a unitig-level pair list in contig coordinates (the rule: include/kmx.h; the kernels:
// lift_kernels.h; the launchers: unitig_device.hip).  Included into kmx_api.hip after reduce_host.h.
//
// lift_core runs the call on device buffers: the classes with the work items, their sort, the scan of the key changes with the
// fold, the store (which checks the merged count against the capacity on the device), and ONE wait that brings n_out and the
// counters to the host.  The work arrays stay on the handle by capacity (kmx_model::lift).  The _dev form checks what can be
// checked without reading a buffer and hands the caller's pointers over; the host form validates offsets, places and the list's
// order, stages input and output in buffers of its own for the length of the call, and downloads.  The checks, the staging owner
// and the phase clock are shared: graph_host.h.
static_assert(sizeof(kmx_pair_lift) == 32 && sizeof(PairLift) == 32 && sizeof(kmx_pair_lift_params) == 8 && sizeof(kmx_pair_lift_stats) == 128,
              "kmx_pair_lift is 32 bytes, kmx_pair_lift_params 8, kmx_pair_lift_stats 128");
static_assert(offsetof(kmx_pair_lift, out) == offsetof(PairLift, out) && offsetof(kmx_pair_lift, A) == offsetof(PairLift, A) && offsetof(kmx_pair_lift, B) == offsetof(PairLift, B) &&
              offsetof(kmx_pair_lift, shift) == offsetof(PairLift, shift) && offsetof(kmx_pair_lift, flipped) == offsetof(PairLift, flipped) && offsetof(kmx_pair_lift, flipped) == 24,
              "PairLift (kmx_types.h) is the layout of kmx_pair_lift");
static_assert(KMX_LIFT_IGNORED == LIFT_IGNORED && KMX_LIFT_SAME == LIFT_SAME && KMX_LIFT_INVERTED == LIFT_INVERTED && KMX_LIFT_LINK == LIFT_LINK && KMX_LIFT_FAR == LIFT_FAR,
              "the classes of kmx_types.h are KMX_LIFT_*");
static_assert(KMX_LIFT_FOLD_WAVE == LIFT_FOLD_WAVE && KMX_LIFT_FOLD_PLAIN == LIFT_FOLD_PLAIN, "the fold variants of kmx_types.h are KMX_LIFT_FOLD_*");

static const char *const kLiftWhat = "the pair list lift";
static int lift_nomem() { return graph_nomem(kLiftWhat); }
static int lift_range(u64 need, u64 cap) { return fail(KMX_E_RANGE, "the lifted list has %llu pair links, the buffer holds %llu", (unsigned long long)need, (unsigned long long)cap); }

// the buffers of one call (n_ubases: the host form fills it in from uoffsets): what both forms check before anything runs
struct LiftArgs {
	int k;
	const uint64_t *uoffs; u64 U, n_ubases;
	const kmx_contig_place *place; const kmx_contig *crec; u64 C;
	const kmx_pair_link *plinks; u64 n_plinks;
	const kmx_pair_lift_params *params;
	kmx_pair_lift *lrec; kmx_pair_link *lout; u64 cap;
	uint64_t *n_out;
	kmx_pair_lift_stats *stats;
};

static int lift_args(kmx_model *m, const LiftArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	if (A.n_plinks >> 31) return fail(KMX_E_ARG, "%llu pair links: a lift call takes fewer than 2^31", (unsigned long long)A.n_plinks);
	if (A.C > A.U) return fail(KMX_E_ARG, "%llu contigs of %llu unitigs", (unsigned long long)A.C, (unsigned long long)A.U);
	if (!A.params || !A.n_out || !A.stats || !A.uoffs) return fail(KMX_E_ARG, "null argument");
	if (A.params->reserved) return fail(KMX_E_ARG, "kmx_pair_lift_params.reserved is not 0");
	if (!A.lout && A.cap) return fail(KMX_E_ARG, "a capacity of %llu without a list", (unsigned long long)A.cap);
	const Span spans[] = {{A.uoffs, (A.U + 1) * 8, false}, {A.place, A.U * sizeof(CtgPlace), false}, {A.crec, A.C * sizeof(Contig), false}, {A.plinks, A.n_plinks * sizeof(PairLink), false},
	                      {A.lrec, A.n_plinks * sizeof(PairLift), true}, opt_span(A.lout, A.cap * sizeof(PairLink), true)};
	TRY(check_spans(spans, 6));
	*A.n_out = 0;
	*A.stats = kmx_pair_lift_stats();
	A.stats->n_entries = A.n_plinks;
	return KMX_OK;
}

// every unitig lies in a contig of the set, inside it (uoffsets have passed check_offsets and check_unitig_lengths)
static int check_places(const uint64_t *uoffs, u64 U, int k, const kmx_contig_place *place, const kmx_contig *crec, u64 C)
{
	for (u64 u = 0; u < U; u++) {
		const u64 c = place[u].oc >> 1, m = uoffs[u + 1] - uoffs[u] - (u64)k + 1;
		if (c >= C) return fail(KMX_E_ARG, "place[%llu] names contig %llu of %llu", (unsigned long long)u, (unsigned long long)c, (unsigned long long)C);
		if (crec[c].n_kmers >> 32 || (u64)place[u].off + m > crec[c].n_kmers)
			return fail(KMX_E_ARG, "place[%llu]: %llu windows at offset %u do not lie in contig %llu of %llu windows", (unsigned long long)u, (unsigned long long)m, place[u].off, (unsigned long long)c,
			            (unsigned long long)crec[c].n_kmers);
	}
	return KMX_OK;
}

// the call on device buffers (D: input, parameters and output; the work arrays are filled in here); D.n_plinks > 0.
// KMX_E_RANGE when a list is asked for and the merged entries do not fit D.cap: records, stats and *n_out are complete and
// nothing is written to the list
static int lift_core(kmx_model *m, LiftDev D, uint64_t *n_out, kmx_pair_lift_stats *stats)
{
	auto &S = m->lift;
	const hipStream_t st = m->stream;
	const u64 E = D.n_plinks;
	for (double &s : S.phase_s) s = 0;
	if (S.d_key.ensure(2 * E, st) != hipSuccess || S.d_idx.ensure(2 * E, st) != hipSuccess || S.d_item.ensure(2 * E, st) != hipSuccess || S.d_sc.ensure(E + 1, st) != hipSuccess ||
	    S.d_cnt.ensure(LIFT_C_N, st) != hipSuccess)
		return lift_nomem();
	D.key = S.d_key; D.skey = S.d_key.get() + E; D.idx = S.d_idx; D.sidx = S.d_idx.get() + E; D.item = S.d_item; D.mrg = S.d_item.get() + E; D.sc = S.d_sc; D.cnt = S.d_cnt;
	D.fold = S.fold;
	PhaseClock clk(m, S.phase_s);
	HIPCHK(kmxk::lift_classify(D, st));
	clk.lap(0);
	hipError_t e = kmxk::lift_sort(D, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return lift_nomem();
	HIPCHK(e);
	clk.lap(1);
	e = kmxk::lift_fold(D, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return lift_nomem();
	HIPCHK(e);
	clk.lap(2);
	HIPCHK(kmxk::lift_store(D, st));
	u64 total = 0;
	unsigned long long c[LIFT_C_N];
	HIPCHK(hipMemcpyAsync(&total, D.sc + E, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait: n_out and the counters
	HIPCHK(hipGetLastError());
	clk.lap(3);
	*n_out = total;
	kmx_pair_lift_stats &T = *stats;
	T = kmx_pair_lift_stats();
	T.n_entries = E; T.n_ignored = c[LIFT_IGNORED]; T.n_same = c[LIFT_SAME]; T.n_inverted = c[LIFT_INVERTED]; T.n_link = c[LIFT_LINK]; T.n_far = c[LIFT_FAR];
	T.n_same_back = c[LIFT_C_SAME_BACK]; T.n_out = total;
	T.pairs_ignored = c[LIFT_C_PAIRS + LIFT_IGNORED]; T.pairs_same = c[LIFT_C_PAIRS + LIFT_SAME]; T.pairs_inverted = c[LIFT_C_PAIRS + LIFT_INVERTED]; T.pairs_link = c[LIFT_C_PAIRS + LIFT_LINK];
	T.pairs_far = c[LIFT_C_PAIRS + LIFT_FAR]; T.pairs_same_back = c[LIFT_C_PAIRS_SAME_BACK]; T.sum_same_d = (int64_t)c[LIFT_C_SUM_SAME_D];
	if (D.lout && total > D.cap) return lift_range(total, D.cap);
	return KMX_OK;
}

// the sizes and parameters of the kernel block; the pointers are the form's own
static LiftDev lift_dev_of(const LiftArgs &A)
{
	LiftDev D{};
	D.k = A.k; D.U = A.U; D.n_ubases = A.n_ubases; D.C = A.C; D.n_plinks = A.n_plinks; D.cap = A.cap;
	D.max_dist = A.params->max_dist;
	return D;
}

static int kmx_unitig_pair_lift_dev_impl(kmx_model *m, const LiftArgs &A)
{
	TRY(lift_args(m, A));
	if (!A.n_plinks) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	LiftDev D = lift_dev_of(A);
	D.uoffs = (const u64 *)A.uoffs; D.place = (const CtgPlace *)A.place; D.crec = (const Contig *)A.crec; D.plinks = (const PairLink *)A.plinks;
	D.lrec = (PairLift *)A.lrec; D.lout = (PairLink *)A.lout;
	return lift_core(m, D, A.n_out, A.stats);
}

static int kmx_unitig_pair_lift_impl(kmx_model *m, LiftArgs A)
{
	TRY(check_unitig_count(A.U));
	TRY(check_offsets(A.uoffs, A.U));
	A.n_ubases = A.uoffs[A.U];
	TRY(lift_args(m, A));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_places(A.uoffs, A.U, A.k, A.place, A.crec, A.C));
	TRY(check_pair_list(A.plinks, A.n_plinks));
	const u64 U = A.U, np = A.n_plinks;
	if (!np) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	Staging G(m, kLiftWhat);
	LiftDev D = lift_dev_of(A);
	D.cap = std::min<u64>(A.cap, np);                              // the list is staged at what always suffices, never beyond the caller's capacity
	D.uoffs = G.in<u64>(A.uoffs, U + 1); D.place = G.in<CtgPlace>(A.place, U); D.crec = G.in<Contig>(A.crec, A.C); D.plinks = G.in<PairLink>(A.plinks, np);
	D.lrec = G.out<PairLift>(np); D.lout = A.lout ? G.out<PairLink>(D.cap) : nullptr;
	TRY(G.status());
	const int rc = lift_core(m, D, A.n_out, A.stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	G.down(A.lrec, D.lrec, np);
	if (rc == KMX_OK && A.lout) G.down(A.lout, D.lout, *A.n_out);
	TRY(G.finish());
	return rc == KMX_OK ? KMX_OK : lift_range(*A.n_out, A.cap);
}

static int kmx_unitig_pair_lift_fold_variant_impl(kmx_model *m, int variant)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (variant != KMX_LIFT_FOLD_WAVE && variant != KMX_LIFT_FOLD_PLAIN) return fail(KMX_E_ARG, "fold variant %d: KMX_LIFT_FOLD_WAVE or KMX_LIFT_FOLD_PLAIN", variant);
	m->lift.fold = variant;
	return KMX_OK;
}

static int kmx_unitig_pair_lift_last_phases_impl(kmx_model *m, double *seconds)
{
	if (!m || !seconds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 4; i++) seconds[i] = m->lift.phase_s[i];
	return KMX_OK;
}
