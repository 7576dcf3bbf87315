// scaffold_host.h -- kmx_unitig_scaffold[_dev]: scaffolds from the pair links between unitigs (the rule: include/kmx.h; the
// kernels: scaffold_kernels.h; the launchers: unitig_device.hip).  Included into kmx_api.hip after pair_host.h.
//
// scaffold_core runs the construction on device buffers: bests and verdicts per list entry, the chain links, the ranking of the
// 2 U oriented unitigs by the contigs' pointer doubling with the second rank in bytes (one stream wait per round: a word says
// whether anything moved), the cut of what is left on cycles and its ranking, the marks and their scan, then records, steps and
// places, and ONE wait for the totals and the counters.  Only when that wait has shown that the bytes fit are they written: 'N'
// over sseq[0, n_sbases), the unitigs over it; a last wait leaves nothing in flight.  The work arrays stay on the handle by
// capacity (kmx_model::scf).  The _dev form checks what can be checked without reading a buffer and hands the caller's pointers
// over; the host form validates offsets and the list's order, stages input and output in buffers of its own for the length of
// the call, and downloads.  The checks of k, offsets, unitig lengths and buffers, the staging owner and the phase clock are
// shared: graph_host.h.
static_assert(sizeof(kmx_scaffold) == 64 && sizeof(Scaffold) == 64 && sizeof(kmx_scaffold_step) == 16 && sizeof(ScfStep) == 16 && sizeof(kmx_scaffold_place) == 16 && sizeof(ScfPlace) == 16 &&
              sizeof(kmx_scaffold_stats) == 80 && sizeof(kmx_scaffold_params) == 32,
              "kmx_scaffold is 64 bytes, kmx_scaffold_step 16, kmx_scaffold_place 16, kmx_scaffold_stats 80, kmx_scaffold_params 32");
static_assert(offsetof(kmx_scaffold, n_kmers) == offsetof(Scaffold, n_kmers) && offsetof(kmx_scaffold, min_count) == offsetof(Scaffold, min_count) && offsetof(kmx_scaffold, first_step) == offsetof(Scaffold, first_step) &&
              offsetof(kmx_scaffold, n_steps) == offsetof(Scaffold, n_steps) && offsetof(kmx_scaffold, n_gap_bases) == offsetof(Scaffold, n_gap_bases) && offsetof(kmx_scaffold, min_pairs) == offsetof(Scaffold, min_pairs) &&
              offsetof(kmx_scaffold, sum_pairs) == offsetof(Scaffold, sum_pairs) && offsetof(kmx_scaffold, sum_pairs) == 56,
              "Scaffold (kmx_types.h) is the layout of kmx_scaffold");
static_assert(offsetof(kmx_scaffold_step, est) == offsetof(ScfStep, est) && offsetof(kmx_scaffold_place, step) == offsetof(ScfPlace, step) && offsetof(kmx_scaffold_place, off) == offsetof(ScfPlace, off) &&
              KMX_SCAFFOLD_CIRCULAR == SCF_CIRCULAR,
              "ScfStep and ScfPlace (kmx_types.h) are the layouts of kmx_scaffold_step and kmx_scaffold_place");

static const char *const kScfWhat = "the scaffold construction";
static int scf_nomem() { return graph_nomem(kScfWhat); }
static int scf_range(u64 need, u64 cap) { return fail(KMX_E_RANGE, "%llu scaffold bases, the buffer holds %llu", (unsigned long long)need, (unsigned long long)cap); }

// the buffers of one call (n_ubases: the host form fills it in from uoffsets): what both forms check before anything runs
struct ScfArgs {
	int k;
	const char *useq; const uint64_t *uoffs; u64 U, n_ubases; const kmx_unitig *urec;
	const kmx_pair_link *plinks; u64 n_plinks;
	const kmx_scaffold_params *params;
	char *sseq; u64 seq_cap; uint64_t *soffs; kmx_scaffold *srec; kmx_scaffold_step *steps; kmx_scaffold_place *place;
	uint64_t *n_scaffolds, *n_sbases;
	kmx_scaffold_stats *stats;
};

static int scaffold_args(kmx_model *m, const ScfArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	if (A.n_plinks >> 31) return fail(KMX_E_ARG, "%llu pair links: a scaffold call takes fewer than 2^31", (unsigned long long)A.n_plinks);
	const kmx_scaffold_params *p = A.params;
	if (!p || !A.n_scaffolds || !A.n_sbases || !A.stats) return fail(KMX_E_ARG, "null argument");
	if (p->ratio > 65536) return fail(KMX_E_ARG, "ratio = %u: at most 65536", p->ratio);
	if (p->min_n > p->max_n) return fail(KMX_E_ARG, "min_n = %u is above max_n = %u", p->min_n, p->max_n);
	if (p->reserved) return fail(KMX_E_ARG, "kmx_scaffold_params.reserved is not 0");
	const u64 U = A.U;                                              // a buffer of no element may be null; the offset arrays always hold one
	const Span spans[] = {{A.useq, A.n_ubases, false}, {A.uoffs, (U + 1) * 8, false}, opt_span(A.urec, U * sizeof(Unitig), false), {A.plinks, A.n_plinks * sizeof(PairLink), false},
	                      {A.sseq, A.seq_cap, true}, {A.soffs, (U + 1) * 8, true}, {A.srec, U * sizeof(Scaffold), true}, {A.steps, U * sizeof(ScfStep), true}, {A.place, U * sizeof(ScfPlace), true}};
	TRY(check_spans(spans, 9));
	*A.n_scaffolds = *A.n_sbases = 0;
	*A.stats = kmx_scaffold_stats{A.n_plinks, 0, U ? 0 : A.n_plinks, 0, 0, 0, 0, 0, 0, 0};   // without a unitig no entry is a pair link
	return KMX_OK;
}

// the construction on device buffers (D: input, parameters and output; the work arrays are filled in here); D.U > 0.
// KMX_E_RANGE when the bytes do not fit D.seq_cap: everything but them is complete
static int scaffold_core(kmx_model *m, ScfDev D, uint64_t *n_scaffolds, uint64_t *n_sbases, kmx_scaffold_stats *stats)
{
	auto &S = m->scf;
	const hipStream_t st = m->stream;
	const u64 U = D.U;
	int lg = 0;
	while ((u64(1) << lg) < 2 * U) lg++;                           // ceil(log2 2U)
	const int T = lg + 1;
	for (double &s : S.phase_s) s = 0;
	S.rounds = 0;
	if (S.d_best.ensure(2 * U, st) != hipSuccess || S.d_nk.ensure(4 * U, st) != hipSuccess || S.d_circ.ensure(U, st) != hipSuccess || S.d_rank[0].ensure(2 * U + 2, st) != hipSuccess ||
	    S.d_rank[1].ensure(2 * U + 2, st) != hipSuccess || S.d_mn.ensure(4 * U, st) != hipSuccess || S.d_sc.ensure(U + 1, st) != hipSuccess || S.d_ubase.ensure(U, st) != hipSuccess ||
	    S.d_cnt.ensure(SCF_C_N, st) != hipSuccess || S.d_flag.ensure(2 * (size_t)T + 2, st) != hipSuccess)
		return scf_nomem();
	D.best = S.d_best; D.nk = S.d_nk; D.only = S.d_nk.get() + 2 * U; D.circ = S.d_circ; D.sc = S.d_sc; D.ubase = S.d_ubase; D.cnt = S.d_cnt;
	HIPCHK(hipMemsetAsync(S.d_flag, 0, (2 * (size_t)T + 2) * 4, st));
	HIPCHK(hipMemsetAsync(S.d_cnt, 0, SCF_C_N * sizeof(unsigned long long), st));
	HIPCHK(hipMemsetAsync(S.d_circ, 0, U, st));
	auto word = [&](int i, u32 *v) {                               // one stream wait
		HIPCHK(hipMemcpyAsync(v, S.d_flag.get() + i, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		return (int)KMX_OK;
	};
	PhaseClock clk(m, S.phase_s);
	u32 *mn[2] = {S.d_mn.get(), S.d_mn.get() + 2 * U};
	HIPCHK(kmxk::scaffold_links(D, S.d_rank[0], mn[0], st));
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
		kmxk::scaffold_cut(D, S.d_rank[c], mn[c], S.d_rank[c ^ 1], st);
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
	const hipError_t e = kmxk::scaffold_mark(D, S.d_rank[c], (CtgTot *)S.d_rank[c ^ 1].get(), S.d_tmp, st);   // the marks: 24 (U + 1) bytes in the spare copy's 16 (2 U + 2)
	if (e == hipErrorOutOfMemory) return scf_nomem();
	HIPCHK(e);
	clk.lap(2);
	kmxk::scaffold_place(D, S.d_rank[c], st);
	CtgTot tot{0, 0, 0};
	unsigned long long cn[SCF_C_N] = {0, 0, 0, 0, 0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&tot, D.sc + U, sizeof tot, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(cn, D.cnt, sizeof cn, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the wait for the counts
	HIPCHK(hipGetLastError());
	clk.lap(3);
	*n_scaffolds = tot.n;
	*n_sbases = tot.len;
	*stats = kmx_scaffold_stats{D.n_plinks, cn[SCF_C_LINKS], cn[SCF_C_IGNORED], cn[SCF_C_BELOW_MIN], cn[SCF_C_BELOW_RATIO], cn[SCF_C_KEPT], cn[SCF_C_CHAIN], tot.n, cn[SCF_C_CIRCULAR], cn[SCF_C_MULTI]};
	if (tot.len > D.seq_cap) return scf_range(tot.len, D.seq_cap);
	HIPCHK(kmxk::scaffold_bytes(D, tot.len, st));
	HIPCHK(hipStreamSynchronize(st));                              // nothing is left in flight
	HIPCHK(hipGetLastError());
	clk.lap(4);
	return KMX_OK;
}

// the sizes and parameters of the kernel block; the pointers are the form's own
static ScfDev scaffold_dev_of(const ScfArgs &A)
{
	ScfDev D{};
	D.k = A.k; D.U = A.U; D.n_ubases = A.n_ubases; D.n_plinks = A.n_plinks; D.seq_cap = A.seq_cap;
	D.min_pairs = A.params->min_pairs; D.ratio = A.params->ratio; D.inner = A.params->inner; D.min_n = A.params->min_n; D.max_n = A.params->max_n;
	return D;
}

static int kmx_unitig_scaffold_dev_impl(kmx_model *m, const ScfArgs &A)
{
	TRY(scaffold_args(m, A));
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!A.U) {
		HIPCHK(hipMemsetAsync(A.soffs, 0, 8, st));
		HIPCHK(hipStreamSynchronize(st));
		return KMX_OK;
	}
	ScfDev D = scaffold_dev_of(A);
	D.useq = (const unsigned char *)A.useq; D.uoffs = (const u64 *)A.uoffs; D.urec = (const Unitig *)A.urec; D.plinks = (const PairLink *)A.plinks;
	D.sseq = (unsigned char *)A.sseq; D.soffs = (u64 *)A.soffs; D.srec = (Scaffold *)A.srec; D.steps = (ScfStep *)A.steps; D.place = (ScfPlace *)A.place;
	return scaffold_core(m, D, A.n_scaffolds, A.n_sbases, A.stats);
}

static int kmx_unitig_scaffold_impl(kmx_model *m, ScfArgs A)
{
	TRY(check_unitig_count(A.U));
	TRY(check_offsets(A.uoffs, A.U));
	A.n_ubases = A.uoffs[A.U];
	TRY(scaffold_args(m, A));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_pair_list(A.plinks, A.n_plinks));
	HIPCHK(hipSetDevice(m->device));
	const u64 U = A.U;
	if (!U) {
		A.soffs[0] = 0;
		return KMX_OK;
	}
	Staging G(m, kScfWhat);
	ScfDev D = scaffold_dev_of(A);
	D.useq = G.in<unsigned char>(A.useq, A.n_ubases); D.uoffs = G.in<u64>(A.uoffs, U + 1); D.urec = A.urec ? G.in<Unitig>(A.urec, U) : nullptr; D.plinks = G.in<PairLink>(A.plinks, A.n_plinks);
	D.sseq = G.out<unsigned char>(A.seq_cap); D.soffs = G.out<u64>(U + 1); D.srec = G.out<Scaffold>(U); D.steps = G.out<ScfStep>(U); D.place = G.out<ScfPlace>(U);
	TRY(G.status());
	const int rc = scaffold_core(m, D, A.n_scaffolds, A.n_sbases, A.stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	const u64 S = *A.n_scaffolds;
	if (S > U) return fail(KMX_E_ARG, "internal error: the scaffolds exceed the input's sizes");
	if (rc == KMX_OK) G.down(A.sseq, D.sseq, *A.n_sbases);
	G.down(A.soffs, D.soffs, S + 1);
	G.down(A.srec, D.srec, S);
	G.down(A.steps, D.steps, U);
	G.down(A.place, D.place, U);
	TRY(G.finish());
	return rc == KMX_OK ? KMX_OK : scf_range(*A.n_sbases, A.seq_cap);
}

static int kmx_unitig_scaffold_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 5; i++) seconds[i] = m->scf.phase_s[i];
	*rounds = m->scf.rounds;
	return KMX_OK;
}
