// contig_host.h -- kmx_unitig_contigs[_dev]: contigs from the read-supported edges between unitigs (the rule: include/kmx.h; the
// kernels: contig_kernels.h; the launchers: unitig_device.hip).  Included into kmx_api.hip after map_host.h.
//
// contig_core runs the construction on device buffers: supports and verdicts, the chain links, the ranking of the 2 U oriented
// unitigs by pointer doubling (one stream wait per round: a word says whether anything moved), the cut of what is left on
// cycles and its ranking, the marks and their scan, then records, steps, places, the bytes and the contig graph, and ONE wait for
// the totals and the counters.  The work arrays stay on the handle by capacity (kmx_model::ctg).  The _dev form checks what
// can be checked without reading a buffer and hands the caller's pointers over; the host form validates offsets and CSR, stages
// input and output in buffers of its own for the length of the call, and downloads.  The entry point fills a CtgArgs, contig_args
// checks it for both forms (the one table of the call's buffers is there) and contig_dev_of fills the kernel block's sizes.  The
// checks of k, offsets, unitig lengths, CSR and buffers, the staging owner and the phase clock are shared: graph_host.h.
static_assert(sizeof(kmx_contig) == 64 && sizeof(Contig) == 64 && sizeof(kmx_contig_place) == 8 && sizeof(CtgPlace) == 8 && sizeof(kmx_contig_stats) == 64 && sizeof(kmx_contig_params) == 16,
              "kmx_contig is 64 bytes, kmx_contig_place 8, kmx_contig_stats 64, kmx_contig_params 16");
static_assert(offsetof(kmx_contig, min_count) == offsetof(Contig, min_count) && offsetof(kmx_contig, first_step) == offsetof(Contig, first_step) && offsetof(kmx_contig, n_steps) == offsetof(Contig, n_steps) &&
              offsetof(kmx_contig, circular) == offsetof(Contig, circular) && offsetof(kmx_contig, min_support) == offsetof(Contig, min_support) && offsetof(kmx_contig, reserved2) == offsetof(Contig, reserved2),
              "Contig (kmx_types.h) is the layout of kmx_contig");
static_assert(sizeof(CtgRank) == 16 && sizeof(CtgTot) == 24, "the rank state is 16 bytes per oriented unitig, a mark 24 per unitig");

static const char *const kCtgWhat = "the contig construction";
static int ctg_nomem() { return graph_nomem(kCtgWhat); }

// the buffers of one call (n_ubases: the host form fills it in from uoffsets): what both forms check before anything runs
struct CtgArgs {
	int k;
	const char *useq; const uint64_t *uoffs; u64 U, n_ubases; const kmx_unitig *urec;
	const uint64_t *loffs; const uint32_t *links; u64 n_links; const uint64_t *hits;
	const kmx_contig_params *params;
	char *cseq; uint64_t *coffs; kmx_contig *crec; uint32_t *steps; kmx_contig_place *place;
	uint64_t *cloffs; uint32_t *clinks; uint64_t *csup;
	uint64_t *n_contigs, *n_cbases, *n_clinks;
	kmx_contig_stats *stats;
};

static int contig_args(kmx_model *m, const CtgArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	const kmx_contig_params *p = A.params;
	if (!p || !A.n_contigs || !A.n_cbases || !A.n_clinks || !A.stats) return fail(KMX_E_ARG, "null argument");
	if (p->ratio > 65536) return fail(KMX_E_ARG, "ratio = %u: at most 65536", p->ratio);
	if (p->reserved) return fail(KMX_E_ARG, "kmx_contig_params.reserved is not 0");
	const u64 U = A.U, nb = A.n_ubases, nl = A.n_links;               // a buffer of no element may be null; the offset arrays always hold one
	const Span spans[] = {{A.useq, nb, false}, {A.uoffs, (U + 1) * 8, false}, opt_span(A.urec, U * sizeof(Unitig), false), {A.loffs, (2 * U + 1) * 8, false}, {A.links, nl * 4, false},
	                      {A.hits, nl * 8, false}, {A.cseq, nb, true}, {A.coffs, (U + 1) * 8, true}, {A.crec, U * sizeof(Contig), true}, {A.steps, U * 4, true}, {A.place, U * 8, true},
	                      {A.cloffs, (2 * U + 1) * 8, true}, {A.clinks, nl * 4, true}, {A.csup, nl * 8, true}};
	TRY(check_spans(spans, 14));
	*A.n_contigs = *A.n_cbases = *A.n_clinks = 0;
	*A.stats = kmx_contig_stats{0, 0, 0, 0, 0, 0, 0, 0};
	return KMX_OK;
}

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
	PhaseClock clk(m, S.phase_s);
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

// the sizes and parameters of the kernel block; the pointers are the form's own
static CtgDev contig_dev_of(const CtgArgs &A)
{
	CtgDev D{};
	D.k = A.k; D.U = A.U; D.n_ubases = A.n_ubases; D.n_links = A.n_links;
	D.min_reads = A.params->min_reads; D.ratio = A.params->ratio;
	return D;
}

static int kmx_unitig_contigs_dev_impl(kmx_model *m, const CtgArgs &A)
{
	TRY(contig_args(m, A));
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!A.U) {
		HIPCHK(hipMemsetAsync(A.coffs, 0, 8, st));
		HIPCHK(hipMemsetAsync(A.cloffs, 0, 8, st));
		HIPCHK(hipStreamSynchronize(st));
		return KMX_OK;
	}
	CtgDev D = contig_dev_of(A);
	D.useq = (const unsigned char *)A.useq; D.uoffs = (const u64 *)A.uoffs; D.urec = (const Unitig *)A.urec; D.loffs = (const u64 *)A.loffs; D.links = A.links; D.hits = (const u64 *)A.hits;
	D.cseq = (unsigned char *)A.cseq; D.coffs = (u64 *)A.coffs; D.crec = (Contig *)A.crec; D.steps = A.steps; D.place = (CtgPlace *)A.place; D.cloffs = (u64 *)A.cloffs; D.clinks = A.clinks;
	D.csup = (u64 *)A.csup;
	return contig_core(m, D, A.n_contigs, A.n_cbases, A.n_clinks, A.stats);
}

static int kmx_unitig_contigs_impl(kmx_model *m, CtgArgs A)
{
	TRY(check_unitig_count(A.U));
	TRY(check_offsets(A.uoffs, A.U));
	A.n_ubases = A.uoffs[A.U];
	TRY(contig_args(m, A));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_link_csr(A.loffs, A.links, A.n_links, A.U, true));
	HIPCHK(hipSetDevice(m->device));
	const u64 U = A.U, n_ubases = A.n_ubases, n_links = A.n_links;
	if (!U) {
		A.coffs[0] = A.cloffs[0] = 0;
		return KMX_OK;
	}
	Staging G(m, kCtgWhat);
	CtgDev D = contig_dev_of(A);
	D.useq = G.in<unsigned char>(A.useq, n_ubases); D.cseq = G.out<unsigned char>(n_ubases); D.uoffs = G.in<u64>(A.uoffs, U + 1); D.loffs = G.in<u64>(A.loffs, 2 * U + 1);
	D.hits = G.in<u64>(A.hits, n_links); D.coffs = G.out<u64>(U + 1); D.cloffs = G.out<u64>(2 * U + 1); D.csup = G.out<u64>(n_links); D.links = G.in<u32>(A.links, n_links);
	D.steps = G.out<u32>(U); D.clinks = G.out<u32>(n_links); D.urec = A.urec ? G.in<Unitig>(A.urec, U) : nullptr; D.crec = G.out<Contig>(U); D.place = G.out<CtgPlace>(U);
	TRY(G.status());
	TRY(contig_core(m, D, A.n_contigs, A.n_cbases, A.n_clinks, A.stats));
	const u64 C = *A.n_contigs, ncl = *A.n_clinks;
	if (C > U || *A.n_cbases > n_ubases || ncl > n_links) return fail(KMX_E_ARG, "internal error: the contigs exceed the input's sizes");
	G.down(A.cseq, D.cseq, *A.n_cbases);
	G.down(A.coffs, D.coffs, C + 1);
	G.down(A.crec, D.crec, C);
	G.down(A.steps, D.steps, U);
	G.down(A.place, D.place, U);
	G.down(A.cloffs, D.cloffs, 2 * C + 1);
	G.down(A.clinks, D.clinks, ncl);
	G.down(A.csup, D.csup, ncl);
	return G.finish();
}

static int kmx_unitig_contigs_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 5; i++) seconds[i] = m->ctg.phase_s[i];
	*rounds = m->ctg.rounds;
	return KMX_OK;
}
