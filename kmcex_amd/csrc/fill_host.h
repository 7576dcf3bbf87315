// fill_host.h -- kmx_unitig_scaffold_fill[_dev]: the scaffolds spelled again with the gaps filled that the pair paths cross (the
// rule: include/kmx.h; the kernels: fill_kernels.h; the launchers: unitig_device.hip).  Included into kmx_api.hip after
// pair_path_host.h.
//
// fill_core runs the call on device buffers: the kinds, the scan, and ONE wait that brings the totals and the counters to the
// host.  Only then are the piece arrays sized (by the pieces there are, not by a bound) and steps, records and pieces written;
// and only when the wait has shown that the bytes fit are they written: 'N' over fseq[0, n_fbases), the steps over it, the path
// pieces over those; a last wait leaves nothing in flight.  The work arrays stay on the handle by capacity (kmx_model::fill).
// The _dev form checks what can be checked without reading a buffer and hands the caller's pointers over; the host form
// validates offsets, the list's order and the scaffolds' step ranges, stages input and output in buffers of its own for the
// length of the call, and downloads.  The checks, the staging owner and the phase clock are shared: graph_host.h.
static_assert(sizeof(kmx_scaffold_fill) == 64 && sizeof(ScfFill) == 64 && sizeof(kmx_fill_step) == 32 && sizeof(FillStep) == 32 && sizeof(kmx_fill_stats) == 80 && sizeof(kmx_fill_params) == 8,
              "kmx_scaffold_fill is 64 bytes, kmx_fill_step 32, kmx_fill_stats 80, kmx_fill_params 8");
static_assert(offsetof(kmx_scaffold_fill, n_fill_bases) == offsetof(ScfFill, n_fill_bases) && offsetof(kmx_scaffold_fill, n_n_links) == offsetof(ScfFill, n_n_links) &&
              offsetof(kmx_scaffold_fill, first_piece) == offsetof(ScfFill, first_piece) && offsetof(kmx_scaffold_fill, first_piece) == 56 && offsetof(kmx_fill_step, entry) == offsetof(FillStep, entry) &&
              offsetof(kmx_fill_step, n_pieces) == offsetof(FillStep, n_pieces) && offsetof(kmx_fill_step, off) == offsetof(FillStep, off) && offsetof(kmx_fill_step, n_front) == offsetof(FillStep, n_front) &&
              offsetof(kmx_fill_step, n_front) == 24,
              "ScfFill and FillStep (kmx_types.h) are the layouts of kmx_scaffold_fill and kmx_fill_step");
static_assert(KMX_FILL_HEAD == FILL_HEAD && KMX_FILL_N == FILL_N && KMX_FILL_ADJACENT == FILL_ADJACENT && KMX_FILL_PATH == FILL_PATH, "the kinds of kmx_types.h are KMX_FILL_*");

static const char *const kFillWhat = "the scaffold fill";
static int fill_nomem() { return graph_nomem(kFillWhat); }
static int fill_range(u64 need, u64 cap, u64 need_pc, u64 cap_pc, bool seq_short)
{
	if (seq_short) return fail(KMX_E_RANGE, "%llu bases of filled scaffolds, the buffer holds %llu", (unsigned long long)need, (unsigned long long)cap);
	return fail(KMX_E_RANGE, "%llu path pieces, the buffer holds %llu", (unsigned long long)need_pc, (unsigned long long)cap_pc);
}

// the buffers of one call (n_ubases: the host form fills it in from uoffsets): what both forms check before anything runs
struct FillArgs {
	int k;
	const char *useq; const uint64_t *uoffs; u64 U, n_ubases;
	const kmx_scaffold *srec; u64 S; const kmx_scaffold_step *steps;
	const kmx_pair_link *plinks; u64 n_plinks; const kmx_pair_path *precs; const uint32_t *psteps; u64 n_psteps;
	const kmx_fill_params *params;
	char *fseq; u64 seq_cap; uint64_t *foffs; kmx_scaffold_fill *frec; kmx_fill_step *fsteps; uint32_t *pieces; u64 piece_cap;
	uint64_t *n_fbases, *n_pieces;
	kmx_fill_stats *stats;
};

static int fill_args(kmx_model *m, const FillArgs &A)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_odd_k(A.k));
	TRY(check_unitig_count(A.U));
	if (A.n_plinks >> 31) return fail(KMX_E_ARG, "%llu pair links: a fill call takes fewer than 2^31", (unsigned long long)A.n_plinks);
	if (A.S > A.U) return fail(KMX_E_ARG, "%llu scaffolds of %llu unitigs", (unsigned long long)A.S, (unsigned long long)A.U);
	const kmx_fill_params *p = A.params;
	if (!p || !A.n_fbases || !A.stats || (A.pieces && !A.n_pieces)) return fail(KMX_E_ARG, "null argument");
	if (p->kinds > 3) return fail(KMX_E_ARG, "kinds = %u: in [0, 3]", p->kinds);
	if (p->reserved) return fail(KMX_E_ARG, "kmx_fill_params.reserved is not 0");
	const u64 U = A.U;
	const Span spans[] = {{A.useq, A.n_ubases, false}, {A.uoffs, (U + 1) * 8, false}, {A.srec, A.S * sizeof(Scaffold), false}, {A.steps, U * sizeof(ScfStep), false},
	                      {A.plinks, A.n_plinks * sizeof(PairLink), false}, {A.precs, A.n_plinks * sizeof(PairPath), false}, {A.psteps, A.n_psteps * 4, false},
	                      {A.fseq, A.seq_cap, true}, {A.foffs, (A.S + 1) * 8, true}, {A.frec, A.S * sizeof(ScfFill), true}, {A.fsteps, U * sizeof(FillStep), true}, opt_span(A.pieces, A.piece_cap * 4, true)};
	TRY(check_spans(spans, 12));
	*A.n_fbases = 0;
	if (A.n_pieces) *A.n_pieces = 0;
	*A.stats = kmx_fill_stats{0, 0, 0, 0, 0, 0, 0, 0, {0, 0}};
	return KMX_OK;
}

// the call on device buffers (D: input, parameters and output; the work arrays are filled in here); D.U > 0.  KMX_E_RANGE when the
// bytes do not fit D.seq_cap or the pieces D.piece_cap: everything but the one that does not fit is complete
static int fill_core(kmx_model *m, FillDev D, uint64_t *n_fbases, uint64_t *n_pieces, kmx_fill_stats *stats)
{
	auto &S = m->fill;
	const hipStream_t st = m->stream;
	const u64 U = D.U;
	for (double &s : S.phase_s) s = 0;
	if (S.d_tot.ensure(U + 1, st) != hipSuccess || S.d_sc.ensure(U + 1, st) != hipSuccess || S.d_ubase.ensure(U, st) != hipSuccess || S.d_cnt.ensure(FILL_C_N, st) != hipSuccess) return fill_nomem();
	D.tot = S.d_tot; D.sc = S.d_sc; D.ubase = S.d_ubase; D.cnt = S.d_cnt;
	PhaseClock clk(m, S.phase_s);
	HIPCHK(kmxk::fill_kinds(D, st));
	clk.lap(0);
	const hipError_t e = kmxk::fill_scan(D, S.d_tmp, st);
	if (e == hipErrorOutOfMemory) return fill_nomem();
	HIPCHK(e);
	FillTot tot{0, 0, 0, 0, 0};
	unsigned long long c[FILL_C_N] = {0, 0, 0, 0, 0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&tot, D.sc + U, sizeof tot, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the wait for the counts
	HIPCHK(hipGetLastError());
	clk.lap(1);
	*n_fbases = tot.len;
	if (n_pieces) *n_pieces = tot.np;
	*stats = kmx_fill_stats{c[FILL_HEAD], c[FILL_PATH], c[FILL_ADJACENT], c[FILL_N], c[FILL_C_NO_ENTRY], c[FILL_C_MIRROR], c[FILL_C_REMOVED], c[FILL_C_FILLED], {0, 0}};
	if (tot.np > 16 * U) return fail(KMX_E_ARG, "internal error: more path pieces than the steps can hold");
	if (S.d_pc_o.ensure(tot.np + 1, st) != hipSuccess || S.d_pc_dst.ensure(tot.np + 1, st) != hipSuccess || S.d_pc_pre.ensure(tot.np + 1, st) != hipSuccess) return fill_nomem();
	D.pc_o = S.d_pc_o; D.pc_dst = S.d_pc_dst; D.pc_pre = S.d_pc_pre; D.n_pc = tot.np; D.pbytes = tot.pb;
	HIPCHK(kmxk::fill_place(D, st));
	clk.lap(2);
	const bool seq_short = tot.len > D.seq_cap, pc_short = D.pieces && tot.np > D.piece_cap;
	if (!seq_short) HIPCHK(kmxk::fill_bytes(D, tot.len, st));
	HIPCHK(hipStreamSynchronize(st));                              // nothing is left in flight
	HIPCHK(hipGetLastError());
	clk.lap(3);
	return seq_short || pc_short ? fill_range(tot.len, D.seq_cap, tot.np, D.piece_cap, seq_short) : (int)KMX_OK;
}

// the sizes and parameters of the kernel block; the pointers are the form's own
static FillDev fill_dev_of(const FillArgs &A)
{
	FillDev D{};
	D.k = A.k; D.kinds = A.params->kinds; D.U = A.U; D.n_ubases = A.n_ubases; D.S = A.S; D.n_plinks = A.n_plinks; D.n_psteps = A.n_psteps; D.seq_cap = A.seq_cap; D.piece_cap = A.piece_cap;
	return D;
}

static int kmx_unitig_scaffold_fill_dev_impl(kmx_model *m, const FillArgs &A)
{
	TRY(fill_args(m, A));
	HIPCHK(hipSetDevice(m->device));
	const hipStream_t st = m->stream;
	if (!A.U) {
		HIPCHK(hipMemsetAsync(A.foffs, 0, 8, st));
		HIPCHK(hipStreamSynchronize(st));
		return KMX_OK;
	}
	FillDev D = fill_dev_of(A);
	D.useq = (const unsigned char *)A.useq; D.uoffs = (const u64 *)A.uoffs; D.srec = (const Scaffold *)A.srec; D.steps = (const ScfStep *)A.steps;
	D.plinks = (const PairLink *)A.plinks; D.precs = (const PairPath *)A.precs; D.psteps = A.psteps;
	D.fseq = (unsigned char *)A.fseq; D.foffs = (u64 *)A.foffs; D.frec = (ScfFill *)A.frec; D.fsteps = (FillStep *)A.fsteps; D.pieces = A.pieces;
	return fill_core(m, D, A.n_fbases, A.n_pieces, A.stats);
}

// srec[S] as kmx_unitig_scaffold leaves it: every scaffold holds a step, its steps lie behind those of the scaffold in front of
// it, and together they are the U steps
static int check_scaffold_steps(const kmx_scaffold *srec, u64 S, u64 U)
{
	if (S && !srec) return fail(KMX_E_ARG, "null argument");
	u64 at = 0;
	for (u64 s = 0; s < S; s++) {
		const u64 n = srec[s].n_steps & ~KMX_SCAFFOLD_CIRCULAR;
		if ((u64)srec[s].first_step + n > U) return fail(KMX_E_ARG, "scaffold %llu: first_step + n_steps = %llu is beyond the %llu steps", (unsigned long long)s, (unsigned long long)(srec[s].first_step + n), (unsigned long long)U);
		if (srec[s].first_step != at || !n) return fail(KMX_E_ARG, "scaffold %llu: its steps do not follow those of the scaffold in front of it", (unsigned long long)s);
		at += n;
	}
	if (at != U) return fail(KMX_E_ARG, "the scaffolds hold %llu steps, not the %llu unitigs", (unsigned long long)at, (unsigned long long)U);
	return KMX_OK;
}

static int kmx_unitig_scaffold_fill_impl(kmx_model *m, FillArgs A)
{
	TRY(check_unitig_count(A.U));
	TRY(check_offsets(A.uoffs, A.U));
	A.n_ubases = A.uoffs[A.U];
	TRY(fill_args(m, A));
	TRY(check_unitig_lengths(A.uoffs, A.U, A.k));
	TRY(check_pair_list(A.plinks, A.n_plinks));
	TRY(check_scaffold_steps(A.srec, A.S, A.U));
	HIPCHK(hipSetDevice(m->device));
	const u64 U = A.U, S = A.S;
	if (!U) {
		A.foffs[0] = 0;
		return KMX_OK;
	}
	Staging G(m, kFillWhat);
	FillDev D = fill_dev_of(A);
	D.piece_cap = std::min<u64>(A.piece_cap, 16 * U);              // the pieces are staged at what always suffices, never beyond the caller's capacity
	D.useq = G.in<unsigned char>(A.useq, A.n_ubases); D.uoffs = G.in<u64>(A.uoffs, U + 1); D.srec = G.in<Scaffold>(A.srec, S); D.steps = G.in<ScfStep>(A.steps, U);
	D.plinks = G.in<PairLink>(A.plinks, A.n_plinks); D.precs = G.in<PairPath>(A.precs, A.n_plinks); D.psteps = G.in<u32>(A.psteps, A.n_psteps);
	D.fseq = G.out<unsigned char>(A.seq_cap); D.foffs = G.out<u64>(S + 1); D.frec = G.out<ScfFill>(S); D.fsteps = G.out<FillStep>(U); D.pieces = A.pieces ? G.out<u32>(D.piece_cap) : nullptr;
	TRY(G.status());
	const int rc = fill_core(m, D, A.n_fbases, A.n_pieces, A.stats);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	if (*A.n_fbases <= A.seq_cap) G.down(A.fseq, D.fseq, *A.n_fbases);
	G.down(A.foffs, D.foffs, S + 1);
	G.down(A.frec, D.frec, S);
	G.down(A.fsteps, D.fsteps, U);
	if (A.pieces) G.down(A.pieces, D.pieces, std::min<u64>(*A.n_pieces, D.piece_cap));
	TRY(G.finish());
	return rc == KMX_OK ? KMX_OK : fill_range(*A.n_fbases, A.seq_cap, A.n_pieces ? *A.n_pieces : 0, A.piece_cap, *A.n_fbases > A.seq_cap);
}

static int kmx_unitig_scaffold_fill_last_phases_impl(kmx_model *m, double *seconds)
{
	if (!m || !seconds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 4; i++) seconds[i] = m->fill.phase_s[i];
	return KMX_OK;
}
