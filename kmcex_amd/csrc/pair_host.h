// pair_host.h -- kmx_unitig_pair_walks[_dev]: the two mates of every read pair placed in the unitig graph (the rule:
// include/kmx.h; the kernels: pair_kernels.h; the launcher: unitig_device.hip).  Included into kmx_api.hip after resolve_host.h.
//
// pair_core runs the pass on device buffers, inside the map session: the anchors, the work items of the fold and the merged
// records stay on the session by capacity (kmx_model::map) and go with kmx_unitig_map_end; everything is enqueued on the model's
// stream, and ONE wait brings the counters and the merged count to the host.  The merged list reaches the caller's buffer by a
// launch that reads the count on the device, so a list that does not fit is never touched.  The _dev form checks what can be
// checked without reading a buffer; the host form validates walk_offsets, the CSR and the input list, stages its input and
// zeroed copies of hist and pair_hits for the length of the call, downloads and adds.  The CSR and buffer checks and the staging
// owner (Staging) are shared: graph_host.h.
static_assert(sizeof(kmx_pair_params) == 16 && sizeof(kmx_pair) == 64 && sizeof(Pair) == 64 && sizeof(kmx_pair_link) == 32 && sizeof(PairLink) == 32 && sizeof(kmx_pair_stats) == 80,
              "kmx_pair_params is 16 bytes, kmx_pair 64, kmx_pair_link 32, kmx_pair_stats 80");
static_assert(offsetof(kmx_pair, walk_b) == offsetof(Pair, walk_b) && offsetof(kmx_pair, cls) == offsetof(Pair, cls) && offsetof(kmx_pair, edge) == offsetof(Pair, edge) &&
              offsetof(kmx_pair, oa) == offsetof(Pair, oa) && offsetof(kmx_pair, xb) == offsetof(Pair, xb) && offsetof(kmx_pair, d) == offsetof(Pair, d) &&
              offsetof(kmx_pair, frag) == offsetof(Pair, frag) && offsetof(kmx_pair, reserved) == offsetof(Pair, reserved) && offsetof(kmx_pair, reserved) == 56,
              "Pair (kmx_types.h) is the layout of kmx_pair");
static_assert(offsetof(kmx_pair_link, b) == offsetof(PairLink, b) && offsetof(kmx_pair_link, n_pairs) == offsetof(PairLink, n_pairs) && offsetof(kmx_pair_link, sum_dist) == offsetof(PairLink, sum_dist) &&
              offsetof(kmx_pair_link, min_dist) == offsetof(PairLink, min_dist) && offsetof(kmx_pair_link, max_dist) == offsetof(PairLink, max_dist) && offsetof(kmx_pair_link, max_dist) == 28,
              "PairLink (kmx_types.h) is the layout of kmx_pair_link");
static_assert(KMX_PAIR_NONE == PAIR_NONE && KMX_PAIR_SINGLE == PAIR_SINGLE && KMX_PAIR_SAME == PAIR_SAME && KMX_PAIR_INVERTED == PAIR_INVERTED && KMX_PAIR_LINK == PAIR_LINK && KMX_PAIR_FAR == PAIR_FAR,
              "the classes of kmx_types.h are KMX_PAIR_*");

// the buffers of one call: what both forms check before anything runs
struct PairArgs {
	const kmx_walk *walks; u64 n_walks;
	const uint64_t *wo; u64 n_seqs;
	const uint32_t *steps; u64 n_steps;
	const uint64_t *loffs; const uint32_t *links; u64 n_links;
	const kmx_pair_params *params;
	kmx_pair *pairs; uint64_t *hist, *pair_hits;
	kmx_pair_link *plinks; u64 capacity; uint64_t *n_plinks;
	kmx_pair_stats *stats;
};

static int pair_args(kmx_model *m, const char *who, const PairArgs &A)
{
	TRY(map_session(m, who));
	const kmx_pair_params *p = A.params;
	if (!p || !A.stats) return fail(KMX_E_ARG, "null argument");
	if (A.n_seqs & 1) return fail(KMX_E_ARG, "n_seqs = %llu is odd: reads 2 p and 2 p + 1 are the mates of pair p", (unsigned long long)A.n_seqs);
	if (!p->bin_width) return fail(KMX_E_ARG, "bin_width = 0");
	if (p->n_bins < 1 || p->n_bins > 65536) return fail(KMX_E_ARG, "n_bins = %u: in [1, 65536]", p->n_bins);
	if (A.plinks && !A.n_plinks) return fail(KMX_E_ARG, "null argument");
	if (A.plinks && *A.n_plinks > A.capacity) return fail(KMX_E_ARG, "the list holds %llu entries, more than its capacity %llu", (unsigned long long)*A.n_plinks, (unsigned long long)A.capacity);
	*A.stats = kmx_pair_stats{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (!A.n_seqs) return KMX_OK;
	if (!A.wo || !A.loffs || (A.n_walks && !A.walks) || (A.n_steps && !A.steps) || (A.n_links && !A.links)) return fail(KMX_E_ARG, "null argument");
	const u64 U = m->map.dev.U, np = A.n_seqs / 2;
	Span s[6] = {{A.walks, A.n_walks * sizeof(kmx_walk), false}, {A.wo, (A.n_seqs + 1) * 8, false}, {A.steps, A.n_steps * 4, false}, {A.loffs, (2 * U + 1) * 8, false}, {A.links, A.n_links * 4, false}, {}};
	const Span out[4] = {opt_span(A.pairs, np * sizeof(kmx_pair), true), opt_span(A.hist, (u64)p->n_bins * 8, true), opt_span(A.pair_hits, A.n_links * 8, true), opt_span(A.plinks, A.capacity * sizeof(kmx_pair_link), true)};
	for (const Span &o : out) {                                    // every output against the inputs: two outputs are not compared
		s[5] = o;
		TRY(check_spans(s, 6));
	}
	return KMX_OK;
}

static int pair_range(u64 need, u64 cap) { return fail(KMX_E_RANGE, "%llu pair links, the list holds %llu", (unsigned long long)need, (unsigned long long)cap); }

// the pass on device buffers (D: input, parameters and output; the session's part and the work arrays are filled in here);
// D.n_pairs > 0.  *merged: the entries of the merged list (0 without one), which the device has stored iff they fit D.cap
static int pair_core(kmx_model *m, PairDev D, kmx_pair_stats *stats, u64 *merged)
{
	auto &S = m->map;
	const hipStream_t st = m->stream;
	D.n_items = D.plinks ? D.n_in + D.n_pairs : 0;
	if (S.d_panchor.ensure(D.n_seqs, st) != hipSuccess || S.d_pcnt.ensure(PAIR_C_N, st) != hipSuccess) return map_nomem();
	if (D.n_items && (S.d_pkey.ensure(4 * D.n_items, st) != hipSuccess || S.d_pdist.ensure(D.n_pairs, st) != hipSuccess || S.d_psc.ensure(D.n_items + 1, st) != hipSuccess ||
	                  S.d_pmrg.ensure(D.n_items, st) != hipSuccess))
		return map_nomem();
	D.mu = S.dev.mu; D.U = S.dev.U; D.k = S.dev.d.k;
	D.anchor = S.d_panchor; D.cnt = S.d_pcnt;
	if (D.n_items) {
		D.key = S.d_pkey; D.idx = D.key + D.n_items; D.skey = D.idx + D.n_items; D.sidx = D.skey + D.n_items;
		D.dist = S.d_pdist; D.sc = S.d_psc; D.mrg = S.d_pmrg;
	}
	const hipError_t e = kmxk::pair_walks(D, S.d_tmp, st);
	if (e != hipSuccess) return map_dev_fail(e);
	unsigned long long c[PAIR_C_N] = {0, 0, 0, 0, 0, 0, 0, 0};
	u64 tot = 0;
	HIPCHK(hipMemcpyAsync(c, D.cnt, sizeof c, hipMemcpyDeviceToHost, st));
	if (D.n_items) HIPCHK(hipMemcpyAsync(&tot, D.sc + D.n_items, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));                              // the call's one wait
	HIPCHK(hipGetLastError());
	*stats = kmx_pair_stats{D.n_pairs, c[PAIR_C_NONE], c[PAIR_C_SINGLE], c[PAIR_C_SAME], c[PAIR_C_NEGATIVE], c[PAIR_C_INVERTED], c[PAIR_C_LINK], c[PAIR_C_ADJACENT], c[PAIR_C_FAR], 0};
	*merged = tot;
	return KMX_OK;
}

static PairDev pair_dev_of(const PairArgs &A)
{
	PairDev D{};
	D.n_walks = A.n_walks; D.n_seqs = A.n_seqs; D.n_pairs = A.n_seqs / 2; D.n_steps = A.n_steps; D.n_links = A.n_links;
	D.min_mapped = A.params->min_mapped; D.max_dist = A.params->max_dist; D.bin_width = A.params->bin_width; D.n_bins = A.params->n_bins;
	D.cap = A.plinks ? A.capacity : 0; D.n_in = A.plinks ? *A.n_plinks : 0;
	return D;
}

static int kmx_unitig_pair_walks_dev_impl(kmx_model *m, const PairArgs &A)
{
	TRY(pair_args(m, "kmx_unitig_pair_walks_dev", A));
	if (!A.n_seqs) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	PairDev D = pair_dev_of(A);
	D.walks = (const Walk *)A.walks; D.wo = (const u64 *)A.wo; D.steps = A.steps; D.loffs = (const u64 *)A.loffs; D.links = A.links;
	D.pairs = (Pair *)A.pairs; D.hist = (unsigned long long *)A.hist; D.pair_hits = A.n_links ? (unsigned long long *)A.pair_hits : nullptr; D.plinks = (PairLink *)A.plinks;
	u64 merged = 0;
	TRY(pair_core(m, D, A.stats, &merged));
	if (!A.plinks) return KMX_OK;
	*A.n_plinks = merged;
	return merged > A.capacity ? pair_range(merged, A.capacity) : KMX_OK;
}

static int kmx_unitig_pair_walks_impl(kmx_model *m, const PairArgs &A)
{
	TRY(pair_args(m, "kmx_unitig_pair_walks", A));
	if (!A.n_seqs) return KMX_OK;
	const u64 U = m->map.dev.U, np = A.n_seqs / 2, n_in = A.plinks ? *A.n_plinks : 0, nb = A.params->n_bins;
	TRY(check_offsets(A.wo, A.n_seqs));
	if (A.wo[A.n_seqs] != A.n_walks) return fail(KMX_E_ARG, "walk_offsets end at %llu, not at n_walks = %llu", (unsigned long long)A.wo[A.n_seqs], (unsigned long long)A.n_walks);
	TRY(check_link_csr(A.loffs, A.links, A.n_links, U, false));
	TRY(check_pair_list(A.plinks, n_in));
	HIPCHK(hipSetDevice(m->device));
	Staging G(m, kMapWhat);
	PairDev D = pair_dev_of(A);
	D.cap = A.plinks ? std::min<u64>(A.capacity, n_in + np) : 0;      // the merge never needs more
	D.walks = G.in<Walk>(A.walks, A.n_walks); D.wo = G.in<u64>(A.wo, A.n_seqs + 1); D.steps = G.in<u32>(A.steps, A.n_steps); D.loffs = G.in<u64>(A.loffs, 2 * U + 1);
	D.links = G.in<u32>(A.links, A.n_links);
	if (A.pairs) D.pairs = G.out<Pair>(np);
	if (A.hist) D.hist = G.zeroed<unsigned long long>(nb);
	if (A.pair_hits && A.n_links) D.pair_hits = G.zeroed<unsigned long long>(A.n_links);
	if (A.plinks) D.plinks = G.in<PairLink>(A.plinks, n_in, D.cap);
	TRY(G.status());
	u64 merged = 0;
	TRY(pair_core(m, D, A.stats, &merged));
	G.down(A.pairs, D.pairs, D.pairs ? np : 0);
	G.down_add(A.hist, D.hist, D.hist ? nb : 0);
	G.down_add(A.pair_hits, D.pair_hits, D.pair_hits ? A.n_links : 0);
	const bool fits = A.plinks && merged <= A.capacity;               // merged <= n_in + np always, so then it also fits D.cap
	if (fits) G.down(A.plinks, D.plinks, merged);
	TRY(G.finish());
	if (!A.plinks) return KMX_OK;
	*A.n_plinks = merged;
	return fits ? KMX_OK : pair_range(merged, A.capacity);
}
