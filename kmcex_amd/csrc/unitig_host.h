// unitig_host.h -- the twelve calls kmx_[count_]unitigs[_dev], kmx_[count_]unitig_graph[_dev], kmx_[count_]unitig_graph_clean[_dev]:
// the compacted de Bruijn graph of a sorted listing, the edges between its unitigs, and the graph after cleaning (the rules:
// include/kmx.h; the kernels: unitig_kernels.h).  Included into kmx_api.hip after count_host.h, whose kept listing the
// kmx_count_* routes read in place.
//
// Every call is unitig_call on three small structs.  UniListing says where the listing is: the caller's, on the host (uploaded
// there, and nowhere else) or on the device, or the counted session's.  UniOut says what is asked for -- the tier: strings,
// strings and links, or the cleaned graph -- where it goes (UniBufs: pointers and capacities, host or device memory), and where
// the counters, removed and stats go.  unitig_call checks the arguments in one order, resolves the listing, runs the first half
// (unitig_rank, or unitig_clean_rounds when the tier cleans), reports the sizes, returns there when this is the sizing call,
// checks the capacities, picks the destination (the caller's device buffers or the handle's staging buffers), runs the second
// half (unitig_emit, and unitig_link_emit when links are wanted) and, for host output, downloads and waits once.
//
// The halves.  unitig_rank validates the listing, builds the adjacency and the links, ranks the 2 n oriented nodes by pointer
// doubling (one stream wait per round: a word says whether anything moved), cuts what is left on cycles and ranks it again, then
// marks the heads and scans the marks: the number of unitigs and of their bytes reach the host.  When links are wanted it also
// counts the edges at the heads and scans the counts (in the copy of the rank state the marks have left free, so no new work
// array), and their total comes with the unitig totals in the same wait.  unitig_emit writes strings, offsets and records,
// unitig_link_emit link_offsets and links.  The work arrays stay on the handle by capacity; nothing here touches the model or
// the listing.
//
// The phase clock (PhaseClock) and the test of k are shared with the later graph calls: graph_host.h.
//
// The phase figures (kmx_*_last_phases) are zeroed once where a call starts its work, and every lap of the phase clock adds to
// them, so a cleaning call's figures are sums over its rounds; only its final emit into the caller's buffers is left out.
static_assert(sizeof(kmx_unitig) == 40 && sizeof(Unitig) == 40, "kmx_unitig is 40 bytes");
static_assert(offsetof(kmx_unitig, min_count) == offsetof(Unitig, min_count) && offsetof(kmx_unitig, first_node) == offsetof(Unitig, first_node) &&
              offsetof(kmx_unitig, circular) == offsetof(Unitig, circular) && offsetof(kmx_unitig, first_fwd) == offsetof(Unitig, first_fwd), "Unitig (kmx_types.h) is the layout of kmx_unitig");
static_assert(sizeof(kmx_clean_params) == 16 && sizeof(kmx_clean_stats) == 64, "kmx_clean_params is 16 bytes, kmx_clean_stats 64");

static const int kUniMaxBits = 26;                             // start[] has at most 2^26 + 1 entries; a bucket of 2^31 entries then holds 32

// a listing: the caller's (k, km, cnt, n), in host memory (host = true: unitig_call uploads it) or on the device, or the
// counted session's (counted = true: unitig_call fills the four from it; who names the entry point for the message)
struct UniListing {
	int k;
	const u64 *km;
	const u32 *cnt;
	u64 n;
	bool host;
	bool counted;
	const char *who;
};
static UniListing uni_listing(int k, const uint64_t *km, const uint32_t *cnt, uint64_t n, bool host) { return UniListing{k, (const u64 *)km, cnt, n, host, false, nullptr}; }
static UniListing uni_counted(const char *who) { return UniListing{0, nullptr, nullptr, 0, false, true, who}; }

// output buffers and their capacities: the caller's (host or device memory) or the handle's staging buffers
struct UniBufs {
	unsigned char *seq;
	u64 seq_cap;
	u64 *offs;                     // [rec_cap + 1]
	Unitig *rec;                   // [rec_cap], or null
	u64 rec_cap;
	u64 *loffs;                    // [2 rec_cap + 1]
	u32 *links;
	u64 link_cap;
};
static UniBufs uni_bufs(char *seq, uint64_t seq_cap, uint64_t *offs, kmx_unitig *rec, uint64_t rec_cap, uint64_t *loffs = nullptr, uint32_t *links = nullptr, uint64_t link_cap = 0)
{
	return UniBufs{(unsigned char *)seq, seq_cap, (u64 *)offs, (Unitig *)rec, rec_cap, (u64 *)loffs, links, link_cap};
}

enum UniTier { kUniStrings, kUniGraph, kUniClean };
// what a call is asked for: the tier, the buffers (host = true: host memory), the counters (n_links: from kUniGraph on) and, for
// kUniClean, the parameters, removed [n] (memory of the buffers' kind, may be null) and stats (host, may be null)
struct UniOut {
	UniTier tier;
	bool host;
	UniBufs b;
	uint64_t *n_uni, *n_bytes, *n_links;
	const kmx_clean_params *clean;
	uint8_t *removed;
	kmx_clean_stats *stats;
};

// what the first half leaves for the second: the view of the work arrays, U.d_pair[cur] the final rank state (U.d_mn the scanned
// marks) and the output's sizes.  With links: U.d_pair[cur ^ 1] + n + 1 holds the scanned link counts, and U.d_succ1 / U.d_pred1
// the head and the tail entry of every unitig.
struct UniRanked {
	UniDev d;
	int cur;
	u64 n_uni, n_bytes, n_links;
};

static int unitig_args(int k, u64 n)
{
	TRY(check_odd_k(k));
	if (n >> 31) return fail(KMX_E_ARG, "%llu listing entries: unitigs take fewer than 2^31", (unsigned long long)n);
	return KMX_OK;
}

static int unitig_clean_args(const kmx_clean_params *p, u32 thr)
{
	if (!p) return fail(KMX_E_ARG, "null cleaning parameters");
	if (!thr) return fail(KMX_E_ARG, "cleaning needs thr >= 1: a removed node is one whose count lies below thr");
	if (!p->ops || (p->ops & ~7u)) return fail(KMX_E_ARG, "ops = %u is no non-empty subset of KMX_CLEAN_TIPS | KMX_CLEAN_ISLANDS | KMX_CLEAN_BUBBLES", p->ops);
	if (!p->max_tip || !p->max_bubble) return fail(KMX_E_ARG, "max_tip and max_bubble are at least 1 k-mer");
	if (p->max_rounds < 1 || p->max_rounds > KMX_CLEAN_MAX_ROUNDS) return fail(KMX_E_ARG, "max_rounds = %u is outside [1, %d]", p->max_rounds, KMX_CLEAN_MAX_ROUNDS);
	return KMX_OK;
}

static int count_unitigs_listing(kmx_model *m, const char *who)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!m->cnt.listed) return fail(KMX_E_STATE, "%s: no listing (kmx_count_finish has not run since the last kmx_count_begin or build)", who);
	return KMX_OK;
}

static int uni_nomem() { return graph_nomem("the unitig construction"); }

// the first half, on a device-resident listing at threshold thr.  On KMX_OK *r is what the second half takes.
static int unitig_rank(kmx_model *m, const UniListing &L, u32 thr, bool links, UniRanked *r)
{
	auto &U = m->uni;
	const u64 n = L.n;
	*r = UniRanked{};
	if (!n) return KMX_OK;
	UniDev *d = &r->d;
	int lg = 0;
	while ((u64(1) << lg) < n) lg++;                               // ceil(log2 n)
	const int T = lg + 1;
	d->km = L.km; d->cnt = L.cnt; d->n = n; d->k = L.k; d->W = (L.k + 31) / 32; d->thr = thr;
	d->bits = std::min({2 * L.k, std::max(lg, 1), kUniMaxBits});
	d->shift = 2 * L.k - d->bits;
	const hipStream_t st = m->stream;
	if (U.d_start.ensure((size_t(1) << d->bits) + 1, st) != hipSuccess || U.d_succ1.ensure(n, st) != hipSuccess || U.d_pred1.ensure(n, st) != hipSuccess ||
	    U.d_deg.ensure(n, st) != hipSuccess || U.d_mn.ensure(4 * n + 4, st) != hipSuccess || U.d_flag.ensure(2 * (size_t)T + 2, st) != hipSuccess ||
	    U.d_pair[0].ensure(2 * n + 2, st) != hipSuccess || U.d_pair[1].ensure(2 * n + 2, st) != hipSuccess)
		return uni_nomem();
	d->start = U.d_start; d->succ1 = U.d_succ1; d->pred1 = U.d_pred1; d->deg = U.d_deg; d->err = U.d_flag;
	HIPCHK(hipMemsetAsync(U.d_flag, 0, (2 * (size_t)T + 2) * 4, st));
	auto word = [&](int i, u32 *v) {                               // one stream wait
		HIPCHK(hipMemcpyAsync(v, U.d_flag.get() + i, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		return (int)KMX_OK;
	};
	PhaseClock clk(m, m->uni.phase_s);
	kmxk::unitig_index(*d, st);
	u32 bad = 0;
	TRY(word(0, &bad));
	if (bad) return fail(KMX_E_ARG, "the listing is not strictly ascending, not canonical, or holds bits above 2k");
	kmxk::unitig_adjacency(*d, st);
	clk.lap(0);
	kmxk::unitig_links(*d, U.d_pair[0], U.d_mn, st);
	clk.lap(1);
	u32 *mn[2] = {U.d_mn.get(), U.d_mn.get() + 2 * n};
	int c = 0;
	bool cycles = false;
	for (int t = 1; t <= T; t++) {
		kmxk::unitig_round(U.d_pair[c], mn[c], U.d_pair[c ^ 1], mn[c ^ 1], n, U.d_flag.get() + t, st);
		c ^= 1;
		U.rounds++;
		u32 moved = 0;
		TRY(word(t, &moved));
		if (!moved) break;
		cycles = t == T;                                           // every path has settled by now: what still moves goes round
	}
	if (cycles) {
		kmxk::unitig_cut(*d, U.d_pair[c], mn[c], U.d_pair[c ^ 1], st);
		c ^= 1;
		u32 moved = 1;
		for (int t = 1; t <= T && moved; t++) {
			kmxk::unitig_round(U.d_pair[c], nullptr, U.d_pair[c ^ 1], nullptr, n, U.d_flag.get() + T + t, st);
			c ^= 1;
			U.rounds++;
			TRY(word(T + t, &moved));
		}
		if (moved) return fail(KMX_E_ARG, "internal error: the cut cycles did not settle");
	}
	clk.lap(2);
	UniTot *sc = (UniTot *)U.d_mn.get();
	const hipError_t e = kmxk::unitig_mark(*d, U.d_pair[c], (UniTot *)U.d_pair[c ^ 1].get(), sc, U.d_tmp, st);
	if (e == hipErrorOutOfMemory) return uni_nomem();
	HIPCHK(e);
	UniTot tot{0, 0};
	u64 n_links = 0;
	HIPCHK(hipMemcpyAsync(&tot, sc + n, sizeof tot, hipMemcpyDeviceToHost, st));
	if (links) {                                                   // the marks' copy of the rank state is free again
		clk.lap(3);
		u64 *lc = U.d_pair[c ^ 1].get();
		const hipError_t el = kmxk::unitig_link_mark(*d, U.d_pair[c], sc, lc, lc + n + 1, U.d_tmp, st);
		if (el == hipErrorOutOfMemory) return uni_nomem();
		HIPCHK(el);
		HIPCHK(hipMemcpyAsync(&n_links, lc + 2 * n + 1, 8, hipMemcpyDeviceToHost, st));
	}
	HIPCHK(hipStreamSynchronize(st));
	clk.lap(links ? 4 : 3);
	r->cur = c;
	r->n_uni = tot.n;
	r->n_bytes = tot.len;
	r->n_links = n_links;
	return KMX_OK;
}

// the second half: enqueued, not awaited (unless the phase clock runs)
static int unitig_emit(kmx_model *m, const UniRanked &r, const UniBufs &b)
{
	if (!r.d.n) { HIPCHK(hipMemsetAsync(b.offs, 0, 8, m->stream)); return KMX_OK; }
	PhaseClock clk(m, m->uni.phase_s);
	kmxk::unitig_emit(r.d, m->uni.d_pair[r.cur], (const UniTot *)m->uni.d_mn.get(), r.n_uni, b.seq, b.seq_cap, b.offs, b.rec, b.rec_cap, m->stream);
	HIPCHK(hipGetLastError());
	clk.lap(3);
	return KMX_OK;
}

// the edges, beside the emit: enqueued, not awaited (unless the phase clock runs)
static int unitig_link_emit(kmx_model *m, const UniRanked &r, const UniBufs &b)
{
	if (!r.d.n) { HIPCHK(hipMemsetAsync(b.loffs, 0, 8, m->stream)); return KMX_OK; }
	PhaseClock clk(m, m->uni.phase_s);
	kmxk::unitig_link_emit(r.d, m->uni.d_pair[r.cur], (const UniTot *)m->uni.d_mn.get(), m->uni.d_pair[r.cur ^ 1].get() + r.d.n + 1, r.n_uni, b.loffs, b.rec_cap, b.links, b.link_cap, m->stream);
	HIPCHK(hipGetLastError());
	clk.lap(4);
	return KMX_OK;
}

// the first half of the cleaning tier: the graph calls' halves run round by round on a working copy of the counts (the rule:
// include/kmx.h).  A round is unitig_rank on (k-mers, working counts, thr), the two emits into the handle's staging buffers
// (records, link_offsets and links; no strings), k_uni_clean and k_uni_drop; its four counters reach the host in one wait.  A
// round that removes nothing leaves the rank state of the final graph standing.  On KMX_OK *S is complete, d_removed[n]
// (device, may be null) holds the round of every removed entry, and *r is what unitig_rank left for the final graph: the emits
// may follow.
static int unitig_clean_rounds(kmx_model *m, const UniListing &L, u32 thr, const kmx_clean_params &P, unsigned char *d_removed, kmx_clean_stats *S, UniRanked *r)
{
	auto &U = m->uni;
	const hipStream_t st = m->stream;
	const u64 n = L.n;
	*S = kmx_clean_stats{0, 0, 0, 0, 0, 0, 0, 0};
	if (n) {
		if (U.d_wcnt.ensure(n, st) != hipSuccess || U.d_cctr.ensure(4, st) != hipSuccess) return uni_nomem();
		HIPCHK(hipMemcpyAsync(U.d_wcnt, L.cnt, n * 4, hipMemcpyDeviceToDevice, st));
		if (d_removed) HIPCHK(hipMemsetAsync(d_removed, 0, n, st));
	}
	UniListing W = L;
	W.cnt = U.d_wcnt;
	for (u32 round = 1;; round++) {
		TRY(unitig_rank(m, W, thr, true, r));
		if (round == 1) { S->n_unitigs_before = r->n_uni; S->n_links_before = r->n_links; }
		if (round > P.max_rounds) { S->rounds_run = P.max_rounds; S->converged = 0; break; }   // the last round still removed something
		if (!r->n_uni) { S->rounds_run = round; S->converged = 1; break; }
		const u64 nu = r->n_uni, nl = r->n_links;
		if (U.d_offs.ensure(nu + 1, st) != hipSuccess || U.d_rec.ensure(nu, st) != hipSuccess || U.d_loffs.ensure(2 * nu + 1, st) != hipSuccess ||
		    U.d_links.ensure(nl, st) != hipSuccess || U.d_verdict.ensure(nu, st) != hipSuccess) return uni_nomem();
		const UniBufs staged{nullptr, 0, U.d_offs, U.d_rec, nu, U.d_loffs, U.d_links, nl};      // the records only: no byte of a string is stored
		TRY(unitig_emit(m, *r, staged));
		TRY(unitig_link_emit(m, *r, staged));
		PhaseClock clk(m, m->uni.phase_s);
		HIPCHK(hipMemsetAsync(U.d_cctr, 0, 4 * sizeof(unsigned long long), st));
		const UniClean c{U.d_rec, U.d_loffs, U.d_links, nu, nl, P.ops, P.max_tip, P.max_bubble};
		kmxk::unitig_clean(c, U.d_verdict, U.d_cctr, st);
		kmxk::unitig_drop(r->d, U.d_pair[r->cur], (const UniTot *)U.d_mn.get(), U.d_verdict, nu, U.d_wcnt, d_removed, (unsigned char)round, U.d_cctr, st);
		HIPCHK(hipGetLastError());
		unsigned long long ctr[4] = {0, 0, 0, 0};
		HIPCHK(hipMemcpyAsync(ctr, U.d_cctr, sizeof ctr, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));                            // the round's one wait beyond the ranking's own
		clk.lap(5);
		S->n_tips += ctr[0]; S->n_islands += ctr[1]; S->n_bubbles += ctr[2]; S->n_kmers_removed += ctr[3];
		if (!ctr[3]) { S->rounds_run = round; S->converged = 1; break; }
	}
	return KMX_OK;
}

// every call: see the head of the file
static int unitig_call(kmx_model *m, UniListing L, u32 thr, const UniOut &o)
{
	const bool links = o.tier != kUniStrings, clean = o.tier == kUniClean;
	const UniBufs &b = o.b;
	if (L.counted) {
		TRY(count_unitigs_listing(m, L.who));
		L.k = m->cnt.k; L.km = m->cnt.d_run[1]; L.cnt = m->cnt.d_runc[1]; L.n = m->cnt.n_list;
	} else if (!m)
		return fail(KMX_E_ARG, "null model");
	if (!o.n_uni || !o.n_bytes || (links && !o.n_links)) return fail(KMX_E_ARG, "null argument");
	*o.n_uni = *o.n_bytes = 0;
	if (links) *o.n_links = 0;
	if (clean && o.stats) *o.stats = kmx_clean_stats{0, 0, 0, 0, 0, 0, 0, 0};
	TRY(unitig_args(L.k, L.n));
	if (clean) TRY(unitig_clean_args(o.clean, thr));
	if ((L.n && (!L.km || !L.cnt)) || (b.seq && (!b.offs || (links && (!b.loffs || !b.links))))) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	auto &U = m->uni;
	const hipStream_t st = m->stream;
	const u64 n = L.n;
	for (double &s : U.phase_s) s = 0;
	U.rounds = 0;
	if (L.host && n) {                                             // the caller's listing, uploaded
		const u64 W = (u64)(L.k + 31) / 32;
		if (U.d_km.ensure(n * W, st) != hipSuccess || U.d_cnt.ensure(n, st) != hipSuccess) return uni_nomem();
		HIPCHK(hipMemcpyAsync(U.d_km, L.km, n * W * 8, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(U.d_cnt, L.cnt, n * 4, hipMemcpyHostToDevice, st));
		L.km = U.d_km; L.cnt = U.d_cnt;
	}
	UniRanked r{};
	if (clean) {
		const bool staged = o.host && o.removed && n;
		if (staged && U.d_removed.ensure(n, st) != hipSuccess) return uni_nomem();
		kmx_clean_stats S;
		TRY(unitig_clean_rounds(m, L, thr, *o.clean, o.host ? (staged ? U.d_removed.get() : nullptr) : o.removed, &S, &r));
		if (o.stats) *o.stats = S;
		if (staged) {
			HIPCHK(hipMemcpyAsync(o.removed, U.d_removed, n, hipMemcpyDeviceToHost, st));
			HIPCHK(hipStreamSynchronize(st));
		}
	} else
		TRY(unitig_rank(m, L, thr, links, &r));
	const u64 nu = r.n_uni, nb = r.n_bytes, nl = r.n_links;
	*o.n_uni = nu;
	*o.n_bytes = nb;
	if (links) *o.n_links = nl;
	if (!b.seq) return KMX_OK;                                     // the sizing call
	if (nu > b.rec_cap || nb > b.seq_cap || (links && nl > b.link_cap)) {
		if (!links) return fail(KMX_E_RANGE, "%llu unitigs of %llu bytes, the buffers hold %llu and %llu", (unsigned long long)nu, (unsigned long long)nb, (unsigned long long)b.rec_cap, (unsigned long long)b.seq_cap);
		return fail(KMX_E_RANGE, "%llu unitigs of %llu bytes with %llu links, the buffers hold %llu, %llu and %llu", (unsigned long long)nu, (unsigned long long)nb, (unsigned long long)nl,
		            (unsigned long long)b.rec_cap, (unsigned long long)b.seq_cap, (unsigned long long)b.link_cap);
	}
	UniBufs dst = b;                                               // the caller's device buffers, or the handle's staging buffers with exact room
	if (o.host) {
		if (U.d_seq.ensure(nb, st) != hipSuccess || U.d_offs.ensure(nu + 1, st) != hipSuccess || (b.rec && U.d_rec.ensure(nu, st) != hipSuccess) ||
		    (links && (U.d_loffs.ensure(2 * nu + 1, st) != hipSuccess || U.d_links.ensure(nl, st) != hipSuccess)))
			return uni_nomem();
		dst = UniBufs{U.d_seq, nb, U.d_offs, b.rec ? U.d_rec.get() : nullptr, nu, U.d_loffs, U.d_links, nl};
	}
	double rounds_s[6];                                            // a cleaning call's figures are its rounds': this emit is not added
	std::copy(U.phase_s, U.phase_s + 6, rounds_s);
	int rc = unitig_emit(m, r, dst);
	if (rc == KMX_OK && links) rc = unitig_link_emit(m, r, dst);
	if (clean) std::copy(rounds_s, rounds_s + 6, U.phase_s);
	TRY(rc);
	if (!o.host) return KMX_OK;
	if (nb) HIPCHK(hipMemcpyAsync(b.seq, dst.seq, nb, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(b.offs, dst.offs, (nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (b.rec && nu) HIPCHK(hipMemcpyAsync(b.rec, dst.rec, nu * sizeof(Unitig), hipMemcpyDeviceToHost, st));
	if (links) HIPCHK(hipMemcpyAsync(b.loffs, dst.loffs, (2 * nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (links && nl) HIPCHK(hipMemcpyAsync(b.links, dst.links, nl * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

// ---- the twelve entry points: tier x (the caller's listing | the counted session's) x (host | device buffers)
static int kmx_unitigs_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, char *d_seq_out, uint64_t seq_capacity,
                                uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	return unitig_call(m, uni_listing(k, d_kmers, d_counts, n, false), thr,
	                   UniOut{kUniStrings, false, uni_bufs(d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity), n_unitigs, n_bases_out, nullptr, nullptr, nullptr, nullptr});
}

static int kmx_unitigs_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, char *seq_out, uint64_t seq_capacity,
                            uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	return unitig_call(m, uni_listing(k, kmers, counts, n, true), thr,
	                   UniOut{kUniStrings, true, uni_bufs(seq_out, seq_capacity, offsets_out, rec, rec_capacity), n_unitigs, n_bases_out, nullptr, nullptr, nullptr, nullptr});
}

static int kmx_count_unitigs_dev_impl(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity,
                                      uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	return unitig_call(m, uni_counted("kmx_count_unitigs_dev"), thr,
	                   UniOut{kUniStrings, false, uni_bufs(d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity), n_unitigs, n_bases_out, nullptr, nullptr, nullptr, nullptr});
}

static int kmx_count_unitigs_impl(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity,
                                  uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	return unitig_call(m, uni_counted("kmx_count_unitigs"), thr,
	                   UniOut{kUniStrings, true, uni_bufs(seq_out, seq_capacity, offsets_out, rec, rec_capacity), n_unitigs, n_bases_out, nullptr, nullptr, nullptr, nullptr});
}

// ... with link_offsets [2 rec_cap + 1] and links [link_cap]
static int kmx_unitig_graph_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, char *d_seq_out, uint64_t seq_capacity,
                                     uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity,
                                     uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	return unitig_call(m, uni_listing(k, d_kmers, d_counts, n, false), thr,
	                   UniOut{kUniGraph, false, uni_bufs(d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity), n_unitigs, n_bases_out, n_links, nullptr, nullptr, nullptr});
}

static int kmx_unitig_graph_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, char *seq_out, uint64_t seq_capacity,
                                 uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity,
                                 uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	return unitig_call(m, uni_listing(k, kmers, counts, n, true), thr,
	                   UniOut{kUniGraph, true, uni_bufs(seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity), n_unitigs, n_bases_out, n_links, nullptr, nullptr, nullptr});
}

static int kmx_count_unitig_graph_dev_impl(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity,
                                           uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	return unitig_call(m, uni_counted("kmx_count_unitig_graph_dev"), thr,
	                   UniOut{kUniGraph, false, uni_bufs(d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity), n_unitigs, n_bases_out, n_links, nullptr, nullptr, nullptr});
}

static int kmx_count_unitig_graph_impl(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity,
                                       uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	return unitig_call(m, uni_counted("kmx_count_unitig_graph"), thr,
	                   UniOut{kUniGraph, true, uni_bufs(seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity), n_unitigs, n_bases_out, n_links, nullptr, nullptr, nullptr});
}

// ... after cleaning under params, with removed [n] and stats
static int kmx_unitig_graph_clean_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, const kmx_clean_params *params, char *d_seq_out,
                                           uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links,
                                           uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *d_removed, kmx_clean_stats *stats)
{
	return unitig_call(m, uni_listing(k, d_kmers, d_counts, n, false), thr,
	                   UniOut{kUniClean, false, uni_bufs(d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity), n_unitigs, n_bases_out, n_links, params, d_removed, stats});
}

static int kmx_unitig_graph_clean_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, const kmx_clean_params *params, char *seq_out,
                                       uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity,
                                       uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *removed, kmx_clean_stats *stats)
{
	return unitig_call(m, uni_listing(k, kmers, counts, n, true), thr,
	                   UniOut{kUniClean, true, uni_bufs(seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity), n_unitigs, n_bases_out, n_links, params, removed, stats});
}

static int kmx_count_unitig_graph_clean_dev_impl(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec,
                                                 uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out,
                                                 uint64_t *n_links, uint8_t *d_removed, kmx_clean_stats *stats)
{
	return unitig_call(m, uni_counted("kmx_count_unitig_graph_clean_dev"), thr,
	                   UniOut{kUniClean, false, uni_bufs(d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity), n_unitigs, n_bases_out, n_links, params, d_removed, stats});
}

static int kmx_count_unitig_graph_clean_impl(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec,
                                             uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out,
                                             uint64_t *n_links, uint8_t *removed, kmx_clean_stats *stats)
{
	return unitig_call(m, uni_counted("kmx_count_unitig_graph_clean"), thr,
	                   UniOut{kUniClean, true, uni_bufs(seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity), n_unitigs, n_bases_out, n_links, params, removed, stats});
}

// the phase figures of the last call on this handle, measured only under kmx_set_profile(m, 1): seconds[0 .. 3] adjacency (with
// validation and the index), links, ranking, emit (with the marks and their scan); [4] the links between unitigs (their counts
// and scan, the links kernel), 0 after a call that asked for no edges; [5] a cleaning call's decisions and removal.  A cleaning
// call's figures are sums over its rounds.  *rounds: the call's doubling rounds, summed likewise.
static int uni_last_phases(kmx_model *m, double *seconds, uint64_t *rounds, int figures)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	std::copy(m->uni.phase_s, m->uni.phase_s + figures, seconds);
	*rounds = m->uni.rounds;
	return KMX_OK;
}
static int kmx_unitigs_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds) { return uni_last_phases(m, seconds, rounds, 4); }
static int kmx_unitig_graph_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds) { return uni_last_phases(m, seconds, rounds, 5); }
static int kmx_unitig_clean_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds) { return uni_last_phases(m, seconds, rounds, 6); }
