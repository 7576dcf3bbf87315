// unitig_host.h -- kmx_unitigs*, kmx_count_unitigs*: the compacted de Bruijn graph of a sorted listing (the rule: include/kmx.h;
// the kernels: unitig_kernels.h).  Included into kmx_api.hip after count_host.h, whose kept listing kmx_count_unitigs* read in
// place.
//
// A call is two halves.  unitig_rank validates the listing, builds the adjacency and the links, ranks the 2 n oriented nodes by
// pointer doubling (one stream wait per round: a word says whether anything moved), cuts what is left on cycles and ranks it
// again, then marks the heads and scans the marks: the number of unitigs and of their bytes reach the host.  unitig_emit writes
// strings, offsets and records.  Between the halves the device variant checks the caller's capacities and the host variant
// sizes its own output.  The work arrays stay on the handle by capacity; nothing here touches the model or the listing.
//
// kmx_unitig_graph*, kmx_count_unitig_graph* are the same calls with the edges between unitigs: the first half also counts the
// edges at the heads and scans the counts (in the copy of the rank state the marks have left free, so no new work array), and
// their total comes with the unitig totals in the same wait; the second half also writes link_offsets and links.
static_assert(sizeof(kmx_unitig) == 40 && sizeof(Unitig) == 40, "kmx_unitig is 40 bytes");
static_assert(offsetof(kmx_unitig, min_count) == offsetof(Unitig, min_count) && offsetof(kmx_unitig, first_node) == offsetof(Unitig, first_node) &&
              offsetof(kmx_unitig, circular) == offsetof(Unitig, circular) && offsetof(kmx_unitig, first_fwd) == offsetof(Unitig, first_fwd), "Unitig (kmx_types.h) is the layout of kmx_unitig");

static const int kUniMaxBits = 26;                             // start[] has at most 2^26 + 1 entries; a bucket of 2^31 entries then holds 32

static int unitig_args(int k, u64 n)
{
	if (k < 5 || k > 63 || !(k & 1)) return fail(KMX_E_ARG, "unitigs need an odd k in [5, 63], not %d (an even k has k-mers that are their own reverse complement)", k);
	if (n >> 31) return fail(KMX_E_ARG, "%llu listing entries: unitigs take fewer than 2^31", (unsigned long long)n);
	return KMX_OK;
}

static int uni_nomem() { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of the unitig construction could not be allocated"); }

// a lap of the phase clock: only under kmx_set_profile(m, 1), where every phase waits for the stream
struct UniClock {
	kmx_model *m;
	std::chrono::steady_clock::time_point t0;
	explicit UniClock(kmx_model *mm) : m(mm) { if (m->prof.on) { hipStreamSynchronize(m->stream); t0 = std::chrono::steady_clock::now(); } }
	void lap(int phase)
	{
		if (!m->prof.on) return;
		hipStreamSynchronize(m->stream);
		const auto t1 = std::chrono::steady_clock::now();
		m->uni.phase_s[phase] += std::chrono::duration<double>(t1 - t0).count();
		t0 = t1;
	}
};

// the first half, on a device-resident listing.  On KMX_OK *n_uni / *n_bytes are the output's sizes, U.d_pair[*cur] the final
// rank state, U.d_mn the scanned marks, and *d is the view the second half takes.  n_links (null: no edges are asked for): the
// number of edges between unitigs; U.d_pair[*cur ^ 1] + n + 1 then holds the scanned link counts, and U.d_succ1 / U.d_pred1
// the head and the tail entry of every unitig.
static int unitig_rank(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, UniDev *d, int *cur, u64 *n_uni, u64 *n_bytes, u64 *n_links = nullptr)
{
	auto &U = m->uni;
	for (double &s : U.phase_s) s = 0;
	U.rounds = 0;
	*n_uni = *n_bytes = 0;
	if (n_links) *n_links = 0;
	*cur = 0;
	if (!n) return KMX_OK;
	int lg = 0;
	while ((u64(1) << lg) < n) lg++;                               // ceil(log2 n)
	const int T = lg + 1;
	d->km = d_km; d->cnt = d_cnt; d->n = n; d->k = k; d->W = (k + 31) / 32; d->thr = thr;
	d->bits = std::min({2 * k, std::max(lg, 1), kUniMaxBits});
	d->shift = 2 * k - d->bits;
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
	UniClock clk(m);
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
	HIPCHK(hipMemcpyAsync(&tot, sc + n, sizeof tot, hipMemcpyDeviceToHost, st));
	if (n_links) {                                                 // the marks' copy of the rank state is free again
		clk.lap(3);
		u64 *lc = U.d_pair[c ^ 1].get();
		const hipError_t el = kmxk::unitig_link_mark(*d, U.d_pair[c], sc, lc, lc + n + 1, U.d_tmp, st);
		if (el == hipErrorOutOfMemory) return uni_nomem();
		HIPCHK(el);
		HIPCHK(hipMemcpyAsync(n_links, lc + 2 * n + 1, 8, hipMemcpyDeviceToHost, st));
	}
	HIPCHK(hipStreamSynchronize(st));
	clk.lap(n_links ? 4 : 3);
	*cur = c;
	*n_uni = tot.n;
	*n_bytes = tot.len;
	return KMX_OK;
}

// the second half: enqueued, not awaited (unless the phase clock runs)
static int unitig_emit(kmx_model *m, const UniDev &d, int cur, u64 n, u64 n_uni, unsigned char *d_seq, u64 seq_cap, u64 *d_offs, Unitig *d_rec, u64 rec_cap)
{
	if (!n) { HIPCHK(hipMemsetAsync(d_offs, 0, 8, m->stream)); return KMX_OK; }
	UniClock clk(m);
	kmxk::unitig_emit(d, m->uni.d_pair[cur], (const UniTot *)m->uni.d_mn.get(), n_uni, d_seq, seq_cap, d_offs, d_rec, rec_cap, m->stream);
	HIPCHK(hipGetLastError());
	clk.lap(3);
	return KMX_OK;
}

// the edges, beside the emit: enqueued, not awaited (unless the phase clock runs)
static int unitig_link_emit(kmx_model *m, const UniDev &d, int cur, u64 n, u64 n_uni, u64 *d_loffs, u64 rec_cap, u32 *d_links, u64 link_cap)
{
	if (!n) { HIPCHK(hipMemsetAsync(d_loffs, 0, 8, m->stream)); return KMX_OK; }
	UniClock clk(m);
	kmxk::unitig_link_emit(d, m->uni.d_pair[cur], (const UniTot *)m->uni.d_mn.get(), m->uni.d_pair[cur ^ 1].get() + n + 1, n_uni, d_loffs, rec_cap, d_links, link_cap, m->stream);
	HIPCHK(hipGetLastError());
	clk.lap(4);
	return KMX_OK;
}

static int uni_range(u64 nu, u64 nb, u64 nl, u64 rec_cap, u64 seq_cap, u64 link_cap)
{
	return fail(KMX_E_RANGE, "%llu unitigs of %llu bytes with %llu links, the buffers hold %llu, %llu and %llu", (unsigned long long)nu, (unsigned long long)nb, (unsigned long long)nl,
	            (unsigned long long)rec_cap, (unsigned long long)seq_cap, (unsigned long long)link_cap);
}

static int unitigs_dev_core(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, char *d_seq_out, u64 seq_cap, u64 *d_offs_out, kmx_unitig *d_rec, u64 rec_cap,
                            uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	if (!n_unitigs || !n_bases_out) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = 0;
	TRY(unitig_args(k, n));
	if ((n && (!d_km || !d_cnt)) || (d_seq_out && !d_offs_out)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	UniDev d{};
	int cur = 0;
	u64 nu = 0, nb = 0;
	TRY(unitig_rank(m, k, d_km, d_cnt, n, thr, &d, &cur, &nu, &nb));
	*n_unitigs = nu;
	*n_bases_out = nb;
	if (!d_seq_out) return KMX_OK;                                 // the sizing call
	if (nu > rec_cap || nb > seq_cap)
		return fail(KMX_E_RANGE, "%llu unitigs of %llu bytes, the buffers hold %llu and %llu", (unsigned long long)nu, (unsigned long long)nb, (unsigned long long)rec_cap, (unsigned long long)seq_cap);
	return unitig_emit(m, d, cur, n, nu, (unsigned char *)d_seq_out, seq_cap, d_offs_out, (Unitig *)d_rec, rec_cap);
}

static int kmx_unitigs_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, char *d_seq_out, uint64_t seq_capacity,
                                uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	return unitigs_dev_core(m, k, (const u64 *)d_kmers, d_counts, n, thr, d_seq_out, seq_capacity, (u64 *)d_offsets_out, d_rec, rec_capacity, n_unitigs, n_bases_out);
}

// host buffers around a device-resident listing (the caller's, uploaded: up = true; or the session's)
static int unitigs_host_core(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, char *seq_out, u64 seq_cap, uint64_t *offs_out, kmx_unitig *rec, u64 rec_cap,
                             uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	auto &U = m->uni;
	UniDev d{};
	int cur = 0;
	u64 nu = 0, nb = 0;
	TRY(unitig_rank(m, k, d_km, d_cnt, n, thr, &d, &cur, &nu, &nb));
	*n_unitigs = nu;
	*n_bases_out = nb;
	if (!seq_out) return KMX_OK;
	if (nu > rec_cap || nb > seq_cap)
		return fail(KMX_E_RANGE, "%llu unitigs of %llu bytes, the buffers hold %llu and %llu", (unsigned long long)nu, (unsigned long long)nb, (unsigned long long)rec_cap, (unsigned long long)seq_cap);
	const hipStream_t st = m->stream;
	if (U.d_seq.ensure(nb, st) != hipSuccess || U.d_offs.ensure(nu + 1, st) != hipSuccess || (rec && U.d_rec.ensure(nu, st) != hipSuccess)) return uni_nomem();
	TRY(unitig_emit(m, d, cur, n, nu, U.d_seq, nb, U.d_offs, rec ? U.d_rec.get() : nullptr, nu));
	if (nb) HIPCHK(hipMemcpyAsync(seq_out, U.d_seq, nb, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(offs_out, U.d_offs, (nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (rec && nu) HIPCHK(hipMemcpyAsync(rec, U.d_rec, nu * sizeof(Unitig), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

static int kmx_unitigs_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, char *seq_out, uint64_t seq_capacity,
                            uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	if (!m || !n_unitigs || !n_bases_out) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = 0;
	TRY(unitig_args(k, n));
	if ((n && (!kmers || !counts)) || (seq_out && !offsets_out)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	auto &U = m->uni;
	const u64 W = (u64)(k + 31) / 32;
	if (n) {
		if (U.d_km.ensure(n * W, m->stream) != hipSuccess || U.d_cnt.ensure(n, m->stream) != hipSuccess) return uni_nomem();
		HIPCHK(hipMemcpyAsync(U.d_km, kmers, n * W * 8, hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(U.d_cnt, counts, n * 4, hipMemcpyHostToDevice, m->stream));
	}
	return unitigs_host_core(m, k, U.d_km, U.d_cnt, n, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, n_unitigs, n_bases_out);
}

static int count_unitigs_listing(kmx_model *m, const char *who)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!m->cnt.listed) return fail(KMX_E_STATE, "%s: no listing (kmx_count_finish has not run since the last kmx_count_begin or build)", who);
	return KMX_OK;
}

static int kmx_count_unitigs_dev_impl(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity,
                                      uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitigs_dev"));
	auto &C = m->cnt;
	return unitigs_dev_core(m, C.k, C.d_run[1], C.d_runc[1], C.n_list, thr, d_seq_out, seq_capacity, (u64 *)d_offsets_out, d_rec, rec_capacity, n_unitigs, n_bases_out);
}

static int kmx_count_unitigs_impl(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity,
                                  uint64_t *n_unitigs, uint64_t *n_bases_out)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitigs"));
	if (!n_unitigs || !n_bases_out || (seq_out && !offsets_out)) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = 0;
	auto &C = m->cnt;
	TRY(unitig_args(C.k, C.n_list));
	HIPCHK(hipSetDevice(m->device));
	return unitigs_host_core(m, C.k, C.d_run[1], C.d_runc[1], C.n_list, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, n_unitigs, n_bases_out);
}

// ---- kmx_unitig_graph*: the twins above with link_offsets [2 rec_cap + 1] and links [link_cap]
static int unitig_graph_dev_core(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, char *d_seq_out, u64 seq_cap, u64 *d_offs_out, kmx_unitig *d_rec, u64 rec_cap,
                                 u64 *d_loffs, u32 *d_links, u64 link_cap, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	if (!n_unitigs || !n_bases_out || !n_links) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = *n_links = 0;
	TRY(unitig_args(k, n));
	if ((n && (!d_km || !d_cnt)) || (d_seq_out && (!d_offs_out || !d_loffs || !d_links))) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	UniDev d{};
	int cur = 0;
	u64 nu = 0, nb = 0, nl = 0;
	TRY(unitig_rank(m, k, d_km, d_cnt, n, thr, &d, &cur, &nu, &nb, &nl));
	*n_unitigs = nu;
	*n_bases_out = nb;
	*n_links = nl;
	if (!d_seq_out) return KMX_OK;                                 // the sizing call
	if (nu > rec_cap || nb > seq_cap || nl > link_cap) return uni_range(nu, nb, nl, rec_cap, seq_cap, link_cap);
	TRY(unitig_emit(m, d, cur, n, nu, (unsigned char *)d_seq_out, seq_cap, d_offs_out, (Unitig *)d_rec, rec_cap));
	return unitig_link_emit(m, d, cur, n, nu, d_loffs, rec_cap, d_links, link_cap);
}

static int kmx_unitig_graph_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, char *d_seq_out, uint64_t seq_capacity,
                                     uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity,
                                     uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	return unitig_graph_dev_core(m, k, (const u64 *)d_kmers, d_counts, n, thr, d_seq_out, seq_capacity, (u64 *)d_offsets_out, d_rec, rec_capacity, (u64 *)d_link_offsets, d_links, link_capacity,
	                             n_unitigs, n_bases_out, n_links);
}

static int unitig_graph_host_core(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, char *seq_out, u64 seq_cap, uint64_t *offs_out, kmx_unitig *rec, u64 rec_cap,
                                  uint64_t *loffs_out, uint32_t *links_out, u64 link_cap, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	auto &U = m->uni;
	UniDev d{};
	int cur = 0;
	u64 nu = 0, nb = 0, nl = 0;
	TRY(unitig_rank(m, k, d_km, d_cnt, n, thr, &d, &cur, &nu, &nb, &nl));
	*n_unitigs = nu;
	*n_bases_out = nb;
	*n_links = nl;
	if (!seq_out) return KMX_OK;
	if (nu > rec_cap || nb > seq_cap || nl > link_cap) return uni_range(nu, nb, nl, rec_cap, seq_cap, link_cap);
	const hipStream_t st = m->stream;
	if (U.d_seq.ensure(nb, st) != hipSuccess || U.d_offs.ensure(nu + 1, st) != hipSuccess || (rec && U.d_rec.ensure(nu, st) != hipSuccess) ||
	    U.d_loffs.ensure(2 * nu + 1, st) != hipSuccess || U.d_links.ensure(nl, st) != hipSuccess)
		return uni_nomem();
	TRY(unitig_emit(m, d, cur, n, nu, U.d_seq, nb, U.d_offs, rec ? U.d_rec.get() : nullptr, nu));
	TRY(unitig_link_emit(m, d, cur, n, nu, U.d_loffs, nu, U.d_links, nl));
	if (nb) HIPCHK(hipMemcpyAsync(seq_out, U.d_seq, nb, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(offs_out, U.d_offs, (nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (rec && nu) HIPCHK(hipMemcpyAsync(rec, U.d_rec, nu * sizeof(Unitig), hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(loffs_out, U.d_loffs, (2 * nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (nl) HIPCHK(hipMemcpyAsync(links_out, U.d_links, nl * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

static int kmx_unitig_graph_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, char *seq_out, uint64_t seq_capacity,
                                 uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity,
                                 uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	if (!m || !n_unitigs || !n_bases_out || !n_links) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = *n_links = 0;
	TRY(unitig_args(k, n));
	if ((n && (!kmers || !counts)) || (seq_out && (!offsets_out || !link_offsets || !links))) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	auto &U = m->uni;
	const u64 W = (u64)(k + 31) / 32;
	if (n) {
		if (U.d_km.ensure(n * W, m->stream) != hipSuccess || U.d_cnt.ensure(n, m->stream) != hipSuccess) return uni_nomem();
		HIPCHK(hipMemcpyAsync(U.d_km, kmers, n * W * 8, hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(U.d_cnt, counts, n * 4, hipMemcpyHostToDevice, m->stream));
	}
	return unitig_graph_host_core(m, k, U.d_km, U.d_cnt, n, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out, n_links);
}

static int kmx_count_unitig_graph_dev_impl(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity,
                                           uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitig_graph_dev"));
	auto &C = m->cnt;
	return unitig_graph_dev_core(m, C.k, C.d_run[1], C.d_runc[1], C.n_list, thr, d_seq_out, seq_capacity, (u64 *)d_offsets_out, d_rec, rec_capacity, (u64 *)d_link_offsets, d_links, link_capacity,
	                             n_unitigs, n_bases_out, n_links);
}

static int kmx_count_unitig_graph_impl(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity,
                                       uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitig_graph"));
	if (!n_unitigs || !n_bases_out || !n_links || (seq_out && (!offsets_out || !link_offsets || !links))) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = *n_links = 0;
	auto &C = m->cnt;
	TRY(unitig_args(C.k, C.n_list));
	HIPCHK(hipSetDevice(m->device));
	return unitig_graph_host_core(m, C.k, C.d_run[1], C.d_runc[1], C.n_list, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out, n_links);
}

// seconds[4]: adjacency (with validation and the index), links, ranking, emit (with the marks and their scan) of the last call
// on this handle, measured only under kmx_set_profile(m, 1); *rounds: its doubling rounds
static int kmx_unitigs_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 4; i++) seconds[i] = m->uni.phase_s[i];
	*rounds = m->uni.rounds;
	return KMX_OK;
}

// seconds[5]: the four of kmx_unitigs_last_phases, then the links between unitigs (their counts and scan, the links kernel): 0
// after a call that asked for no edges
static int kmx_unitig_graph_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 5; i++) seconds[i] = m->uni.phase_s[i];
	*rounds = m->uni.rounds;
	return KMX_OK;
}

// ---- kmx_*unitig_graph_clean*: the graph calls above run round by round on a working copy of the counts (the rule: include/kmx.h).
// A round is unitig_rank on (k-mers, working counts, thr), the two emits into the handle's staging buffers (records, link_offsets
// and links; no strings), k_uni_clean and k_uni_drop; its four counters reach the host in one wait.  A round that removes nothing
// leaves the rank state of the final graph standing, and the caller's buffers are written from it.
static_assert(sizeof(kmx_clean_params) == 16 && sizeof(kmx_clean_stats) == 64, "kmx_clean_params is 16 bytes, kmx_clean_stats 64");

// the phase figures as they stand, put back when the scope ends: what runs inside it is not added to them
struct UniPhaseKeep {
	kmx_model *m;
	double s[6];
	explicit UniPhaseKeep(kmx_model *mm) : m(mm) { for (int i = 0; i < 6; i++) s[i] = m->uni.phase_s[i]; }
	~UniPhaseKeep() { for (int i = 0; i < 6; i++) m->uni.phase_s[i] = s[i]; }
};

static int unitig_clean_args(const kmx_clean_params *p, u32 thr)
{
	if (!p) return fail(KMX_E_ARG, "null cleaning parameters");
	if (!thr) return fail(KMX_E_ARG, "cleaning needs thr >= 1: a removed node is one whose count lies below thr");
	if (!p->ops || (p->ops & ~7u)) return fail(KMX_E_ARG, "ops = %u is no non-empty subset of KMX_CLEAN_TIPS | KMX_CLEAN_ISLANDS | KMX_CLEAN_BUBBLES", p->ops);
	if (!p->max_tip || !p->max_bubble) return fail(KMX_E_ARG, "max_tip and max_bubble are at least 1 k-mer");
	if (p->max_rounds < 1 || p->max_rounds > KMX_CLEAN_MAX_ROUNDS) return fail(KMX_E_ARG, "max_rounds = %u is outside [1, %d]", p->max_rounds, KMX_CLEAN_MAX_ROUNDS);
	return KMX_OK;
}

// the rounds, on a device-resident listing.  On KMX_OK *S is complete, d_removed[n] (device, may be null) holds the round of
// every removed entry, and (*d, *cur, *nu, *nb, *nl) are what unitig_rank left for the final graph: the emits may follow.
static int unitig_clean_rounds(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, const kmx_clean_params &P, unsigned char *d_removed, kmx_clean_stats *S,
                               UniDev *d, int *cur, u64 *nu, u64 *nb, u64 *nl)
{
	auto &U = m->uni;
	const hipStream_t st = m->stream;
	double acc[6] = {0, 0, 0, 0, 0, 0};
	u64 doublings = 0;
	auto add = [&] { for (int i = 0; i < 6; i++) acc[i] += U.phase_s[i]; doublings += U.rounds; };
	auto keep = [&] { for (int i = 0; i < 6; i++) U.phase_s[i] = acc[i]; U.rounds = doublings; };
	*S = kmx_clean_stats{0, 0, 0, 0, 0, 0, 0, 0};
	if (n) {
		if (U.d_wcnt.ensure(n, st) != hipSuccess || U.d_cctr.ensure(4, st) != hipSuccess) return uni_nomem();
		HIPCHK(hipMemcpyAsync(U.d_wcnt, d_cnt, n * 4, hipMemcpyDeviceToDevice, st));
		if (d_removed) HIPCHK(hipMemsetAsync(d_removed, 0, n, st));
	}
	for (u32 r = 1;; r++) {
		const int rc = unitig_rank(m, k, d_km, U.d_wcnt, n, thr, d, cur, nu, nb, nl);
		if (rc != KMX_OK) { add(); keep(); return rc; }
		if (r == 1) { S->n_unitigs_before = *nu; S->n_links_before = *nl; }
		if (r > P.max_rounds) { S->rounds_run = P.max_rounds; S->converged = 0; add(); break; }   // the last round still removed something
		if (!*nu) { S->rounds_run = r; S->converged = 1; add(); break; }
		if (U.d_offs.ensure(*nu + 1, st) != hipSuccess || U.d_rec.ensure(*nu, st) != hipSuccess || U.d_loffs.ensure(2 * *nu + 1, st) != hipSuccess ||
		    U.d_links.ensure(*nl, st) != hipSuccess || U.d_verdict.ensure(*nu, st) != hipSuccess) { add(); keep(); return uni_nomem(); }
		TRY(unitig_emit(m, *d, *cur, n, *nu, nullptr, 0, U.d_offs, U.d_rec, *nu));          // the records only: no byte of a string is stored
		TRY(unitig_link_emit(m, *d, *cur, n, *nu, U.d_loffs, *nu, U.d_links, *nl));
		UniClock clk(m);
		HIPCHK(hipMemsetAsync(U.d_cctr, 0, 4 * sizeof(unsigned long long), st));
		const UniClean c{U.d_rec, U.d_loffs, U.d_links, *nu, *nl, P.ops, P.max_tip, P.max_bubble};
		kmxk::unitig_clean(c, U.d_verdict, U.d_cctr, st);
		kmxk::unitig_drop(*d, U.d_pair[*cur], (const UniTot *)U.d_mn.get(), U.d_verdict, *nu, U.d_wcnt, d_removed, (unsigned char)r, U.d_cctr, st);
		HIPCHK(hipGetLastError());
		unsigned long long ctr[4] = {0, 0, 0, 0};
		HIPCHK(hipMemcpyAsync(ctr, U.d_cctr, sizeof ctr, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));                            // the round's one wait beyond the ranking's own
		clk.lap(5);
		add();
		S->n_tips += ctr[0]; S->n_islands += ctr[1]; S->n_bubbles += ctr[2]; S->n_kmers_removed += ctr[3];
		if (!ctr[3]) { S->rounds_run = r; S->converged = 1; break; }
	}
	keep();
	return KMX_OK;
}

static int unitig_clean_dev_core(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, const kmx_clean_params *P, char *d_seq_out, u64 seq_cap, u64 *d_offs_out,
                                 kmx_unitig *d_rec, u64 rec_cap, u64 *d_loffs, u32 *d_links, u64 link_cap, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links,
                                 uint8_t *d_removed, kmx_clean_stats *stats)
{
	if (!n_unitigs || !n_bases_out || !n_links) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = *n_links = 0;
	if (stats) *stats = kmx_clean_stats{0, 0, 0, 0, 0, 0, 0, 0};
	TRY(unitig_args(k, n));
	TRY(unitig_clean_args(P, thr));
	if ((n && (!d_km || !d_cnt)) || (d_seq_out && (!d_offs_out || !d_loffs || !d_links))) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	UniDev d{};
	int cur = 0;
	u64 nu = 0, nb = 0, nl = 0;
	kmx_clean_stats S;
	TRY(unitig_clean_rounds(m, k, d_km, d_cnt, n, thr, *P, d_removed, &S, &d, &cur, &nu, &nb, &nl));
	*n_unitigs = nu;
	*n_bases_out = nb;
	*n_links = nl;
	if (stats) *stats = S;
	if (!d_seq_out) return KMX_OK;                                 // the sizing call
	if (nu > rec_cap || nb > seq_cap || nl > link_cap) return uni_range(nu, nb, nl, rec_cap, seq_cap, link_cap);
	const UniPhaseKeep sums(m);                                    // the figures are the rounds' own: the emit into the caller's buffers is not added
	TRY(unitig_emit(m, d, cur, n, nu, (unsigned char *)d_seq_out, seq_cap, d_offs_out, (Unitig *)d_rec, rec_cap));
	return unitig_link_emit(m, d, cur, n, nu, d_loffs, rec_cap, d_links, link_cap);
}

static int kmx_unitig_graph_clean_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, const kmx_clean_params *params, char *d_seq_out,
                                           uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links,
                                           uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *d_removed, kmx_clean_stats *stats)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	return unitig_clean_dev_core(m, k, (const u64 *)d_kmers, d_counts, n, thr, params, d_seq_out, seq_capacity, (u64 *)d_offsets_out, d_rec, rec_capacity, (u64 *)d_link_offsets, d_links,
	                             link_capacity, n_unitigs, n_bases_out, n_links, d_removed, stats);
}

static int unitig_clean_host_core(kmx_model *m, int k, const u64 *d_km, const u32 *d_cnt, u64 n, u32 thr, const kmx_clean_params &P, char *seq_out, u64 seq_cap, uint64_t *offs_out,
                                  kmx_unitig *rec, u64 rec_cap, uint64_t *loffs_out, uint32_t *links_out, u64 link_cap, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links,
                                  uint8_t *removed, kmx_clean_stats *stats)
{
	auto &U = m->uni;
	const hipStream_t st = m->stream;
	UniDev d{};
	int cur = 0;
	u64 nu = 0, nb = 0, nl = 0;
	kmx_clean_stats S;
	if (removed && n && U.d_removed.ensure(n, st) != hipSuccess) return uni_nomem();
	TRY(unitig_clean_rounds(m, k, d_km, d_cnt, n, thr, P, removed && n ? U.d_removed.get() : nullptr, &S, &d, &cur, &nu, &nb, &nl));
	*n_unitigs = nu;
	*n_bases_out = nb;
	*n_links = nl;
	if (stats) *stats = S;
	if (removed && n) {
		HIPCHK(hipMemcpyAsync(removed, U.d_removed, n, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	if (!seq_out) return KMX_OK;
	if (nu > rec_cap || nb > seq_cap || nl > link_cap) return uni_range(nu, nb, nl, rec_cap, seq_cap, link_cap);
	if (U.d_seq.ensure(nb, st) != hipSuccess || U.d_offs.ensure(nu + 1, st) != hipSuccess || U.d_rec.ensure(nu, st) != hipSuccess ||
	    U.d_loffs.ensure(2 * nu + 1, st) != hipSuccess || U.d_links.ensure(nl, st) != hipSuccess)
		return uni_nomem();
	const UniPhaseKeep sums(m);
	TRY(unitig_emit(m, d, cur, n, nu, U.d_seq, nb, U.d_offs, rec ? U.d_rec.get() : nullptr, nu));
	TRY(unitig_link_emit(m, d, cur, n, nu, U.d_loffs, nu, U.d_links, nl));
	if (nb) HIPCHK(hipMemcpyAsync(seq_out, U.d_seq, nb, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(offs_out, U.d_offs, (nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (rec && nu) HIPCHK(hipMemcpyAsync(rec, U.d_rec, nu * sizeof(Unitig), hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(loffs_out, U.d_loffs, (2 * nu + 1) * 8, hipMemcpyDeviceToHost, st));
	if (nl) HIPCHK(hipMemcpyAsync(links_out, U.d_links, nl * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return KMX_OK;
}

static int kmx_unitig_graph_clean_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, const kmx_clean_params *params, char *seq_out,
                                       uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity,
                                       uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *removed, kmx_clean_stats *stats)
{
	if (!m || !n_unitigs || !n_bases_out || !n_links) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = *n_links = 0;
	if (stats) *stats = kmx_clean_stats{0, 0, 0, 0, 0, 0, 0, 0};
	TRY(unitig_args(k, n));
	TRY(unitig_clean_args(params, thr));
	if ((n && (!kmers || !counts)) || (seq_out && (!offsets_out || !link_offsets || !links))) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	auto &U = m->uni;
	const u64 W = (u64)(k + 31) / 32;
	if (n) {
		if (U.d_km.ensure(n * W, m->stream) != hipSuccess || U.d_cnt.ensure(n, m->stream) != hipSuccess) return uni_nomem();
		HIPCHK(hipMemcpyAsync(U.d_km, kmers, n * W * 8, hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(U.d_cnt, counts, n * 4, hipMemcpyHostToDevice, m->stream));
	}
	return unitig_clean_host_core(m, k, U.d_km, U.d_cnt, n, thr, *params, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out,
	                              n_links, removed, stats);
}

static int kmx_count_unitig_graph_clean_dev_impl(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec,
                                                 uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out,
                                                 uint64_t *n_links, uint8_t *d_removed, kmx_clean_stats *stats)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitig_graph_clean_dev"));
	auto &C = m->cnt;
	return unitig_clean_dev_core(m, C.k, C.d_run[1], C.d_runc[1], C.n_list, thr, params, d_seq_out, seq_capacity, (u64 *)d_offsets_out, d_rec, rec_capacity, (u64 *)d_link_offsets, d_links,
	                             link_capacity, n_unitigs, n_bases_out, n_links, d_removed, stats);
}

static int kmx_count_unitig_graph_clean_impl(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec,
                                             uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out,
                                             uint64_t *n_links, uint8_t *removed, kmx_clean_stats *stats)
{
	TRY(count_unitigs_listing(m, "kmx_count_unitig_graph_clean"));
	if (!n_unitigs || !n_bases_out || !n_links || (seq_out && (!offsets_out || !link_offsets || !links))) return fail(KMX_E_ARG, "null argument");
	*n_unitigs = *n_bases_out = *n_links = 0;
	if (stats) *stats = kmx_clean_stats{0, 0, 0, 0, 0, 0, 0, 0};
	auto &C = m->cnt;
	TRY(unitig_args(C.k, C.n_list));
	TRY(unitig_clean_args(params, thr));
	HIPCHK(hipSetDevice(m->device));
	return unitig_clean_host_core(m, C.k, C.d_run[1], C.d_runc[1], C.n_list, thr, *params, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs,
	                              n_bases_out, n_links, removed, stats);
}

// seconds[6]: the five of kmx_unitig_graph_last_phases summed over the rounds of the last cleaning call on this handle, then the
// decisions and the removal; *rounds: its doubling rounds, summed likewise
static int kmx_unitig_clean_last_phases_impl(kmx_model *m, double *seconds, uint64_t *rounds)
{
	if (!m || !seconds || !rounds) return fail(KMX_E_ARG, "null argument");
	for (int i = 0; i < 6; i++) seconds[i] = m->uni.phase_s[i];
	*rounds = m->uni.rounds;
	return KMX_OK;
}
