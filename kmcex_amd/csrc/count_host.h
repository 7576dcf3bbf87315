// count_host.h -- kmx_count_* and kmx_build_from_reads: KMC's counting step on the device, then the build from its listing
// (main.cpp:137-146 runs KMC on the reads, then KModel::init on its database, kmodel.hpp:57-86).  Included into kmx_api.hip
// after the query-along-sequences section, whose chunk rule (SeqChunks) and pinned pipeline the host variant shares.
//
// A session: kmx_count_begin allocates one piece of window keys.  Batches of sequences launch k_count_windows into it
// (count_kernels.h); a full piece is sorted, run-length encoded and merged into the running listing (count_device.hip), so
// device memory follows the distinct k-mers, not the windows.  kmx_count_finish flushes the last piece, keeps the k-mers
// with ci <= count <= 10^9, caps their counts at cs, and runs build_common -- what kmx_build_dev runs -- on that listing.

static const u64 kCountPiece = u64(1) << 26;                   // window keys per piece
static const u32 kCountMax = 1000000000u;                      // KMC's default -cx (kmcEx's driver does not override it)

// KMX_COUNT_PIECE (test hook): pieces, host chunks and reader batches of this many windows / bases, so a small test crosses
// many of their boundaries.  Read at every kmx_count_begin (a test sets it after the library is loaded).
static u64 count_piece_hook()
{
	const char *e = hook_env("KMX_COUNT_PIECE");
	const long long x = e ? atoll(e) : 0;
	return x > 0 ? std::min<u64>((u64)x, kCountPiece) : 0;
}

static int count_dev_fail(hipError_t e, const char *what, u64 distinct)
{
	if (e == hipErrorOutOfMemory)
		return fail(KMX_E_NOMEM, "counting: out of device memory in %s, after %llu distinct k-mers", what, (unsigned long long)distinct);
	return fail(KMX_E_NODEVICE, "counting: %s failed: %s", what, hipGetErrorString(e));
}

// a failure inside a session ends it (the model is untouched: the build runs only at the end of kmx_count_finish)
static int count_abort(kmx_model *m, int rc)
{
	hipGetLastError();
	free_count(m, true);
	return rc;
}

// d_run[b] / d_runc[b] hold at least `need` entries afterwards (what they held is dropped); they grow by half again
static int count_grow(kmx_model *m, int b, u64 need)
{
	auto &C = m->cnt;
	if (C.d_run[b] && C.d_runc[b].cap() >= need) return KMX_OK;
	HIPCHK(hipStreamSynchronize(m->stream));
	C.d_run[b].reset(); C.d_runc[b].reset();
	for (u64 want : {need + need / 2, need}) {
		want = std::max<u64>(want, 1);
		if (C.d_run[b].alloc(want * C.W) == hipSuccess && C.d_runc[b].alloc(want) == hipSuccess) return KMX_OK;
		C.d_run[b].reset(); C.d_runc[b].reset();
		hipGetLastError();
	}
	return fail(KMX_E_NOMEM, "counting: out of device memory for %llu listing entries, after %llu distinct k-mers", (unsigned long long)need, (unsigned long long)C.D);
}

static int count_read(kmx_model *m, int i, u64 *v)
{
	unsigned long long x = 0;
	HIPCHK(hipMemcpyAsync(&x, m->cnt.d_n + i, sizeof x, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	*v = x;
	return KMX_OK;
}

// the current piece -> sorted, run-length encoded, merged into the running listing (d_run[0], D entries)
static int count_flush(kmx_model *m)
{
	auto &C = m->cnt;
	if (!C.fill) return KMX_OK;
	u64 np = 0, nu = 0;
	TRY(count_read(m, 0, &np));
	HIPCHK(hipMemsetAsync(C.d_n, 0, sizeof(unsigned long long), m->stream));
	C.fill = 0;
	np = std::min<u64>(np, C.piece);
	if (!np) return KMX_OK;
	C.windows += np;
	hipError_t e = kmxk::count_piece(C.W, C.k, C.d_pa, C.d_pb, C.piece, np, C.d_pc, C.d_n + 1, C.d_tmp, m->stream);
	if (e != hipSuccess) return count_dev_fail(e, "the sort of a piece", C.D);
	TRY(count_read(m, 1, &nu));
	if (!C.D) {                                                    // the first piece is the listing
		TRY(count_grow(m, 0, nu));
		HIPCHK(hipMemcpyAsync(C.d_run[0], C.d_pa, nu * C.W * 8, hipMemcpyDeviceToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(C.d_runc[0], C.d_pc, nu * 4, hipMemcpyDeviceToDevice, m->stream));
		C.D = nu;
		return KMX_OK;
	}
	const u64 nm = C.D + nu;
	TRY(count_grow(m, 1, nm));
	e = kmxk::count_merge(C.W, C.d_run[0], C.d_runc[0], C.D, C.d_pa, C.d_pc, nu, C.d_run[1], C.d_runc[1], C.d_tmp, m->stream);
	if (e != hipSuccess) return count_dev_fail(e, "the merge", C.D);
	TRY(count_grow(m, 0, nm));                                     // (the merge has read d_run[0]: count_grow waits for it)
	e = kmxk::count_reduce(C.W, C.d_run[1], C.d_runc[1], nm, C.d_run[0], C.d_runc[0], C.d_n + 2, C.d_tmp, m->stream);
	if (e != hipSuccess) return count_dev_fail(e, "the merge", C.D);
	return count_read(m, 2, &C.D);
}

// windows [p0, p0 + n_win) of one batch on the device into the current piece, flushing the piece whenever it is full
static int count_launch(kmx_model *m, const unsigned char *d_seq, u64 n_bases, const u64 *d_offs, u64 n_seqs, u64 p0, u64 n_win)
{
	auto &C = m->cnt;
	while (n_win) {
		if (C.fill == C.piece) TRY(count_flush(m));
		const u64 w = std::min<u64>(n_win, C.piece - C.fill);
		kmxk::count_windows(C.k, d_seq, n_bases, d_offs, n_seqs, p0, w, C.d_pa, C.d_pa + C.piece, C.piece, C.d_n, m->stream);
		C.fill += w;
		p0 += w;
		n_win -= w;
	}
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

static int kmx_count_begin_impl(kmx_model *m, int k)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_model_k(k));
	HIPCHK(hipSetDevice(m->device));
	free_count(m, true);
	auto &C = m->cnt;
	C.k = k;
	C.W = (k + 31) / 32;
	const u64 hook = count_piece_hook();
	C.piece = hook ? hook : kCountPiece;
	hipError_t e = C.d_pa.alloc(C.piece * C.W);
	if (e == hipSuccess) e = C.d_pb.alloc(C.piece * C.W);
	if (e == hipSuccess) e = C.d_pc.alloc(C.piece);
	if (e == hipSuccess) e = C.d_n.alloc(4);
	if (e == hipSuccess) e = hipMemsetAsync(C.d_n, 0, 4 * sizeof(unsigned long long), m->stream);
	if (e != hipSuccess) return count_abort(m, count_dev_fail(e, "kmx_count_begin", 0));
	C.on = true;
	return KMX_OK;
}

static int kmx_count_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!m->cnt.on) return fail(KMX_E_STATE, "kmx_count_seqs_dev outside a counting session (kmx_count_begin first)");
	if (!n_seqs || !n_bases) return KMX_OK;
	if (!d_seq || !d_offsets) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const int rc = count_launch(m, (const unsigned char *)d_seq, n_bases, (const u64 *)d_offsets, n_seqs, 0, n_bases);
	return rc ? count_abort(m, rc) : KMX_OK;
}

static int kmx_count_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (!m->cnt.on) return fail(KMX_E_STATE, "kmx_count_seqs outside a counting session (kmx_count_begin first)");
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	const u64 n_bases = offsets[n_seqs];
	if (!n_bases) return KMX_OK;
	if (!seq) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	std::lock_guard<std::mutex> lk(m->query_mu);                  // the pinned slots of m->qfeed
	const u64 hook = count_piece_hook();
	SeqChunks sc(seq, offsets, n_seqs, (u64)m->cnt.k, std::min<u64>(hook ? hook : kSeqChunk, m->cnt.piece));
	const SlotShape shape = sc.shape();
	auto &F = m->qfeed;
	int rc = KMX_OK;
	const int prc = query_pipeline(m, n_bases, 1, seq_workers(n_bases),
		[&](int, u64 lo, u64 hi, unsigned char *dst) { sc.stage(lo, hi, dst); },
		[&](int s, u64 cn, u64 c) {
			if (!rc) rc = count_launch(m, F.d_in[s], sc.nbytes_of(c), sc.bounds(F.d_in[s]), sc.seqs_of(c), 0, cn);
		}, (int32_t *)nullptr, &shape);
	if (!rc) rc = prc;
	return rc ? count_abort(m, rc) : KMX_OK;
}

static int kmx_count_finish_impl(kmx_model *m, uint64_t *n_listed)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	auto &C = m->cnt;
	if (!C.on) return fail(KMX_E_STATE, "kmx_count_finish outside a counting session (kmx_count_begin first)");
	HIPCHK(hipSetDevice(m->device));
	int rc = count_flush(m);
	if (rc) return count_abort(m, rc);
	HIPCHK(hipStreamSynchronize(m->stream));
	C.d_pa.reset(); C.d_pb.reset(); C.d_pc.reset();
	// ci <= c <= 10^9, capped at cs: d_run[0] -> d_run[1]
	if ((rc = count_grow(m, 1, C.D))) return count_abort(m, rc);
	DevBuf<unsigned char> keep;
	hipError_t e = keep.alloc(C.D);
	if (e == hipSuccess) e = kmxk::count_filter(C.W, C.d_run[0], C.d_runc[0], C.D, (u32)m->ci, (u32)m->cs, kCountMax, C.d_run[1], C.d_runc[1], keep, C.d_n + 2, C.d_tmp, m->stream);
	if (e != hipSuccess) return count_abort(m, count_dev_fail(e, "the filter", C.D));
	u64 n = 0;
	if ((rc = count_read(m, 2, &n))) return count_abort(m, rc);
	C.listed = true;
	C.n_list = n;
	free_count(m, false);                                          // everything of the session but the listing
	if (n_listed) *n_listed = n;
	C.building = true;
	rc = build_common(m, C.k, C.d_run[1], C.d_runc[1], n, n);      // = kmx_build_dev on the listing
	C.building = false;
	return rc;
}

static int kmx_count_listing_impl(kmx_model *m, uint64_t *kmers, uint32_t *counts, uint64_t capacity, uint64_t *n)
{
	if (!m || !n) return fail(KMX_E_ARG, "null argument");
	auto &C = m->cnt;
	if (!C.listed) return fail(KMX_E_STATE, "no listing: kmx_count_finish has not run since the last kmx_count_begin or build");
	*n = C.n_list;
	if (!kmers) return KMX_OK;
	if (capacity < C.n_list) return fail(KMX_E_ARG, "capacity %llu < %llu k-mers listed", (unsigned long long)capacity, (unsigned long long)C.n_list);
	HIPCHK(hipSetDevice(m->device));
	if (C.n_list) {
		HIPCHK(hipMemcpyAsync(kmers, C.d_run[1], C.n_list * C.W * 8, hipMemcpyDeviceToHost, m->stream));
		if (counts) HIPCHK(hipMemcpyAsync(counts, C.d_runc[1], C.n_list * 4, hipMemcpyDeviceToHost, m->stream));
	}
	HIPCHK(hipStreamSynchronize(m->stream));
	return KMX_OK;
}

// FASTQ / FASTA (plain or gzip) or "@list": a reader thread parses batches (reads_reader.cpp) while the previous batch is
// counted through the pinned pipeline above; begin, the count and finish as one call.
static int kmx_build_from_reads_impl(kmx_model *m, int k, const char *input)
{
	if (!m || !input) return fail(KMX_E_ARG, "null argument");
	TRY(check_model_k(k));
	std::vector<std::string> files;
	std::string err;
	if (!kmx::reads_inputs(input, files, err)) return fail(KMX_E_IO, "%s", err.c_str());
	TRY(kmx_count_begin_impl(m, k));
	const u64 hook = count_piece_hook();
	kmx::ReadsReader rd(files, k, hook ? std::max<u64>(hook, 2 * (u64)k) : u64(1) << 26);
	kmx::ReadBatch b[2];
	std::thread th;
	int ok[2] = {0, 0};
	auto parse = [&](int i) { ok[i] = rd.next(b[i]); };
	int cur = 0;
	parse(cur);
	int rc = KMX_OK;
	while (ok[cur] > 0) {
		th = std::thread(parse, cur ^ 1);                          // the next batch is parsed while this one is counted
		rc = kmx_count_seqs_impl(m, b[cur].bases.data(), b[cur].offs.data(), b[cur].offs.size() - 1);
		th.join();
		if (rc) return rc;                                         // (the session has ended)
		cur ^= 1;
	}
	if (ok[cur] < 0) return count_abort(m, fail(KMX_E_IO, "%s", rd.error().c_str()));
	return kmx_count_finish_impl(m, nullptr);
}
