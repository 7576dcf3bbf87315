// kmx_api.hip -- host orchestration + the C ABI of include/kmx.h.
//
// Mirrors KModel's life cycle (kmodel.hpp:45-235, :674-696) with the bit arrays resident in HBM.
// There is no CPU compute path in this file: every insert/query runs in the gfx950 kernels of
// kernels.hip; the host only sizes, streams, sorts the (small) rest table and does file I/O.
#include "../../include/kmx.h"
#include "hip_owned.h"
#include "kmc_reader.h"
#include "launchers.h"
#include "reads_reader.h"
#include "strpack.h"

#include <algorithm>
#include <atomic>
#include <exception>
#include <new>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <dlfcn.h>
#include <fcntl.h>
#include <rccl/rccl.h>                                             // types and prototypes only: librccl.so is opened with dlopen when the RCCL transport is asked for
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

// Every behaviour-changing environment variable of this library is a TEST HOOK (forced code paths, shrunken tables): they
// are read only when KMX_TEST_HOOKS=1 is set as well, so that a stray variable cannot move a user onto an untuned path.
// (KMX_INIT_TRACE only prints phase times and is not gated.)
static const char *hook_env(const char *name)
{
	static const bool on = [] { const char *e = getenv("KMX_TEST_HOOKS"); return e && atoi(e) != 0; }();
	return on ? getenv(name) : nullptr;
}
static int fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}
#define HIPCHK(call)                                                                             \
	do {                                                                                         \
		hipError_t e_ = (call);                                                                  \
		if (e_ != hipSuccess) return fail(KMX_E_NODEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
	} while (0)

extern "C" const char *kmx_last_error(void) { return g_err; }

static int kmx_device_count_impl(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// ------------------------------------------------------------------------------------------ OccuBin
// occu_bin.hpp:27-83: three zones -- identity below e1 = 2^nh/4, 2^nh/2 bins 3 wide, 2^nh/4 bins `cap` wide.
static int occubin_tables(int cs, int nh, std::vector<u32> &bin_of_occ, std::vector<u32> &mean_of_bin)
{
	const int mc = cs + 1, e3 = 1 << nh, e1 = e3 / 4, e2 = e1 + e3 / 2;
	bin_of_occ.assign(mc, 0xFFFFFFFFu);
	std::vector<u32> mean_of_occ(mc, 0xFFFFFFFFu);
	int start = e1;
	for (int i = 0; i < e3 / 2; i++, start += 3)
		for (int j = 0; j < 3; j++) {
			if (start + j >= mc) return -1;                    // cs too small for nh (reference overruns, Q11)
			mean_of_occ[start + j] = start + 1;
			bin_of_occ[start + j] = e1 + i;
		}
	const int nz3 = e3 / 4, cap = (mc - start) / nz3;
	for (int i = 0; i < nz3; i++, start += cap)
		for (int j = 0; j < cap; j++) {
			mean_of_occ[start + j] = (2 * start + cap) / 2;
			bin_of_occ[start + j] = e2 + i;
		}
	for (int i = start; i < mc; i++) {
		mean_of_occ[i] = (2 * start - cap) / 2;
		bin_of_occ[i] = e3 - 1;
	}
	for (int i = 0; i < e1 && i < mc; i++) bin_of_occ[i] = i;
	mean_of_bin.assign(e3, 0);                                 // unordered_map::operator[] on a missing bin yields 0
	for (int b = 0; b < e1; b++) mean_of_bin[b] = b;
	std::vector<char> seen(e3, 0);
	for (int i = e1; i < mc; i++) {                            // map::insert keeps the first mean per bin
		u32 b = bin_of_occ[i];
		if (b < (u32)e3 && !seen[b]) { seen[b] = 1; if ((int)b >= e1) mean_of_bin[b] = mean_of_occ[i]; }
	}
	return 0;
}

static int kmx_occubin_impl(int cs, int nh, uint32_t *bin_of_occ, uint32_t *mean_of_bin)
{
	if (nh < 3 || nh > KMX_MAX_NH || cs < 1) return fail(KMX_E_ARG, "bad cs/nh");
	std::vector<u32> b, m;
	if (occubin_tables(cs, nh, b, m)) return fail(KMX_E_ARG, "cs=%d too small for nh=%d", cs, nh);
	memcpy(bin_of_occ, b.data(), b.size() * 4);
	memcpy(mean_of_bin, m.data(), m.size() * 4);
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ rest table (host side)
// rest.hpp:46-65 arrays in their on-disk form (Appendix B.2) + the device form used by k_query.
struct RestTable {
	int k = 0, pre_len = 0, map_size = 0, pre_buffer_size = 0, suff_group = 0;
	u64 suff_bin_size = 0, entries = 0;
	std::vector<int> hash2index, pre_buffer, count_bin;
	std::vector<unsigned char> suffix_bin;
	bool host_valid = false;       // the four on-disk arrays above are materialised (load, or lazily at save)
	// device: kept by capacity from build to build like the arrays (grow-only; a table is valid through `entries` and the
	// sizes above, never through what the buffers can hold)
	DevBuf<int> d_h2i, d_pre, d_cnt;   // d_cnt: counts in sorted order
	DevBuf<u64> d_suf;
	DevBuf<u64> d_sorted;          // sorted k-mers [entries][W] (kept for save after a device build)
	int fbits = 0;                 // lookup accelerators (see ModelDev)
	DevBuf<u32> d_fine;
	DevBuf<u64> d_q;
	DevBuf<unsigned char> d_tmp;   // scratch of rest_sort / rest_index (rest_device.hip)
	// an empty table again; the device buffers stay for the next one
	void clear()
	{
		k = pre_len = map_size = pre_buffer_size = suff_group = fbits = 0;
		suff_bin_size = entries = 0;
		hash2index = {}; pre_buffer = {}; count_bin = {}; suffix_bin = {};
		host_valid = false;
	}
};
static int rest_prefix_len(int k) { for (int i = 7; i >= 3; i--) if ((k - i) % 4 == 0) return i; return 3; }   // rest.hpp:78-83
// k of a model or of a counting session.  rest.hpp:78-83 gives k = 3 a prefix of 7 bases (-4 % 4 == 0 in C): a suffix of
// -1 groups and a -8-bit suffix field, so the reference cannot build that model; like any input it cannot handle, it is refused.
static int check_model_k(int k)
{
	if (k < 4 || k > 64) return fail(KMX_E_ARG, "k=%d out of range [4,64]%s", k, k == 3 ? ": the reference's rest table is undefined at k = 3 (prefix of 7 bases, rest.hpp:78-83)" : "");
	return KMX_OK;
}

struct RestEnt { u64 w[2]; int c; };

// ------------------------------------------------------------------------------------------ the model
enum { ST_EMPTY = 0, ST_BUILDING = 1, ST_READY = 2 };

// The fold kernel a handle starts with in kmx_unitig_pair_lift* (lift_kernels.h): the fold inside the wavefront, or with
// -DKMX_LIFT_PLAIN_FOLD the lane-per-item fold it was measured against.
#ifdef KMX_LIFT_PLAIN_FOLD
#define KMX_LIFT_FOLD_DEFAULT KMX_LIFT_FOLD_PLAIN
#else
#define KMX_LIFT_FOLD_DEFAULT KMX_LIFT_FOLD_WAVE
#endif

// Ownership: every device / pinned buffer, stream and event below is a member that releases itself (hip_owned.h), so
// kmx_destroy is `delete` once the caller's stream has drained.  Members go in reverse order of declaration, and a Stream
// drains before it is destroyed: inside KmcFeed, QueryFeed and the probe the streams are declared AFTER the events and the
// buffers their copies touch, so a stream has drained before those go.  `stream` is the caller's (kmx_set_stream), never
// destroyed here; kmx_destroy synchronises it first.  Pointers into a slab (d_bf, d_bf_back, d_surv) and the device alias
// d_feedback own nothing; the by-value kernel argument blocks (md, bd, blm, kmb, range.rd, probe) are views filled from the owners.
struct kmx_model {
	int ci = 1, cs = 1023, nh = 7, nb = 5, k = 0, bf_num = 1, W = 1;
	int device = 0, state = ST_EMPTY;
	hipStream_t stream = nullptr;
	std::vector<u32> h_bin_of_occ, h_mean_of_bin;
	DevBuf<u32> d_bin_of_occ, d_mean_of_bin;
	u64 n_total = 0, n_km = 0, n_bf[3] = {0, 0, 0};
	u64 byte_bf[3] = {0, 0, 0}, byte_bf_back[3] = {0, 0, 0}, km_byte_size = 0, byte_km_back = 0, ncells = 0;
	DevBuf<u32> d_bloom;                                       // ONE slab for bf[i] / bf_back[i], back to back (d_bf / d_bf_back point into it)
	u64 bloom_words = 0, bf_woff[3] = {0, 0, 0}, bf_back_woff[3] = {0, 0, 0};
	u32 *d_bf[3] = {nullptr, nullptr, nullptr}, *d_bf_back[3] = {nullptr, nullptr, nullptr};
	DevBuf<u32> d_km_back;
	DevBuf<cell_t> d_cells[KMX_MAX_NB];
	RestTable rest;
	ModelDev md;
	// ---- build-time state
	DevBuf<u64> d_stg_kmers;
	DevBuf<u32> d_stg_counts;                                  // (its capacity is the staging stream's: one front-end chunk + one block)
	u64 stg_n = 0;
	BlockDev bd;
	DevBuf<unsigned char> d_block_scratch;
	int scratch_nb = 0, scratch_W = 0;
	DevBuf<u64> d_rest_kmers;
	DevBuf<int> d_rest_counts;                                 // (its capacity is the rest accumulators')
	DevBuf<unsigned long long> d_rest_n;
	u64 rest_upper = 0;
	DevBuf<u64> d_stale_kmers;
	DevBuf<int> d_stale_counts;
	DevBuf<u64> d_stats, d_nbf;
	DevBuf<int> d_tile_cnt, d_tile_off, d_total;
	DevBuf<int> d_totals;                                      // per-chunk totals of one insert_batch call
	PinBuf<int> h_totals, h_total;
	PinBuf<u64> h_words;                                       // what a build reads back between its steps: [ST_N] stats, then the HW_* words
	PinBuf<u64> h_feedback{hipHostMallocMapped};               // ST_MAX_U0 as of some earlier block (heuristic input)
	u64 *d_feedback = nullptr;                                 // the same words as the device sees them (k_rest_append writes them)
	u64 epoch = 1, blocks = 0, rounds = 0;
	// Bloom-class k-mers of the front end as a partitioned bit-set over the slab (k_classify_count emits, k_bs_apply sweeps)
	BitScatter blm;
	DevBuf<u32> d_blm_tup;
	DevBuf<int> d_blm_cnt;
	bool blm_deferred = false;
	int blm_sweep_every = 1;                                   // chunks of the front end per sweep of the slab
	// km_back insert as a partitioned bit-set (k_kmback_emit per round, k_bs_apply every few blocks)
	BitScatter kmb;
	DevBuf<u32> d_kmb_tup;
	DevBuf<int> d_kmb_cnt;
	u64 kmb_pending = 0, kmb_budget = 0;                       // upper bound of tuples emitted since the last apply / what the bins take
	bool kmb_deferred = false;
	bool dbg_kmb_direct = false;                               // KMX_KMB_DIRECT=1: the atomic path at every size (test hook)
	unsigned char *d_surv[2] = {nullptr, nullptr};             // survivor flags of the current and of the previous block (inside the scratch slab)
	KmbackJob kmb_job = {nullptr, nullptr, 0, 0, 0};            // km_back emission the last block still owes (hosted by the next block's finisher launches)
	bool dbg_kmb_host = true;                                  // KMX_KMB_HOST=0: every block emits in a launch of its own (test hook)
	DevBuf<u32> d_bs2_tup;                                     // second level of the two bit-sets (big filters), shared: [bins * tiles][cap2]
	DevBuf<int> d_bs2_cnt;
	// feed of KModel::init(db): pinned slots, device buffers, copy stream -- kept across calls on the handle (allocating and
	// freeing ~300 MB of pinned + device memory costs ~30 ms per call on this stack)
	struct KmcFeed {
		PinBuf<unsigned char> raw[2];                              // B raw records ...
		DevBuf<unsigned char> draw[2];                             // ... and their device twins
		PinBuf<u64> km[2];                                         // host-decoded (or the caller's) k-mers / counts
		PinBuf<u32> cnt[2];
		DevBuf<u64> dk[2], d_lut;                                  // k-mers / counts of a batch on the device; the prefix LUT
		DevBuf<u32> dc[2];
		PinBuf<u64> h_lut;
		Event ev_copied[2], ev_free[2];
		Stream copy;
		enum { RAW = 1, HOST = 2, DEV = 4, LUT = 8 };
		hipError_t ensure(int parts, size_t B, size_t rb, int W, size_t n_lut);
	} feed;
	// feed of kmer_to_occ(vector<string>): three slots of pinned + device buffers (strings in, answers out), a copy stream
	// each way -- kept on the handle like the KMC feed
	struct QueryFeed {
		static const int S = 3;
		PinBuf<unsigned char> h_in[S];
		DevBuf<unsigned char> d_in[S];
		PinBuf<int32_t> h_out[S];
		DevBuf<int32_t> d_out[S];
		// kmx_query_seqs*: the positions of one piece's windows that are not uppercase ACGT + two counters (one per piece
		// parity); at most one piece of windows, whatever the length of the input
		DevBuf<u32> d_seq_list, d_seq_cnt;
		// kmx_correct_seqs*: one bit per window of a piece and its halos, one byte per workgroup of the piece
		DevBuf<u64> d_corr_bits;
		DevBuf<unsigned char> d_corr_flags;
		// kmx_edit_seqs* / kmx_apply_edits_dev: one weak bit per window of the WHOLE input, the edit counter (and the totals of
		// an apply), room for the sort's second list and the scan of an apply, rocPRIM's scratch
		DevBuf<u64> d_edit_bits, d_edit_alt;
		DevBuf<unsigned long long> d_edit_cnt;
		DevBuf<unsigned char> d_edit_tmp;
		// kmx_polish_seqs*: one pass's edit list, its scan and its kmx_seq_edits records; kinds, targets and the scanned triples of
		// the active reads; the two active batches (bytes, offsets, map to the caller's reads) that passes 2, 3, ... alternate
		// between; a parking area per pass; the reads' homes, lengths and (when the caller wants none) records
		DevBuf<u64> d_pol_edits, d_pol_escan, d_pol_delta, d_pol_home, d_pol_len, d_pol_offs[2], d_pol_ids[2];
		DevBuf<unsigned char> d_pol_kind, d_pol_act[2], d_pol_park[POLISH_MAX_PASSES + 1];
		DevBuf<SeqEdits> d_pol_re;
		DevBuf<SeqPolish> d_pol_rec;
		DevBuf<PolishTri> d_pol_tri;
		PinBuf<u64> h_pol_cnt;                                     // where a pass's counts reach the host
		// kmx_extend_seqs*: the walks of one chunk of seeds, the two lists of live walks and their three counters
		DevBuf<ExtWalk> d_ext_walk;
		DevBuf<u32> d_ext_lists, d_ext_cnt;
		Event ev_in[S], ev_k[S], ev_out[S];
		Stream to_dev, to_host;
	} qfeed;
	// position-range partition over several GPUs (kmx_range_*): this rank's exchange buffers, its resolver tables, and the
	// owner-side view of the block working set (overflow flags + padded bin counters for the detect kernel on received claims)
	struct RangeState {
		bool on = false;
		bool pending = false;                                      // a round was resolved since the last seal: its winners' commits sit in front of the regions
		bool mailbox = false;                                      // the regions live in the owners' inboxes (kmx_build_from_kmc_multi_ex), not in d_send
		RangeDev rd = {};                                          // (a view: range_begin_common fills it from the owners below)
		DevBuf<int> d_ccnt, d_tcnt, d_n_contended;
		DevBuf<u32> d_tidx, d_contended, d_rt_resv, d_rt_mark, d_rt_eidx, d_rt_um;
		DevBuf<u64> d_rt_key;
		RangePlan plan = {};
		RangeIn in = {};                                           // mailbox transport: this rank's inbox as its owner-side kernels see it
		BlockDev obd = {};
		DevBuf<int> d_oovf;
		DevBuf<int> d_opcnt;                                       // the owner's claim-bin counters, one per 128-byte line (k_range_verdict)
		DevBuf<unsigned char> d_lver;                              // one verdict byte per triple received in a round (detect answers there, k_range_ship sends it on)
		// caller-moved transport (kmx_range_*_dev): the regions and their headers in this rank's memory
		DevBuf<u64> d_send;
		DevBuf<u32> d_hdr;                                         // [KMX_MAX_RANKS][2]
		PinBuf<u32> h_hdr;                                         // its pinned copy
		u64 sent_tot[KMX_MAX_RANKS] = {};                          // words per destination of the last emit (where each region's verdicts start in what comes back)
		bool inband = false;                                       // the regions travel as fixed-size messages [header | capx words] (kmx_range_inband)
		u64 capx = 0, cap_full = 0;                                // words per region shipped / the worst case of a round
		DevBuf<int> d_ovf;                                         // raised by a launch that had to drop a word (fixed-size messages only)
		// mailbox transport: what the other ranks write into (through peer mappings when they sit on other devices)
		DevBuf<u64> d_inbox;                                       // [world][cap] region of sender s
		DevBuf<u32> d_in_hdr;                                      // [world][2]
		DevBuf<unsigned char> d_vbox;                              // [world][cap] verdict bytes of the words this rank sent to owner q
		u64 alloc_key = 0;                                         // nb, nh, world, transport the buffers were sized for
		int n0[KMX_MAX_NB] = {};                                   // entries of the held lists when the block came in (km_back is emitted once per block)
	} range;
	RoundProbe probe = {false, nullptr, nullptr, nullptr, nullptr};   // KMX_PREGATHER_PROBE=1 (test hook): kernels.hip k_probe_pregather
	DevBuf<u32> probe_sink;                                    // ... and what it points at
	Event probe_fork, probe_done;
	Stream probe_side;
	bool ring = false;                                         // built by several GPUs (kmx_shard_begin): this handle holds ONE rank's share
	int ring_rank = 0, ring_world = 1;
	int nsub = 1;                                              // grid-wide ordered passes in round 0 (see process_block)
	// The winners of a round are committed beside the check of the NEXT round (k_round_commit_check), also across a block
	// boundary: `pending` says that the round with list parity pp ^ 1 and round index pending_t still owes its commit.
	int pp = 0;                                                // list / per-slot-state parity of the next round (alternates from round to round, never reset inside a build)
	bool pending = false;
	int pending_t = 0;
	bool defer = true;                                         // false: every round commits in a launch of its own before the next check (arrays above 2^KMX_CL_MIX_BITS = 2^36 positions; KMX_PIPE=0)
	bool dbg_no_defer = false;
	// test hooks, read from the environment by kmx_begin: forced pass counts, forced older code
	// paths (KMX_ROUND_* flags of kmx_types.h), a trace of the pass-count controller
	int dbg_nsub0 = -1, dbg_nsub1 = -1, dbg_flags = 0;
	int dbg_small_detect = -1;                                 // KMX_SMALL_DETECT=0/1: force the form of the late rounds' k_round_detect (test hook)
	bool dbg_ctrl = false;
	u64 h_stats[ST_N] = {0};
	double t_insert_kernels = 0, t_total = 0;
	Event ev0, ev1;
	// per-kernel-class timing (kmx_set_profile)
	KernelProf prof;
	std::vector<Event> prof_events;
	std::vector<int> prof_spans;
	size_t prof_used = 0;
	double kc_seconds[KC_N] = {0};
	uint64_t kc_launches[KC_N] = {0};
	// queries on one handle may come from several host threads (the reference's kmer_to_occ is called from an OpenMP loop):
	// one query at a time holds this for its whole length -- qfeed, prof's vectors and h_stats[ST_QUERY_*] are shared
	std::mutex query_mu;
	// a counting session (kmx_count_*, count_host.h): one piece of window keys, the running listing (sorted, unique, saturating
	// counts) in two buffers, and after finish the listing the model was built from
	struct CountState {
		bool on = false;                                           // between kmx_count_begin and the end of kmx_count_finish
		bool building = false;                                     // kmx_count_finish is building from the listing (kmx_begin keeps it)
		int k = 0, W = 1;
		u64 piece = 0, fill = 0;                                   // window slots per piece / windows launched into the current one
		DevBuf<u64> d_pa, d_pb;                                    // [W piece] each: the piece's keys, then its distinct keys; sort scratch
		DevBuf<u32> d_pc;                                          // [piece] the distinct keys' counts
		DevBuf<unsigned long long> d_n;                            // [4] windows in the piece, distinct in the piece, listed, spare
		DevBuf<u64> d_run[2];                                      // keys (W words each) of the running listing / of the merge
		DevBuf<u32> d_runc[2];                                     // ... their counts (the capacity of d_runc[b] is the entries the pair holds)
		u64 D = 0;                                                 // entries of the running listing (in d_run[0])
		u64 windows = 0;                                           // windows counted so far
		DevBuf<unsigned char> d_tmp;                               // rocPRIM scratch
		bool listed = false;                                       // d_run[1] holds the listing of the last finish
		u64 n_list = 0;
	} cnt;
	// kmx_unitigs* (unitig_host.h): the work arrays of a call, kept by capacity from call to call
	struct UniState {
		DevBuf<u32> d_start, d_succ1, d_pred1, d_mn, d_flag;       // d_mn: [2][2 n] ranks' minima, later the scanned marks; d_flag: [0] bad listing, [1 + t] round t moved
		DevBuf<unsigned char> d_deg, d_tmp;
		DevBuf<u64> d_pair[2];                                     // [2 n + 2] each: the rank state and its copy, later the marks
		DevBuf<u64> d_km;                                          // the host variant's listing and its output
		DevBuf<u32> d_cnt;
		DevBuf<unsigned char> d_seq;
		DevBuf<u64> d_offs;
		DevBuf<Unitig> d_rec;
		DevBuf<u64> d_loffs;                                       // the host variant's link_offsets and links (kmx_unitig_graph)
		DevBuf<u32> d_links;
		DevBuf<u32> d_wcnt;                                        // kmx_*unitig_graph_clean*: the working copy of the counts (a removed node's is 0), ...
		DevBuf<unsigned char> d_verdict, d_removed;                // ... a verdict per unitig of the round, the host variant's removed[], ...
		DevBuf<unsigned long long> d_cctr;                         // ... [4] tips, islands, bubbles, k-mers removed this round
		double phase_s[6] = {0, 0, 0, 0, 0, 0};                    // under kmx_set_profile(m, 1): adjacency (with the index), links, ranking, emit, links between unitigs, cleaning (decisions and removal)
		u64 rounds = 0;                                            // doubling rounds of the last call
	} uni;
	// kmx_unitig_map_* (map_host.h): a session's index -- the listing's bucket index, the place of every entry, m_u -- and the
	// work arrays of one chunk of windows, kept by capacity from batch to batch
	struct MapState {
		bool on = false;                                           // between kmx_*unitig_map_begin* and kmx_unitig_map_end
		bool from_count = false;                                   // the listing is cnt.d_run[1]: what drops that ends the session
		MapDev dev{};
		DevBuf<u64> d_km;                                          // the host variant's copy of the listing
		DevBuf<u32> d_start, d_mu, d_err;                          // d_err: [0] bad listing, [1] bad unitig set
		DevBuf<u64> d_place;
		DevBuf<u64> d_code, d_spos, d_state;                       // per chunk: codes, segment starts; [2] segments so far, the open segment's start
		DevBuf<u32> d_ex;                                          // the scanned start flags
		DevBuf<unsigned char> d_tmp;                               // rocPRIM scratch
		DevBuf<unsigned char> d_wflag;                             // kmx_unitig_walk_segs*, per segment: the flag byte, ...
		DevBuf<u32> d_wjoin;                                       // ... the join's overlap and d, ...
		DevBuf<WalkTot> d_wsc;                                     // ... [n_segs + 1] the walk and step starts in front of it; ...
		DevBuf<unsigned long long> d_wcnt;                         // ... [WALK_C_N] the call's counters
		DevBuf<unsigned long long> d_panchor, d_pcnt;              // kmx_unitig_pair_walks* (pair_host.h): [n_seqs] the anchor words, [PAIR_C_N] the call's counters, ...
		DevBuf<u64> d_pkey, d_psc;                                 // ... [4][n_items] keys, indices and both sorted; [n_items + 1] the scanned key changes, ...
		DevBuf<u32> d_pdist;                                       // ... [n_pairs] the distance of every pair that is a link, ...
		DevBuf<PairLink> d_pmrg;                                   // ... [n_items] the merged list
	} map;
	// kmx_unitig_contigs* (contig_host.h): the work arrays of a call, kept by capacity from call to call
	struct CtgState {
		DevBuf<u64> d_esup, d_best, d_supo, d_ubase;               // sup per link; best, the only kept edge's support per oriented unitig; where a unitig's bytes go
		DevBuf<u64> d_clc;                                         // [2][2 U + 1] the kept edges at the contig ends, and their scan
		DevBuf<unsigned char> d_ekeep, d_nk, d_circ, d_tmp;        // the verdict per link, the kept count per oriented unitig, the cycle flag per unitig; rocPRIM scratch
		DevBuf<u32> d_only, d_mn, d_last, d_flag;                  // d_mn: [2][2 U] running minima; d_flag: [1 + t] round t moved
		DevBuf<CtgRank> d_rank[2];                                 // [2 U + 2] each: the rank state and its copy, later the marks
		DevBuf<CtgTot> d_sc;                                       // [U + 1] the scanned marks
		DevBuf<unsigned long long> d_cnt;                          // [CTG_C_N]
		double phase_s[5] = {0, 0, 0, 0, 0};                       // under kmx_set_profile(m, 1): supports and verdicts, ranking, marks, records and graph, bytes
		u64 rounds = 0;
	} ctg;
	// kmx_unitig_walk_through* and kmx_unitig_resolve* (resolve_host.h): the work arrays of a call, kept by capacity from call to call
	struct ResState {
		DevBuf<unsigned char> d_mark;                              // [n_steps + 1] 1 where a walk starts
		DevBuf<unsigned long long> d_cnt;                          // [THR_C_N] the call's counters
		// kmx_unitig_resolve*
		DevBuf<unsigned char> d_bad, d_tmp;                        // [U] an edge at this unitig has no mirror; rocPRIM scratch
		DevBuf<u32> d_ver;                                         // [U] the copies with pi packed above them
		DevBuf<CtgTot> d_tot, d_sc;                                // [U + 1] each: (copies, bytes, edges) and their scan
		DevBuf<unsigned long long> d_rcnt;                         // [RES_C_N]
		double phase_s[4] = {0, 0, 0, 0};                          // under kmx_set_profile(m, 1): verdicts, scan and records, links, bytes
	} res;
	// kmx_unitig_scaffold* (scaffold_host.h): the work arrays of a call, kept by capacity from call to call
	struct ScfState {
		DevBuf<u64> d_best, d_ubase;                               // best per oriented unitig; where a unitig's bytes go
		DevBuf<u32> d_nk, d_mn, d_flag;                            // d_nk: [2][2 U] the kept count and the smallest kept entry; d_mn: [2][2 U] running minima; d_flag: [1 + t] round t moved
		DevBuf<unsigned char> d_circ, d_tmp;                       // the cycle flag per unitig; rocPRIM scratch
		DevBuf<CtgRank> d_rank[2];                                 // [2 U + 2] each: the rank state and its copy, later the marks
		DevBuf<CtgTot> d_sc;                                       // [U + 1] the scanned marks
		DevBuf<unsigned long long> d_cnt;                          // [SCF_C_N]
		double phase_s[5] = {0, 0, 0, 0, 0};                       // under kmx_set_profile(m, 1): verdicts, ranking, marks, records, bytes
		u64 rounds = 0;
	} scf;
	// kmx_unitig_pair_paths* (pair_path_host.h): the work arrays of a call, kept by capacity from call to call
	struct PpState {
		DevBuf<u32> d_work;                                        // [n_plinks][max_steps] the steps of every entry's first hit
		DevBuf<u64> d_sc;                                          // [n_plinks + 1] the scanned steps of the PATH entries
		DevBuf<unsigned long long> d_cnt;                          // [PP_C_N]
		DevBuf<unsigned char> d_tmp;                               // rocPRIM scratch
		double phase_s[3] = {0, 0, 0};                             // under kmx_set_profile(m, 1): search, scan, additions
	} ppath;
	// kmx_unitig_scaffold_fill* (fill_host.h): the work arrays of a call, kept by capacity from call to call
	struct FillState {
		DevBuf<FillTot> d_tot, d_sc;                               // [U + 1] each: what a step writes, and the scan
		DevBuf<u64> d_ubase;                                       // [U] where a unitig's own bytes go
		DevBuf<u32> d_pc_o;                                        // [pieces + 1] the oriented unitig of a path piece
		DevBuf<u64> d_pc_dst, d_pc_pre;                            // [pieces + 1] each: where its bytes go; the piece bytes in front of it
		DevBuf<unsigned long long> d_cnt;                          // [FILL_C_N]
		DevBuf<unsigned char> d_tmp;                               // rocPRIM scratch
		double phase_s[4] = {0, 0, 0, 0};                          // under kmx_set_profile(m, 1): kinds, scan with the wait, records, bytes
	} fill;
	// kmx_unitig_pair_reduce* (reduce_host.h): the work arrays of a call, kept by capacity from call to call
	struct ReduceState {
		DevBuf<u64> d_key, d_sc;                                   // d_key: [2][2 E] the rows' keys and their sorted copy; d_sc: [E + 1] the scanned keep flags
		DevBuf<u32> d_val, d_flag;                                 // d_val: [2][2 E] the rows' numbers and their sorted copy; d_flag: [E] the entry stays
		DevBuf<unsigned long long> d_cnt;                          // [RED_C_N]
		DevBuf<unsigned char> d_tmp;                               // rocPRIM scratch
		double phase_s[4] = {0, 0, 0, 0};                          // under kmx_set_profile(m, 1): rows, sort, verdicts, scan with the wait and the compaction
	} red;
	// kmx_unitig_pair_lift* (lift_host.h): the work arrays of a call, kept by capacity from call to call
	struct LiftState {
		DevBuf<u64> d_key, d_sc;                                   // d_key: [2][E] the items' keys and their sorted copy; d_sc: [E + 1] the scanned key changes
		DevBuf<u32> d_idx;                                         // [2][E] the items' indices and their sorted copy
		DevBuf<PairLink> d_item;                                   // [2][E] the shifted items, then the merged records
		DevBuf<unsigned long long> d_cnt;                          // [LIFT_C_N]
		DevBuf<unsigned char> d_tmp;                               // rocPRIM scratch
		int fold = KMX_LIFT_FOLD_DEFAULT;                          // the fold kernel of the next call (kmx_unitig_pair_lift_fold_variant)
		double phase_s[4] = {0, 0, 0, 0};                          // under kmx_set_profile(m, 1): classes, sort, scan and fold, store with the wait
	} lift;
};

// the end of a map session: its index and work arrays go (after the stream has drained)
static void map_drop(kmx_model *m)
{
	auto &S = m->map;
	if (S.d_start || S.d_place || S.d_code || S.d_km) hipStreamSynchronize(m->stream);
	S.d_km.reset(); S.d_start.reset(); S.d_mu.reset(); S.d_err.reset(); S.d_place.reset();
	S.d_code.reset(); S.d_spos.reset(); S.d_state.reset(); S.d_ex.reset(); S.d_tmp.reset();
	S.d_wflag.reset(); S.d_wjoin.reset(); S.d_wsc.reset(); S.d_wcnt.reset();
	S.d_panchor.reset(); S.d_pcnt.reset(); S.d_pkey.reset(); S.d_psc.reset(); S.d_pdist.reset(); S.d_pmrg.reset();
	S.dev = MapDev{};
	S.on = S.from_count = false;
}

static void prof_begin(KernelProf *p, int cls, hipStream_t st)
{
	auto *ev = (std::vector<Event> *)p->events;
	auto *sp = (std::vector<int> *)p->spans;
	const size_t need = 2 * sp->size() + 2;
	while (ev->size() < need) { Event e; if (e.ensure(hipEventDefault) != hipSuccess) return; ev->push_back(std::move(e)); }
	sp->push_back(cls);
	hipEventRecord((*ev)[2 * sp->size() - 2], st);
}
static void prof_end(KernelProf *p, hipStream_t st)
{
	auto *ev = (std::vector<Event> *)p->events;
	auto *sp = (std::vector<int> *)p->spans;
	if (sp->empty() || ev->size() < 2 * sp->size()) return;
	hipEventRecord((*ev)[2 * sp->size() - 1], st);
}
// fold the recorded spans into kc_seconds / kc_launches (stream must be idle)
static void prof_collect(kmx_model *m)
{
	for (size_t i = 0; i < m->prof_spans.size(); i++) {
		float ms = 0;
		if (hipEventElapsedTime(&ms, m->prof_events[2 * i], m->prof_events[2 * i + 1]) == hipSuccess) {
			m->kc_seconds[m->prof_spans[i]] += ms * 1e-3;
			m->kc_launches[m->prof_spans[i]]++;
		}
	}
	m->prof_spans.clear();
}

enum { HW_NREST = ST_N, HW_NBF, HW_BAD = HW_NBF + 3, HW_N };   // kmx_model::h_words
static const u64 kChunk = u64(1) << 23;                       // k-mers classified per pass of the front end

// the malloc-time counter and the KMX_FAIL_ALLOC countdown of hip_owned.h (three translation units allocate through it)
std::atomic<unsigned long long> kmx_malloc_ns{0};
std::atomic<long long> kmx_fail_alloc{0};

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
#include "graph_checks.h"                                      // check_offsets, the CSR and buffer checks: they need fail and TRY only

// n elements, fresh (what the buffer held goes) / grown only when n exceeds what is there; `zero`: cleared on the stream
template <typename T> static int dalloc(DevBuf<T> &b, u64 n, bool zero, hipStream_t st)
{
	HIPCHK(b.alloc(n));
	if (zero) HIPCHK(hipMemsetAsync(b.get(), 0, n ? n * sizeof(T) : 16, st));
	return KMX_OK;
}
template <typename T> static int ensure(DevBuf<T> &b, u64 n, bool zero, hipStream_t st)
{
	HIPCHK(b.ensure(n, st));
	if (zero) HIPCHK(hipMemsetAsync(b.get(), 0, n ? n * sizeof(T) : 16, st));
	return KMX_OK;
}

// everything kmx_begin sizes by (nb, W): dropped when the shape changes
static void free_build_state(kmx_model *m)
{
	m->d_stg_kmers.reset(); m->d_stg_counts.reset(); m->d_block_scratch.reset();
	m->d_rest_kmers.reset(); m->d_rest_counts.reset(); m->d_rest_n.reset();
	m->d_stale_kmers.reset(); m->d_stale_counts.reset();
	m->d_tile_cnt.reset(); m->d_tile_off.reset(); m->d_total.reset();
	m->d_blm_tup.reset(); m->d_blm_cnt.reset();
	m->d_kmb_tup.reset(); m->d_kmb_cnt.reset();
	m->d_bs2_tup.reset(); m->d_bs2_cnt.reset();
	m->stg_n = 0;
}

static int create_device_side(kmx_model *m);
static int kmx_destroy_impl(kmx_model *m);
static int kmx_create_impl(int ci, int cs, int nh, int nb, kmx_model **out)
{
	if (!out) return fail(KMX_E_ARG, "null out");
	*out = nullptr;
	if (nh < 3 || nh > KMX_MAX_NH || nb < 1 || nb > KMX_MAX_NB || ci < 1 || cs < ci)
		return fail(KMX_E_ARG, "bad parameters ci=%d cs=%d nh=%d nb=%d", ci, cs, nh, nb);
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
		return fail(KMX_E_NODEVICE, "no HIP device: libkmx has no CPU fallback");
	kmx_model *m = new kmx_model();
	m->ci = ci; m->cs = cs; m->nh = nh; m->nb = nb;
	m->bf_num = ci == 1 ? 1 : 3;                               // kmodel.hpp:50
	if (occubin_tables(cs, nh, m->h_bin_of_occ, m->h_mean_of_bin)) { delete m; return fail(KMX_E_ARG, "cs=%d too small for nh=%d", cs, nh); }
	const int rc = create_device_side(m);
	if (rc) { kmx_destroy_impl(m); return rc; }                // whatever was allocated so far goes with the handle
	*out = m;
	return KMX_OK;
}

static int create_device_side(kmx_model *m)
{
	HIPCHK(hipGetDevice(&m->device));
	HIPCHK(m->d_bin_of_occ.alloc(m->h_bin_of_occ.size()));
	HIPCHK(m->d_mean_of_bin.alloc(m->h_mean_of_bin.size()));
	HIPCHK(hipMemcpy(m->d_bin_of_occ, m->h_bin_of_occ.data(), m->h_bin_of_occ.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(m->d_mean_of_bin, m->h_mean_of_bin.data(), m->h_mean_of_bin.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(m->d_stats.alloc(ST_N));
	HIPCHK(m->d_nbf.alloc(3));
	HIPCHK(hipMemset(m->d_stats, 0, ST_N * 8));
	HIPCHK(m->h_total.alloc(16));
	HIPCHK(m->h_words.alloc(HW_N));
	HIPCHK(m->h_feedback.alloc(8));
	HIPCHK(hipHostGetDevicePointer((void **)&m->d_feedback, m->h_feedback, 0));
	// [2]: the fullest claim bin of a late round (t >= 2), which picks the form of their k_round_detect: until the device reports
	// one, a guess -- a quarter of a list still alive, every survivor a candidate on all its positions -- so that wide
	// configurations (nh >= 9: 2304 > 2048) start on the full-size tables instead of overflowing the small ones
	m->h_feedback[0] = ~0ULL; m->h_feedback[1] = 0; m->h_feedback[2] = (u64)KMX_BUCKET * (u64)m->nh / KMX_CL_MAXBINS / 4;
	{
		auto env_int = [](const char *name, int dflt) { const char *v = hook_env(name); return v ? atoi(v) : dflt; };
		m->dbg_nsub0 = env_int("KMX_NSUB0", -1);
		m->dbg_nsub1 = env_int("KMX_NSUB1", -1);
		m->dbg_flags = (env_int("KMX_FIN_GLOBAL", 0) ? KMX_ROUND_FIN_GLOBAL : 0) | (env_int("KMX_RESOLVE_GATHER", 0) ? KMX_ROUND_RESOLVE_GATHER : 0);
		m->dbg_small_detect = env_int("KMX_SMALL_DETECT", -1);
		m->dbg_no_defer = env_int("KMX_PIPE", 1) == 0;                      // KMX_PIPE=0: commit after every round, check against the committed state only
		m->dbg_ctrl = env_int("KMX_CTRL_DEBUG", 0) != 0;
		m->dbg_kmb_direct = env_int("KMX_KMB_DIRECT", 0) != 0;
		m->dbg_kmb_host = env_int("KMX_KMB_HOST", 1) != 0;
	}
	HIPCHK(m->ev0.ensure(hipEventDefault));
	HIPCHK(m->ev1.ensure(hipEventDefault));
	m->prof.events = &m->prof_events; m->prof.spans = &m->prof_spans; m->prof.begin = prof_begin; m->prof.end = prof_end;
	return KMX_OK;
}

// the buffers of a counting session; with `listing`, the listing of the last kmx_count_finish as well
static void free_count(kmx_model *m, bool listing)
{
	auto &C = m->cnt;
	if (C.d_pa || C.d_pc || C.d_n || C.d_tmp || C.d_run[0] || C.d_run[1]) hipStreamSynchronize(m->stream);
	C.d_pa.reset(); C.d_pb.reset(); C.d_pc.reset(); C.d_n.reset(); C.d_tmp.reset(); C.d_run[0].reset(); C.d_runc[0].reset();
	C.on = false;
	C.piece = C.fill = C.D = C.windows = 0;
	if (listing || !C.listed) {
		if (m->map.on && m->map.from_count) map_drop(m);             // the map session reads the listing where it lies
		C.d_run[1].reset(); C.d_runc[1].reset();
		C.listed = false;
		C.n_list = 0;
	}
}

static int kmx_destroy_impl(kmx_model *m)
{
	if (!m) return KMX_OK;
	hipSetDevice(m->device);
	hipStreamSynchronize(m->stream);
	delete m;                                                  // (the order its members go in: see the comment at the struct)
	return KMX_OK;
}

static int kmx_set_stream_impl(kmx_model *m, void *s)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	m->stream = (hipStream_t)s;
	return KMX_OK;
}

// sizes (kmodel.hpp:402-420, :436-456) and the by-value kernel argument block
static void compute_sizes(kmx_model *m)
{
	u64 nbf = 0;
	for (int i = 0; i < m->bf_num; i++) {
		m->byte_bf[i] = (u64)((double)m->n_bf[i] / 5.5 * (double)(m->nh - 1));          // f64 then truncation (Q5)
		m->byte_bf_back[i] = (m->n_bf[i] >> 3) * (u64)(m->nh - 2);
		nbf += m->n_bf[i];
	}
	m->n_km = m->n_total - nbf;                                                        // kmodel.hpp:433
	m->km_byte_size = (m->n_km >> 4) * (u64)m->nh;
	m->byte_km_back = (m->n_km >> 4) * (u64)(m->nh - 2);
	m->ncells = (m->km_byte_size + 1) / 2;
}

static void fill_model_dev(kmx_model *m)
{
	ModelDev &md = m->md;
	memset(&md, 0, sizeof md);
	md.k = m->k; md.nh = m->nh; md.nb = m->nb; md.ci = m->ci; md.cs = m->cs; md.bf_num = m->bf_num;
	{
		// a failing attempt usually fails on its first few positions: fetch those first (KMX_NH_FIRST >= nh: all at once)
		// (measured at nh = 7: 2 + 2 + 3 positions, profiles/r03_experiments_measured_and_rejected.txt)
		const char *e = hook_env("KMX_NH_FIRST"), *e2 = hook_env("KMX_NH_SECOND");
		const int f = e ? atoi(e) : (2 * m->nh + 3) / 7, f2 = e2 ? atoi(e2) : (4 * m->nh + 3) / 7;
		md.nh_first = f < 1 ? 1 : (f > m->nh ? m->nh : f);
		md.nh_second = f2 < md.nh_first ? md.nh_first : (f2 > m->nh ? m->nh : f2);
	}
	md.gfull = make_geom(m->k);
	md.gback = make_geom(m->k - 2);
	for (int i = 0; i < 3; i++) {
		md.bf[i] = m->d_bf[i]; md.bf_mod[i] = make_mod(i < m->bf_num ? m->byte_bf[i] * 8 : 0);
		md.bf_back[i] = m->d_bf_back[i]; md.bf_back_mod[i] = make_mod(i < m->bf_num ? m->byte_bf_back[i] * 8 : 0);
	}
	md.km_back = m->d_km_back; md.km_back_mod = make_mod(m->byte_km_back * 8);
	md.kmb_direct = m->kmb_deferred ? 0 : 1;
	md.bloom_direct = m->blm_deferred ? 0 : 1;
	for (int i = 0; i < 3; i++) { md.bf_woff[i] = m->bf_woff[i]; md.bf_back_woff[i] = m->bf_back_woff[i]; }
	for (int a = 0; a < m->nb; a++) md.cells[a] = m->d_cells[a];
	md.km_mod = make_mod(m->km_byte_size * 8);
	md.bin_of_occ = m->d_bin_of_occ; md.mean_of_bin = m->d_mean_of_bin;
	md.rest_pre_len = m->rest.pre_len; md.rest_W = m->W; md.rest_entries = m->rest.entries;
	md.rest_h2i = m->rest.d_h2i; md.rest_pre = m->rest.d_pre; md.rest_suf = m->rest.d_suf; md.rest_cnt = m->rest.d_cnt;
	md.rest_fbits = m->rest.fbits; md.rest_fine = m->rest.d_fine; md.rest_q = m->rest.d_q;
}

static int alloc_arrays(kmx_model *m)
{
	{   // the Bloom filters and their back filters live back to back in one slab (the BitScatter of the front end sweeps it)
		u64 off = 0;
		for (int i = 0; i < 3; i++) {
			m->bf_woff[i] = off; off += i < m->bf_num ? (m->byte_bf[i] + 3) / 4 + 1 : 0;
			m->bf_back_woff[i] = off; off += i < m->bf_num ? (m->byte_bf_back[i] + 3) / 4 + 1 : 0;
		}
		m->bloom_words = off;
		TRY(ensure(m->d_bloom, off + 1, true, m->stream));
		for (int i = 0; i < 3; i++) {
			m->d_bf[i] = i < m->bf_num ? m->d_bloom + m->bf_woff[i] : nullptr;
			m->d_bf_back[i] = i < m->bf_num ? m->d_bloom + m->bf_back_woff[i] : nullptr;
		}
	}
	TRY(ensure(m->d_km_back, (m->byte_km_back + 3) / 4 + 1, true, m->stream));
	// (hipMalloc of fresh device memory costs ~90 ms per GB on this stack, also from several threads at once:
	// a cold build of 2.5e9 k-mers spends 2.3 s here, a rebuild on the same handle nothing)
	for (int a = 0; a < m->nb; a++) TRY(ensure(m->d_cells[a], m->ncells + 1, true, m->stream));
	return KMX_OK;
}

// km_back as a partitioned bit-set: bins of a power-of-two number of positions, swept in tiles of 2^20.  Up to 8 tiles per
// bin (a filter of 256 MB: ~8*10^8 coupled k-mers at nh = 7) one workgroup per bin sweeps its tiles one after the other and
// re-reads the bin's tuples for each (k_bs_apply); doing that with 32 tiles LOSES against plain atomics (2.5*10^9 k-mers:
// warm build 2.66 s -> 4.14 s).  Bigger filters get a second level: k_bs_split deals every bin's tuples to its tiles
// (up to 256 per bin: filters of 8 GB), k_bs_apply2 sweeps one tile per workgroup, so every tuple and every word of the
// filter is read once per sweep.  Beyond 2^36 positions the direct atomic path stays.
static const u32 kBsMaxTileShift = 3;
// test hooks: KMX_BS_CAP=<tuples per bin> (read once per process) shrinks the bins of both partitioned bit-sets, so that
// producers meet full bins all the time and set those bits with atomics instead (the result must not change);
// KMX_BS_TILE_LOG2=<t> (10..20) shrinks the tiles, so that small filters take the multi-tile and the two-level sweeps
static u64 bs_cap_hook()
{
	static const u64 v = [] { const char *e = hook_env("KMX_BS_CAP"); const long long x = e ? atoll(e) : 0; return x > 0 ? (u64)std::min<long long>(x, 1 << 18) : 0ull; }();
	return v;
}
static u32 bs_tile_log2()
{
	const char *e = hook_env("KMX_BS_TILE_LOG2");                    // (read at every kmx_begin, so one test process can try several)
	const int x = e ? atoi(e) : 20;
	return (u32)std::min(std::max(x, 10), 20);
}
// geometry of a partitioned bit-set over `nwords` words: false when the filter is too big for it.  L2 storage (shared by
// the two bit-sets of a model: their sweeps never overlap) is grown to what this one needs.
static int bs_geometry(kmx_model *m, BitScatter &bs, u64 nwords, u64 cap, bool *ok)
{
	*ok = false;
	const u32 tlog2 = bs_tile_log2();
	u32 wshift = 5;
	while ((((u64)BS_BINS) << wshift) < nwords * 32) wshift++;
	if (wshift > tlog2 + BS_MAX_TILES_LOG2 || wshift > 32) return KMX_OK;
	bs.nwords = nwords; bs.wshift = wshift; bs.tlog2 = tlog2; bs.cap = (u32)cap;
	bs.cap2 = 0; bs.tup2 = nullptr; bs.cnt2 = nullptr;
	if (wshift > tlog2 + kBsMaxTileShift) {
		const u32 tiles = 1u << (wshift - tlog2);
		// uniform hashing: a tile receives cap/tiles tuples on average when the bin is full; 1/4 more + 256 never fills in
		// practice (and a full tile only costs atomics)
		const u64 cap2 = bs_cap_hook() ? std::max<u64>(bs_cap_hook() / 4, 8) : (cap / tiles + cap / (4 * tiles) + 256);
		const u64 need = (u64)BS_BINS * tiles * cap2, ncnt = (u64)BS_BINS * tiles;
		if (m->d_bs2_tup.cap() < need || m->d_bs2_cnt.cap() < ncnt) {
			HIPCHK(hipStreamSynchronize(m->stream));
			m->d_bs2_tup.reset(); m->d_bs2_cnt.reset();
			TRY(dalloc(m->d_bs2_tup, need, false, m->stream));
			TRY(dalloc(m->d_bs2_cnt, ncnt, true, m->stream));
		}
		bs.cap2 = (u32)cap2;
	}
	*ok = true;
	return KMX_OK;
}
static int setup_kmback_scatter(kmx_model *m)
{
	m->kmb_deferred = false;
	m->kmb_pending = 0;
	m->kmb_job.n_lists = 0;
	const u64 nwords = (m->byte_km_back + 3) / 4;
	if (m->dbg_kmb_direct || nwords == 0) return KMX_OK;
	u32 wshift = 5;
	while ((((u64)BS_BINS) << wshift) < nwords * 32) wshift++;
	const u64 blk = (u64)m->nb * KMX_BUCKET, per_block = blk * (u64)(m->nh - 2);
	// tuples per bin: 1 MB while a bin is a few tiles; more when the sweep re-reads the tuples tile after tile or the filter
	// is big, so that a sweep of the whole filter is shared by more blocks
	u64 cap = wshift <= 22 ? (1u << 18) : (wshift == 23 ? (1u << 19) : (1u << 20));
	// two levels: every sweep reads and writes the whole filter, so the bins grow with it (a sweep per ~nwords/3 tuples:
	// at 10^10 k-mers 2^22 per bin = 4 GB + 5 GB of second-level storage, 52 sweeps of 15.6 GB instead of 207)
	while (wshift > 23 && cap < (1u << 22) && cap * 512 < nwords) cap <<= 1;
	const u64 cap_hook = bs_cap_hook();
	if (cap_hook) cap = cap_hook;
	bool ok;
	TRY(bs_geometry(m, m->kmb, nwords, cap, &ok));
	if (!ok) return KMX_OK;                                        // too big: direct atomics
	const u64 bins_used = (nwords * 32 + (1ULL << m->kmb.wshift) - 1) >> m->kmb.wshift;
	if (m->d_kmb_tup.cap() < (u64)BS_BINS * cap || !m->d_kmb_cnt) {
		HIPCHK(hipStreamSynchronize(m->stream));
		m->d_kmb_tup.reset(); m->d_kmb_cnt.reset();
		TRY(dalloc(m->d_kmb_tup, (u64)BS_BINS * cap, false, m->stream));
		TRY(dalloc(m->d_kmb_cnt, (u64)BS_BINS, true, m->stream));
	}
	m->kmb.words = m->d_km_back;
	m->kmb.tup = m->d_kmb_tup; m->kmb.cnt = m->d_kmb_cnt;
	// positions are hashed uniformly over the used bins: keep the expected fill of a bin below 3/4 (a full bin is still exact)
	m->kmb_budget = bins_used * cap * 3 / 4;
	if (m->kmb_budget < per_block && !cap_hook) return KMX_OK;     // a single block would not fit: tiny filter, direct path
	m->kmb_deferred = true;
	return KMX_OK;
}

// The Bloom slab as a partitioned bit-set: the front end emits a chunk (2^23 k-mers) and sweeps; the bins take a chunk of
// which ~2/3 is Bloom class (more falls back to atomics, bit by bit).
static int setup_bloom_scatter(kmx_model *m)
{
	m->blm_deferred = false;
	if (m->dbg_kmb_direct || m->bloom_words == 0) return KMX_OK;
	m->blm_sweep_every = 1;
	// a slab above 256 MB (second level) costs > 0.5 GB of traffic per sweep: bigger bins, so that a sweep serves more chunks
	const u64 cap = bs_cap_hook() ? bs_cap_hook() : (m->bloom_words > (1ull << 26) ? (1u << 20) : (1u << 18));
	bool ok;
	TRY(bs_geometry(m, m->blm, m->bloom_words, cap, &ok));
	if (!ok) return KMX_OK;
	if (m->d_blm_tup.cap() < (u64)BS_BINS * cap || !m->d_blm_cnt) {
		HIPCHK(hipStreamSynchronize(m->stream));
		m->d_blm_tup.reset(); m->d_blm_cnt.reset();
		TRY(dalloc(m->d_blm_tup, (u64)BS_BINS * cap, false, m->stream));
		TRY(dalloc(m->d_blm_cnt, (u64)BS_BINS, true, m->stream));
	}
	{
		// chunks per sweep from the EXPECTED number of tuples of a chunk (the share of Bloom-class k-mers is known from pass 1):
		// positions are hashed uniformly over the used bins, aim at 3/4 of their capacity; a bin that fills up all the same
		// only costs atomics
		const u64 bins_used = (m->bloom_words * 32 + (1ULL << m->blm.wshift) - 1) >> m->blm.wshift;
		u64 nbf = 0;
		for (int i = 0; i < m->bf_num; i++) nbf += m->n_bf[i];
		const double per_chunk = (double)kChunk * ((double)nbf / (double)std::max<u64>(m->n_total, 1)) * (double)(2 * m->nh - 3) * 1.25;
		const double budget = (double)bins_used * (double)cap * 0.75;
		const double e = per_chunk > 0 ? budget / per_chunk : 1.0;
		m->blm_sweep_every = (int)std::min(std::max(e, 1.0), 64.0);
	}
	m->blm.words = m->d_bloom;
	m->blm.tup = m->d_blm_tup; m->blm.cnt = m->d_blm_cnt;
	m->blm_deferred = true;
	return KMX_OK;
}
// (the two bit-sets share the second-level storage: point both at it once both geometries are known)
static void bs_attach_level2(kmx_model *m)
{
	m->kmb.tup2 = m->blm.tup2 = m->d_bs2_tup;
	m->kmb.cnt2 = m->blm.cnt2 = m->d_bs2_cnt;
}

// sweep km_back with what the rounds have emitted so far
static int kmback_flush(kmx_model *m)
{
	if (!m->kmb_deferred || !m->kmb_pending) return KMX_OK;
	kmxk::bs_apply(m->kmb, m->stream);
	m->kmb_pending = 0;
	HIPCHK(hipGetLastError());
	return KMX_OK;
}
// the (k-2)-mers of the successes -> bins: of round t (n_in_block < 0; the ring, where a rank holds a list for one round)
// or of a whole block after its last round (n_in_block >= 0); `bound` = most k-mers that can have been inserted
static int kmback_reserve(kmx_model *m, u64 bound)
{
	const u64 add = bound * (u64)(m->nh - 2);
	if (m->kmb_pending + add > m->kmb_budget) TRY(kmback_flush(m));
	m->kmb_pending += add;
	return KMX_OK;
}
static int kmback_emit(kmx_model *m, int t, int pp, int n_in_block, u64 bound)
{
	if (m->kmb_deferred) TRY(kmback_reserve(m, bound));          // (else: md.kmb_direct, the kernel ORs the bits in itself)
	kmxk::kmback_emit(m->md, m->bd, m->bd.kmers, m->bd.surv, 0, m->nb, t, pp, n_in_block, m->kmb, m->stream);
	return KMX_OK;
}
// what is left of the job a finished block handed on: emitted in a launch of its own (the k-mers it points at are about to
// be overwritten, the build ends, or no late round can host it)
static int kmback_job_flush(kmx_model *m)
{
	KmbackJob &j = m->kmb_job;
	if (j.n_lists <= 0) return KMX_OK;
	const u64 lo = (u64)j.i0 * KMX_BUCKET, nbk = (u64)j.n_in_block;
	TRY(kmback_reserve(m, nbk > lo ? std::min<u64>(nbk - lo, (u64)j.n_lists * KMX_BUCKET) : 0));
	kmxk::kmback_emit(m->md, m->bd, j.kmers, j.surv, j.i0, j.n_lists, 0, 0, j.n_in_block, m->kmb, m->stream);
	j.n_lists = 0;
	return KMX_OK;
}

// the build-time buffers of one shape (nb, W): staging stream, the block working set in one slab, the small counters
static int alloc_build_state(kmx_model *m)
{
	const int nb = m->nb;
	const u64 blk = (u64)nb * KMX_BUCKET;
	// staging stream for coupled-array k-mers: one front-end chunk plus one block of carry-over
	TRY(dalloc(m->d_stg_kmers, (kChunk + blk) * m->W, false, m->stream));
	TRY(dalloc(m->d_stg_counts, kChunk + blk, false, m->stream));
	// one slab for the block working set
	u64 off = 0;
	auto carve = [&](u64 bytes) { u64 o = off; off += (bytes + 255) & ~u64(255); return o; };
	u64 o_list0 = carve(blk * 4), o_list1 = carve(blk * 4), o_mv0 = carve(blk * 4), o_mv1 = carve(blk * 4);
	u64 o_n0 = carve(nb * 4), o_n1 = carve(nb * 4), o_status0 = carve(blk), o_status1 = carve(blk), o_dfail = carve(blk);
	u64 o_U[KMX_NSLOW];
	for (int s2 = 0; s2 < KMX_NSLOW; s2++) o_U[s2] = carve(blk * 8 * (1 + m->W));
	u64 o_Un = carve((u64)KMX_NSLOW * nb * KMX_CTR_STRIDE * 4), o_R = carve((u64)nb * KMX_RSIZE * 8);
	u64 o_tc0 = carve((u64)nb * KMX_NTILES * 4), o_tc1 = carve((u64)nb * KMX_NTILES * 4);
	const u64 cl_bins = m->nh <= 8 ? KMX_CL_BINS(8) : KMX_CL_BINS(16);
	u64 o_surv = carve(blk), o_surv1 = carve(blk);
	const u64 cl_bytes = (u64)nb * cl_bins * (u64)(m->nh <= 8 ? KMX_CL_CAP_OF(8) : KMX_CL_CAP_OF(16)) * 8;
	u64 o_uw[2], o_crec[2], o_cl_tup[2], o_cl_cnt[2];
	const u64 rec_words = (u64)((m->nh + (m->nh <= 8 ? 1 : 2) + 3) & ~3);      // kernels.hip crec_words
	for (int q = 0; q < 2; q++) {
		o_uw[q] = carve(blk * 4); o_crec[q] = carve(blk * 4 * rec_words);
		o_cl_tup[q] = carve(cl_bytes); o_cl_cnt[q] = carve((u64)nb * KMX_CL_MAXBINS * 4);
	}
	u64 o_cl_ovf = carve((u64)nb * 4);
	TRY(dalloc(m->d_block_scratch, off, true, m->stream));             // R starts at epoch 0; epochs only grow
	m->scratch_nb = nb; m->scratch_W = m->W;
	char *base = (char *)m->d_block_scratch.get();
	BlockDev &bd = m->bd;
	bd.kmers = nullptr; bd.counts = nullptr;
	bd.list[0] = (u32 *)(base + o_list0); bd.list[1] = (u32 *)(base + o_list1);
	bd.mover[0] = (u32 *)(base + o_mv0); bd.mover[1] = (u32 *)(base + o_mv1);
	bd.n[0] = (int *)(base + o_n0); bd.n[1] = (int *)(base + o_n1);
	bd.status[0] = (unsigned char *)(base + o_status0); bd.status[1] = (unsigned char *)(base + o_status1); bd.dfail = (unsigned char *)(base + o_dfail);
	for (int s2 = 0; s2 < KMX_NSLOW; s2++) bd.Urec[s2] = (u64 *)(base + o_U[s2]);
	bd.Un = (int *)(base + o_Un); bd.R = (u64 *)(base + o_R);
	bd.tile_cnt[0] = (int *)(base + o_tc0); bd.tile_cnt[1] = (int *)(base + o_tc1);
	bd.surv = (unsigned char *)(base + o_surv);
	m->d_surv[0] = bd.surv; m->d_surv[1] = (unsigned char *)(base + o_surv1);   // block b flags into d_surv[b & 1]
	for (int q = 0; q < 2; q++) {
		bd.uw[q] = (u32 *)(base + o_uw[q]); bd.crec[q] = (u32 *)(base + o_crec[q]);
		bd.cl_tup[q] = (u64 *)(base + o_cl_tup[q]); bd.cl_cnt[q] = (int *)(base + o_cl_cnt[q]);
	}
	bd.cl_ovf = (int *)(base + o_cl_ovf);                        // zeroed with the slab; the kernels keep it zero between rounds
	bd.stats = m->d_stats;
	TRY(dalloc(m->d_rest_n, 1, false, m->stream));
	TRY(dalloc(m->d_stale_kmers, (u64)nb * 2, false, m->stream));
	TRY(dalloc(m->d_stale_counts, (u64)nb, false, m->stream));
	TRY(dalloc(m->d_total, 4, true, m->stream));
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ streamed build
static int kmx_begin_impl(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_model_k(k));
	HIPCHK(hipSetDevice(m->device));
	if (!m->cnt.building) free_count(m, true);                   // a build from other data ends a counting session and drops its listing
	u64 s = 0;
	for (int i = 0; i < m->bf_num; i++) s += n_bf[i];
	if (s > n_total) return fail(KMX_E_ARG, "n_bf exceeds n_total");
	m->k = k; m->W = (k + 31) / 32;
	m->n_total = n_total;
	for (int i = 0; i < 3; i++) m->n_bf[i] = i < m->bf_num ? n_bf[i] : 0;
	compute_sizes(m);
	// Build-time buffers are kept across builds of the same shape (nb, W): only the counters are re-zeroed.  (Dropped here,
	// before the bit-sets below are pointed at their tuple buffers, which go with them.)
	if (m->d_block_scratch && (m->scratch_nb != m->nb || m->scratch_W != m->W)) free_build_state(m);
	TRY(alloc_arrays(m));
	m->rest.clear();
	TRY(setup_kmback_scatter(m));
	TRY(setup_bloom_scatter(m));
	bs_attach_level2(m);
	fill_model_dev(m);
	const int nb = m->nb;
	const u64 B = KMX_BUCKET, blk = (u64)nb * B;
	if (!m->d_block_scratch) {
		const int rc = alloc_build_state(m);
		if (rc) { m->d_block_scratch.reset(); return rc; }        // (the slab stands for all of it at the next kmx_begin)
	}
	m->stg_n = 0;
	// a build that ended on an error may have left claim counters or dfail marks behind
	for (int q = 0; q < 2; q++) HIPCHK(hipMemsetAsync(m->bd.cl_cnt[q], 0, (u64)nb * KMX_CL_MAXBINS * 4, m->stream));
	HIPCHK(hipMemsetAsync(m->bd.dfail, 0, blk, m->stream));
	HIPCHK(hipMemsetAsync(m->bd.cl_ovf, 0, (u64)nb * 4, m->stream));
	m->pp = 0; m->pending = false; m->pending_t = 0;
	m->defer = !m->dbg_no_defer && m->km_byte_size * 8 <= (1ULL << KMX_CL_MIX_BITS);      // position identity inside a detect table is exact up to 2^36
	// rest accumulators: grown on demand (see ensure_rest_capacity)
	const u64 want_rest = std::max<u64>(m->n_km / 8, 2 * blk) + blk;
	if (m->d_rest_counts.cap() < want_rest || !m->d_rest_kmers) {
		m->d_rest_kmers.reset(); m->d_rest_counts.reset();
		TRY(dalloc(m->d_rest_kmers, want_rest * m->W, false, m->stream));
		TRY(dalloc(m->d_rest_counts, want_rest, false, m->stream));
	}
	m->rest_upper = 0;
	HIPCHK(hipMemsetAsync(m->d_rest_n, 0, 8, m->stream));
	HIPCHK(hipMemsetAsync(m->d_stale_kmers, 0, (u64)nb * 16, m->stream));
	HIPCHK(hipMemsetAsync(m->d_stale_counts, 0, (u64)nb * 4, m->stream));
	HIPCHK(hipMemsetAsync(m->d_stats, 0, ST_N * 8, m->stream));
	m->blocks = 0; m->rounds = 0;
	// [2]: the fullest claim bin of a late round (t >= 2), which picks the form of their k_round_detect: until the device reports
	// one, a guess -- a quarter of a list still alive, every survivor a candidate on all its positions -- so that wide
	// configurations (nh >= 9: 2304 > 2048) start on the full-size tables instead of overflowing the small ones
	m->h_feedback[0] = ~0ULL; m->h_feedback[1] = 0; m->h_feedback[2] = (u64)KMX_BUCKET * (u64)m->nh / KMX_CL_MAXBINS / 4;
	{   // first guess of the contended set per list in round 0: a candidate is contended when one of its nh positions
		// is also claimed with the other value by one of the ~2^18*nh/2 opposite claims spread over the L positions
		const double L = (double)m->km_byte_size * 8.0;
		const double p = L > 0 ? std::min(1.0, (double)m->nh * m->nh * 131072.0 / L) : 1.0;
		const double u0 = 157000.0 * p;
		const double fin = 1024.0 * KMX_FIN_RPT(m->nh <= 8 ? 8 : 16);       // what the LDS finisher holds per list
		// measured at 10^8 k-mers: one load of the finisher 50-60 us; two loads (index ranges) 115 us; one grid-wide pass
		// (37 us) decides half of the set and leaves one load (40 us)
		m->nsub = u0 <= fin ? 0 : (u0 <= 6 * fin ? 1 : (u0 <= 16 * fin ? 3 : (u0 <= 40 * fin ? 5 : 8)));
	}
	m->t_insert_kernels = 0; m->t_total = 0;
	memset(m->h_stats, 0, sizeof m->h_stats);
	{
		const char *pe = hook_env("KMX_PREGATHER_PROBE");
		const bool want = pe && pe[0] == '1';
		if (want && !m->probe.side) {
			HIPCHK(m->probe_side.ensure());
			HIPCHK(m->probe_fork.ensure());
			HIPCHK(m->probe_done.ensure());
			HIPCHK(m->probe_sink.alloc(64));
			m->probe = {false, m->probe_side, m->probe_fork, m->probe_done, m->probe_sink};
		}
		if (want) HIPCHK(hipEventRecord(m->probe.done, m->probe.side));
		m->probe.on = want;
	}
	m->ring = false; m->ring_rank = 0; m->ring_world = 1;
	m->state = ST_BUILDING;
	return KMX_OK;
}

static int ensure_rest_capacity(kmx_model *m, u64 add)
{
	if (m->rest_upper + add <= m->d_rest_counts.cap()) { m->rest_upper += add; return KMX_OK; }
	unsigned long long actual = 0;
	HIPCHK(hipMemcpyAsync(&actual, m->d_rest_n, 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	m->rest_upper = actual;
	if (m->rest_upper + add > m->d_rest_counts.cap()) {
		u64 ncap = std::max<u64>(m->d_rest_counts.cap() * 2, m->rest_upper + add);
		DevBuf<u64> nk;
		DevBuf<int> nc;
		HIPCHK(nk.alloc(ncap * m->W));
		HIPCHK(nc.alloc(ncap));
		HIPCHK(hipMemcpyAsync(nk, m->d_rest_kmers, actual * m->W * 8, hipMemcpyDeviceToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(nc, m->d_rest_counts, actual * 4, hipMemcpyDeviceToDevice, m->stream));
		HIPCHK(hipStreamSynchronize(m->stream));
		m->d_rest_kmers = std::move(nk); m->d_rest_counts = std::move(nc);
	}
	m->rest_upper += add;
	return KMX_OK;
}

// Stale-slot duplicate (quirk Q1, kmodel.hpp:520-527 + :539): in the final partial block every unused
// buffer row whose slot 0 still holds a survivor of the previous block re-offers it to nb-1 arrays (it
// fails on all of them: bits are never cleared) and pushes it to the rest table a second time.
__global__ void k_stale_dup(int first_unused_row, int nb, int W, const u64 *stale_kmers, const int *stale_counts, u64 *rest_kmers, int *rest_counts, unsigned long long *rest_n, u64 *stats)
{
	int i = first_unused_row + threadIdx.x;
	if (i >= nb || stale_counts[i] == 0) return;
	u64 p = atomicAdd(rest_n, 1ULL);
	for (int w = 0; w < W; w++) rest_kmers[p * W + w] = stale_kmers[(u64)i * W + w];
	rest_counts[p] = stale_counts[i];
	atomicAdd(stats + ST_ATTEMPTS, (u64)(nb - 1));
}

// Contention feedback (pinned words that k_rest_append writes, read here while the device is some blocks behind; they
// steer a launch-count heuristic only, never the result): the largest contended set per list, and the largest set that
// reached the single-workgroup finisher.  Small sets are decided by the finisher alone; when too much reaches it,
// grid-wide ordered passes are added in front of it.
static void steer_passes(kmx_model *m)
{
	const u64 u0 = ((volatile u64 *)m->h_feedback)[0], ufin = ((volatile u64 *)m->h_feedback)[1];
	if (u0 != ~0ULL) {
		const u64 fin = 1024ull * KMX_FIN_RPT(m->nh <= 8 ? 8 : 16);
		if (ufin > fin) m->nsub = std::min(m->nsub + (ufin > 4 * fin ? 2 : 1), KMX_MAX_NSUB);
		else if (m->nsub > 0 && u0 <= fin * 7 / 8) m->nsub--;               // the finisher could have taken all of it in one load
		else if (m->nsub > 1 && ufin < fin / 4) m->nsub--;
	}
	if (m->dbg_ctrl) fprintf(stderr, "[kmx] block %llu feedback u0=%lld ufin=%lld -> nsub=%d\n", (unsigned long long)m->blocks, (long long)u0, (long long)ufin, m->nsub);
}
static int passes_of_round(const kmx_model *m, int t)
{
	int nsub = t == 0 ? m->nsub : m->nsub / 2;
	if (t == 0 && m->dbg_nsub0 >= 0) nsub = m->dbg_nsub0;
	if (t > 0 && m->dbg_nsub1 >= 0) nsub = m->dbg_nsub1;
	return nsub;
}

// insert_with_thread (kmodel.hpp:557-573) for the block at staging offset `head`
// the commit the last round still owes (see kmx_model::pending), in a launch of its own
static int flush_pending_commit(kmx_model *m)
{
	if (!m->pending) return KMX_OK;
	kmxk::commit_flush(m->md, m->bd, m->pending_t, m->pp ^ 1, m->stream, &m->prof);
	m->pending = false;
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// one round of the block in m->bd (list parity m->pp): the previous round's commit rides with its check; its own winners
// stay pending -- or are committed right away when the build does not defer (m->defer false: arrays beyond 2^36 positions,
// KMX_PIPE=0).  A rank of the multi-GPU ring defers too (kmx_ring_round_dev passes m->defer): it owns its arrays whole, so
// the claims its detect needs as settled positions are its own.  Deferring is sound only while cl_mix is a bijection on the
// positions of an array -- the gate in kmx_begin and the static_assert below tie the two together.
static_assert(KMX_CL_MIX_BITS == 36, "kmx_begin's defer gate, cl_mix's mask and the 8 + 28-bit table entry of k_round_detect all assume 36 bits");
static int run_round(kmx_model *m, int t, bool defer, const KmbackJob *job)
{
	// late rounds: small detect tables while the fullest late bin the device reported stays far below what they take (a
	// launch-shape heuristic like steer_passes: a bin that does not fit only sends its list down the ordered path, never changes the result)
	const u64 late_bin = ((volatile u64 *)m->h_feedback)[2];
	const bool small_detect = m->dbg_small_detect >= 0 ? m->dbg_small_detect != 0 : late_bin <= 2048;
	const int flags = m->dbg_flags | (m->pending ? KMX_ROUND_PENDING : 0) | (defer ? KMX_ROUND_KEEP : 0) | (small_detect ? KMX_ROUND_SMALL_DETECT : 0);
	kmxk::round(m->md, m->bd, t, m->pp, passes_of_round(m, t), &m->epoch, flags, m->stream, &m->prof, job, &m->kmb, m->probe.on ? &m->probe : nullptr);
	m->pending = true; m->pending_t = t;
	m->pp ^= 1;
	m->rounds++;
	if (!defer) TRY(flush_pending_commit(m));
	return KMX_OK;
}

// insert_with_thread (kmodel.hpp:557-573) for the block at staging offset `head`
static int process_block(kmx_model *m, u64 head, u64 n_in_block, bool final_partial)
{
	const int nb = m->nb;
	m->bd.kmers = m->d_stg_kmers + head * m->W;
	m->bd.counts = m->d_stg_counts + head;
	m->bd.surv = m->d_surv[m->blocks & 1];                        // (the previous block's flags stay readable for its job)
	kmxk::block_init(m->bd, nb, m->pp, (int)n_in_block, m->stream);   // (the pending commit of the previous block reads the OTHER parity)
	steer_passes(m);
	// The previous block's km_back emission rides along with this block's finisher launches, one list per round: 128
	// rider workgroups beside the nb finisher workgroups, one wave of workgroups on 256 CUs.
	KmbackJob &job = m->kmb_job;
	for (int t = 0; t < nb; t++) {
		KmbackJob part = {nullptr, nullptr, 0, 0, 0};
		if (job.n_lists > 0) {
			part = job;
			part.n_lists = 1;
			const u64 lo = (u64)part.i0 * KMX_BUCKET, nbk = (u64)part.n_in_block;
			TRY(kmback_reserve(m, nbk > lo ? std::min<u64>(nbk - lo, (u64)part.n_lists * KMX_BUCKET) : 0));
			job.i0 += part.n_lists;
			job.n_lists -= part.n_lists;
		}
		TRY(run_round(m, t, m->defer, part.n_lists ? &part : nullptr));
	}
	const int pp = m->pp;                                          // the lists the last reorder wrote: the block's survivors
	TRY(ensure_rest_capacity(m, n_in_block + (u64)nb));
	if (final_partial) {
		int row = (int)((n_in_block - 1) / KMX_BUCKET);
		if (row + 1 < nb && m->blocks > 0)
			hipLaunchKernelGGL(k_stale_dup, dim3(1), dim3(64), 0, m->stream, row + 1, nb, m->W, (const u64 *)m->d_stale_kmers,
			                   (const int *)m->d_stale_counts, m->d_rest_kmers.get(), m->d_rest_counts.get(), m->d_rest_n.get(), m->d_stats.get());
	}
	kmxk::rest_append(m->md, m->bd, pp, 0, nb, m->d_rest_kmers, m->d_rest_counts, m->d_rest_n, m->d_stale_kmers, m->d_stale_counts, m->d_feedback, m->stream);
	// km_back insert of everything the block inserted (kmodel.hpp:548-550): handed to the next block's finisher launches,
	// or done here when there is no next block to host it (or the filter takes the direct path)
	if (m->kmb_deferred && m->dbg_kmb_host && !final_partial) {
		job.kmers = m->bd.kmers; job.surv = m->bd.surv; job.n_in_block = (int)n_in_block; job.i0 = 0; job.n_lists = nb;
	} else TRY(kmback_emit(m, 0, pp, (int)n_in_block, n_in_block));
	m->blocks++;
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// per-tile counters / per-chunk totals of the classification front end for a batch of n k-mers
static int ensure_front_end(kmx_model *m, u64 n)
{
	const u64 n_chunks = (n + kChunk - 1) / kChunk, tiles = (u64)kmxk::classify_tiles(n);
	HIPCHK(m->d_tile_cnt.ensure(tiles, m->stream));
	HIPCHK(m->d_tile_off.ensure(tiles, m->stream));
	HIPCHK(m->d_totals.ensure(n_chunks, m->stream));
	HIPCHK(m->h_totals.ensure(n_chunks, m->stream));
	return KMX_OK;
}

// Pass 2 for one batch (kmodel.hpp:68-74).  The batch is cut into chunks of kChunk k-mers.  The front end of the WHOLE
// batch (classification + Bloom insert, commutative: one k_classify_count launch per chunk, the sweeps of the bit-set,
// one k_scan_tiles launch for all chunks) runs first, on the model's stream, and the host waits once for the chunk
// totals.  Then, chunk by chunk and in order on the same stream: the compaction into the staging stream and the
// ordered coupled-array rounds of every full block.
static int kmx_insert_batch_dev_impl(kmx_model *m, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (m->state != ST_BUILDING) return fail(KMX_E_STATE, "insert_batch before begin");
	if (!n) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	const u64 blk = (u64)m->nb * KMX_BUCKET;
	const u64 n_chunks = (n + kChunk - 1) / kChunk;
	TRY(ensure_front_end(m, n));
	const u64 *km0 = (const u64 *)d_kmers;
	const u32 *ct0 = (const u32 *)d_counts;
	// the order-free front end of the whole batch first (classification, Bloom classes), then the ordered rounds chunk by chunk
	kmxk::classify_count(m->md, km0, ct0, n, kChunk, m->d_tile_cnt, m->d_tile_off, m->d_totals, m->d_stats, m->blm, m->blm_sweep_every, m->stream, &m->prof);
	HIPCHK(hipMemcpyAsync(m->h_totals, m->d_totals, n_chunks * 4, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	for (u64 ci = 0, done = 0; ci < n_chunks; ci++) {
		const u64 c = std::min<u64>(kChunk, n - done);
		const u64 *km = km0 + done * m->W;
		const u32 *ct = ct0 + done;
		const u64 add = (u64)m->h_totals[ci];
		done += c;
		if (m->km_byte_size == 0 && add) continue;               // divergence D2: no arrays to insert into
		if (m->stg_n + add > m->d_stg_counts.cap()) return fail(KMX_E_STATE, "staging overflow");
		kmxk::classify_scatter(m->md, km, ct, c, m->d_tile_off + ci * (kChunk / KMX_CLS_TILE), m->d_stg_kmers, m->d_stg_counts, m->stg_n, m->stream);
		m->stg_n += add;
		u64 head = 0;
		while (m->stg_n - head >= blk) {
			TRY(process_block(m, head, blk, false));
			head += blk;
		}
		TRY(kmback_job_flush(m));                                // (the next scatter overwrites the k-mers the job points at)
		if (head) {                                              // carry the remainder (< one block) to the front
			const u64 rem = m->stg_n - head;
			if (rem) {
				HIPCHK(hipMemcpyAsync(m->d_stg_kmers, m->d_stg_kmers + head * m->W, rem * m->W * 8, hipMemcpyDeviceToDevice, m->stream));
				HIPCHK(hipMemcpyAsync(m->d_stg_counts, m->d_stg_counts + head, rem * 4, hipMemcpyDeviceToDevice, m->stream));
			}
			m->stg_n = rem;
		}
	}
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// The slots of the KMC feed for batches of B records of rb bytes / k-mers of W words, the copy stream and its events: the
// `parts` asked for are grown to that size (never shrunk), whatever else the handle holds stays.  Host buffers reach the
// device the same way (kmx_insert_batch: HOST | DEV): two pinned slots filled by a parallel memcpy, a copy stream that
// moves slot b+1 (hipMemcpyAsync) while the model's stream inserts batch b.
hipError_t kmx_model::KmcFeed::ensure(int parts, size_t B, size_t rb, int W, size_t n_lut)
{
	RCHK(copy.ensure());
	for (int s = 0; s < 2; s++) {
		RCHK(ev_copied[s].ensure());
		RCHK(ev_free[s].ensure());
		if (parts & RAW) { RCHK(raw[s].ensure(B * rb + 16, copy)); RCHK(draw[s].ensure(B * rb + 16, copy)); }
		if (parts & HOST) { RCHK(km[s].ensure(B * W, copy)); RCHK(cnt[s].ensure(B, copy)); }
		if (parts & DEV) { RCHK(dk[s].ensure(B * W, copy)); RCHK(dc[s].ensure(B, copy)); }
	}
	if (parts & LUT) { RCHK(d_lut.ensure(n_lut, copy)); RCHK(h_lut.ensure(n_lut, copy)); }
	return hipSuccess;
}

static void parallel_copy(void *dst, const void *src, size_t bytes)
{
	const unsigned hw = std::thread::hardware_concurrency();
	const int T = (int)std::max<size_t>(1, std::min<size_t>(std::min<unsigned>(hw ? hw : 1, 16), bytes / (4u << 20) + 1));
	if (T == 1) { memcpy(dst, src, bytes); return; }
	std::vector<std::thread> th;
	const size_t per = ((bytes + T - 1) / T + 4095) & ~size_t(4095);
	for (int t = 0; t < T; t++)
		th.emplace_back([=] {
			const size_t lo = (size_t)t * per, hi = std::min(bytes, lo + per);
			if (lo < hi) memcpy((char *)dst + lo, (const char *)src + lo, hi - lo);
		});
	for (auto &x : th) x.join();
}

static int kmx_insert_batch_impl(kmx_model *m, const uint64_t *kmers, const uint32_t *counts, uint64_t n)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (m->state != ST_BUILDING) return fail(KMX_E_STATE, "insert_batch before begin");
	if (!n) return KMX_OK;
	if (!kmers || !counts) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const size_t B = size_t(1) << 23;
	const int W = m->W;
	auto &F = m->feed;
	HIPCHK(F.ensure(F.HOST | F.DEV, B, 0, W, 0));
	auto drain = scope_exit([&] { hipStreamSynchronize(F.copy); hipStreamSynchronize(m->stream); });   // the caller's buffers and the slots are free on return
	HIPCHK(hipEventRecord(F.ev_free[0], m->stream));
	HIPCHK(hipEventRecord(F.ev_free[1], m->stream));
	auto stage = [&](int s, uint64_t lo, uint64_t c) -> int {        // host -> pinned slot s -> device buffers s, on the copy stream
		HIPCHK(hipEventSynchronize(F.ev_copied[s]));                 // the previous copy out of this slot (a fresh event is complete)
		parallel_copy(F.km[s], kmers + lo * W, c * W * 8);
		parallel_copy(F.cnt[s], counts + lo, c * 4);
		HIPCHK(hipStreamWaitEvent(F.copy, F.ev_free[s], 0));        // the insert that read the device buffers two batches ago
		HIPCHK(hipMemcpyAsync(F.dk[s], F.km[s], c * W * 8, hipMemcpyHostToDevice, F.copy));
		HIPCHK(hipMemcpyAsync(F.dc[s], F.cnt[s], c * 4, hipMemcpyHostToDevice, F.copy));
		HIPCHK(hipEventRecord(F.ev_copied[s], F.copy));
		return KMX_OK;
	};
	TRY(stage(0, 0, std::min<uint64_t>(B, n)));
	int s = 0;
	for (uint64_t done = 0; done < n; s ^= 1) {
		const uint64_t c = std::min<uint64_t>(B, n - done), next = done + c;
		if (next < n) TRY(stage(s ^ 1, next, std::min<uint64_t>(B, n - next)));      // copied under this batch's rounds
		HIPCHK(hipStreamWaitEvent(m->stream, F.ev_copied[s], 0));
		TRY(kmx_insert_batch_dev(m, (const uint64_t *)F.dk[s].get(), F.dc[s], c));
		HIPCHK(hipEventRecord(F.ev_free[s], m->stream));
		done = next;
	}
	return KMX_OK;
}

// KRestData::build (rest.hpp:95-135,157-161) on the device: radix sort of the survivors + index kernels
// (rest_device.hip).  The on-disk byte arrays are produced lazily by rest_materialize_host (save only).
static int rest_to_device(kmx_model *m);
static int rest_build_accel(kmx_model *m);

static int build_rest(kmx_model *m, u64 n)
{
	RestTable &r = m->rest;
	const int W = m->W, k = m->k;
	r.k = k;
	r.pre_len = rest_prefix_len(k);
	r.map_size = 1 << (2 * r.pre_len);
	r.suff_group = (k - r.pre_len) / 4;
	r.entries = n;
	r.suff_bin_size = n * (u64)r.suff_group;
	r.host_valid = false;
	HIPCHK(r.d_sorted.ensure(n * W + 2, m->stream));
	HIPCHK(r.d_cnt.ensure(n + 4, m->stream));
	HIPCHK(r.d_suf.ensure(n * W + 2, m->stream));
	HIPCHK(r.d_h2i.ensure((u64)r.map_size, m->stream));
	HIPCHK(r.d_pre.ensure((u64)r.map_size + 2, m->stream));
	HIPCHK(hipMemsetAsync(r.d_h2i, 0xFF, (u64)r.map_size * 4, m->stream));
	KPROF_BEGIN(&m->prof, KC_REST, m->stream);                        // class 5: the rest table -- radix sort + index kernels (the accelerators follow)
	HIPCHK(kmxk::rest_sort(m->d_rest_kmers, m->d_rest_counts, n, W, k, r.d_sorted, r.d_cnt, r.d_tmp, m->stream));
	HIPCHK(kmxk::rest_index(r.d_sorted, n, W, k, r.pre_len, r.d_h2i, r.d_pre, r.d_suf, m->d_total, r.d_tmp, m->stream));
	KPROF_END(&m->prof, m->stream);
	HIPCHK(hipMemcpyAsync(m->h_total, m->d_total, 4, hipMemcpyDeviceToHost, m->stream));
	const int rc = rest_build_accel(m);                                // (needs no count of groups: enqueued before the one wait of this function)
	HIPCHK(hipStreamSynchronize(m->stream));
	r.pre_buffer_size = *m->h_total + 1;
	return rc;
}

// bucket index + next-group table for k_query's lookup (device only)
static int rest_build_accel(kmx_model *m)
{
	RestTable &r = m->rest;
	int F = 1;
	while ((1ULL << F) < r.entries * 2 && F < 26) F++;
	F = std::max(F, 2 * r.pre_len);
	F = std::min(F, 2 * r.k);
	r.fbits = F;
	HIPCHK(r.d_fine.ensure((1ULL << F) + 2, m->stream));
	HIPCHK(r.d_q.ensure((u64)r.map_size * m->W, m->stream));
	kmxk::rest_accel(r.d_sorted, r.entries, m->W, r.k, F, r.d_h2i, r.d_pre, r.d_suf, r.map_size, r.d_fine, r.d_q, m->stream);
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// on-disk arrays of rest.bin (Appendix B.2) from the device-resident sorted table
static int rest_materialize_host(kmx_model *m)
{
	RestTable &r = m->rest;
	if (r.host_valid) return KMX_OK;
	const u64 n = r.entries;
	r.hash2index.resize(r.map_size); r.pre_buffer.resize(r.pre_buffer_size); r.count_bin.resize(n);
	r.suffix_bin.assign(r.suff_bin_size, 0);
	HIPCHK(hipMemcpy(r.hash2index.data(), r.d_h2i, (u64)r.map_size * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(r.pre_buffer.data(), r.d_pre, (u64)r.pre_buffer_size * 4, hipMemcpyDeviceToHost));
	if (n) {
		DevBuf<unsigned char> d_bytes;                              // the byte rows are cut on the device
		HIPCHK(d_bytes.alloc(r.suff_bin_size));
		kmxk::rest_suffix_bytes(r.d_sorted, n, m->W, r.suff_group, d_bytes, m->stream);
		hipError_t e = hipMemcpyAsync(r.suffix_bin.data(), d_bytes, r.suff_bin_size, hipMemcpyDeviceToHost, m->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(r.count_bin.data(), r.d_cnt, n * 4, hipMemcpyDeviceToHost, m->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
		if (e != hipSuccess) return fail(KMX_E_NODEVICE, "rest table download failed");
	}
	r.host_valid = true;
	return KMX_OK;
}

// load path: device form (suffix integers, W words per row) from the byte rows read from rest.bin
static int rest_to_device(kmx_model *m)
{
	RestTable &r = m->rest;
	const int W = m->W;
	const u64 n = r.entries;
	std::vector<u64> suf(n * W + 1, 0);
	for (u64 e = 0; e < n; e++) {
		unsigned __int128 val = 0;
		for (int g = 0; g < r.suff_group; g++) val = (val << 8) | r.suffix_bin[e * (u64)r.suff_group + g];
		if (W == 1) suf[e] = (u64)val;
		else { suf[2 * e] = (u64)(val >> 64); suf[2 * e + 1] = (u64)val; }
	}
	HIPCHK(r.d_h2i.alloc((u64)r.map_size));
	HIPCHK(r.d_pre.alloc((u64)r.pre_buffer_size + 1));
	HIPCHK(r.d_cnt.alloc(n + 1));
	HIPCHK(r.d_suf.alloc(suf.size()));
	HIPCHK(hipMemcpy(r.d_h2i, r.hash2index.data(), (u64)r.map_size * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(r.d_pre, r.pre_buffer.data(), (u64)r.pre_buffer_size * 4, hipMemcpyHostToDevice));
	if (n) HIPCHK(hipMemcpy(r.d_cnt, r.count_bin.data(), n * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(r.d_suf, suf.data(), suf.size() * 8, hipMemcpyHostToDevice));
	HIPCHK(r.d_sorted.alloc(n * W + 2));
	kmxk::rest_expand(r.d_h2i, r.d_pre, r.d_suf, r.map_size, W, r.k, r.pre_len, r.d_sorted, m->stream);
	r.host_valid = true;
	return rest_build_accel(m);
}

static int kmx_finish_impl(kmx_model *m)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (m->state != ST_BUILDING) return fail(KMX_E_STATE, "finish before begin");
	HIPCHK(hipSetDevice(m->device));
	if (m->stg_n) TRY(process_block(m, 0, m->stg_n, true));   // push_last_to_array; an empty tail is skipped (divergence D1)
	m->stg_n = 0;
	TRY(flush_pending_commit(m));
	TRY(kmback_flush(m));
	u64 *hw = m->h_words;                                            // pinned: the copies are enqueued, one wait for all of them
	HIPCHK(hipMemcpyAsync(hw, m->d_stats, ST_N * 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipMemcpyAsync(hw + HW_NREST, m->d_rest_n, 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	memcpy(m->h_stats, hw, ST_N * 8);
	const unsigned long long n_rest = hw[HW_NREST];
	if (m->h_stats[ST_BAD_COUNT]) {
		m->state = ST_EMPTY;
		return fail(KMX_E_RANGE, "%llu k-mers with a count outside [ci=%d, cs=%d]", (unsigned long long)m->h_stats[ST_BAD_COUNT], m->ci, m->cs);
	}
	if (m->prof.on) {
		double before = 0, after = 0;
		for (int c = 0; c < KC_N; c++) if (c != KC_QUERY) before += m->kc_seconds[c];
		prof_collect(m);
		for (int c = 0; c < KC_N; c++) if (c != KC_QUERY) after += m->kc_seconds[c];
		m->t_insert_kernels = after - before;                   // HIP-event time inside the insert kernels of this build
	}
	TRY(build_rest(m, n_rest));
	fill_model_dev(m);
	m->state = ST_READY;
	return KMX_OK;
}

static int build_common(kmx_model *m, int k, const u64 *d_kmers, const u32 *d_counts, u64 n, u64 n_total)
{
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipEventRecord(m->ev0, m->stream));
	HIPCHK(hipMemsetAsync(m->d_nbf, 0, 24, m->stream));
	HIPCHK(hipMemsetAsync(m->d_stats, 0, ST_N * 8, m->stream));
	kmxk::histogram(d_counts, n, m->ci, m->cs, m->bf_num, m->d_nbf, m->d_stats, m->stream);    // pass 1
	HIPCHK(hipMemcpyAsync(m->h_words + HW_NBF, m->d_nbf, 24, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipMemcpyAsync(m->h_words + HW_BAD, m->d_stats + ST_BAD_COUNT, 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	const u64 nbf[3] = {m->h_words[HW_NBF], m->h_words[HW_NBF + 1], m->h_words[HW_NBF + 2]}, bad = m->h_words[HW_BAD];
	if (bad) return fail(KMX_E_RANGE, "%llu k-mers with a count outside [ci=%d, cs=%d]", (unsigned long long)bad, m->ci, m->cs);
	const auto t0 = std::chrono::steady_clock::now();
	TRY(kmx_begin(m, k, (const uint64_t *)nbf, n_total));
	if (m->dbg_ctrl) hipStreamSynchronize(m->stream);
	const auto t1 = std::chrono::steady_clock::now();
	TRY(kmx_insert_batch_dev(m, (const uint64_t *)d_kmers, d_counts, n));
	if (m->dbg_ctrl) hipStreamSynchronize(m->stream);
	const auto t2 = std::chrono::steady_clock::now();
	TRY(kmx_finish(m));
	if (m->dbg_ctrl) {
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
		fprintf(stderr, "[kmx] build: begin (allocate + clear) %.1f ms of which hipMalloc %.1f ms, insert %.1f ms, finish (last block + rest table) %.1f ms\n", ms(t0, t1), (double)kmx_malloc_ns.exchange(0) * 1e-6, ms(t1, t2), ms(t2, std::chrono::steady_clock::now()));
	}
	HIPCHK(hipEventRecord(m->ev1, m->stream));
	HIPCHK(hipEventSynchronize(m->ev1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, m->ev0, m->ev1));
	m->t_total = ms * 1e-3;
	return KMX_OK;
}

static int kmx_build_dev_impl(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_model_k(k));
	return build_common(m, k, (const u64 *)d_kmers, (const u32 *)d_counts, n, n);
}

static int kmx_build_host_impl(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	TRY(check_model_k(k));
	if (n && (!kmers || !counts)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipEventRecord(m->ev0, m->stream));
	// pass 1 on the host cores (kmodel.hpp:423-428): the class histogram of the caller's counts, in parallel
	u64 nbf[3] = {0, 0, 0}, bad = 0;
	{
		const unsigned hw = std::thread::hardware_concurrency();
		const int T = (int)std::max<u64>(1, std::min<u64>(std::min<unsigned>(hw ? hw : 1, 16), n / 1000000 + 1));
		std::vector<u64> acc((size_t)T * 8, 0);
		auto work = [&](int t) {
			const u64 per = (n + T - 1) / T, lo = (u64)t * per, hi = std::min<u64>(n, lo + per);
			u64 a[4] = {0, 0, 0, 0};
			for (u64 i = lo; i < hi; i++) {
				const u32 c = counts[i];
				if (c < (u32)m->ci || c > (u32)m->cs) a[3]++;
				else if (c < (u32)(m->ci + m->bf_num)) a[c - (u32)m->ci]++;
			}
			for (int q = 0; q < 4; q++) acc[(size_t)t * 8 + q] = a[q];
		};
		if (T == 1) work(0);
		else {
			std::vector<std::thread> th;
			for (int t = 0; t < T; t++) th.emplace_back(work, t);
			for (auto &x : th) x.join();
		}
		for (int t = 0; t < T; t++) { for (int q = 0; q < 3; q++) nbf[q] += acc[(size_t)t * 8 + q]; bad += acc[(size_t)t * 8 + 3]; }
	}
	if (bad) return fail(KMX_E_RANGE, "%llu k-mers with a count outside [ci=%d, cs=%d]", (unsigned long long)bad, m->ci, m->cs);
	TRY(kmx_begin(m, k, (const uint64_t *)nbf, n));
	TRY(kmx_insert_batch(m, kmers, counts, n));                  // pinned double-buffered hipMemcpyAsync under the rounds
	TRY(kmx_finish(m));
	HIPCHK(hipEventRecord(m->ev1, m->stream));
	HIPCHK(hipEventSynchronize(m->ev1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, m->ev0, m->ev1));
	m->t_total = ms * 1e-3;
	return KMX_OK;
}

// KModel::init(db_file) (kmodel.hpp:57-87).  The host does I/O only: it counts the classes over the record file (pass 1,
// kmodel.hpp:423-428: one parallel scan of the counter bytes) while a producer thread already copies the RAW records of
// the first batches into pinned slots; a copy stream moves a slot to the device (hipMemcpyAsync) while the model's stream
// is still inserting the previous batch; the records are decoded there (k_kmc_decode: prefix lookup, byte swaps,
// packing) and inserted.  ONE decode of the database, none of it on the host.  Databases that hold records outside the
// header's [min_count, max_count] (ReadNextKmer skips those; KMC itself never writes them) take the host decoder
// instead, and so does KMX_KMC_HOST_DECODE=1 (test hook).
namespace {
struct FeedSlot {
	unsigned char *raw = nullptr;     // GPU decode: record bytes
	u64 *km = nullptr;                // host decode: packed k-mers / counts
	u32 *cnt = nullptr;
	size_t n = 0;
	uint64_t rec0 = 0;
	bool full = false, last = false;
};
}   // namespace

// the feed of KModel::init(db) on the handle (kmx_model::KmcFeed) for this database, its prefix LUT(s) on the device: file ->
// the handle's pinned buffer (parallel preads into memory that is resident already) -> device
static bool feed_alloc(kmx_model *m, size_t B, size_t rb, int W, const kmx::KmcListing &db)
{
	auto &F = m->feed;
	const size_t n_lut = db.lut_entries();
	return hipSetDevice(m->device) == hipSuccess && F.ensure(F.RAW | F.DEV | F.LUT, B, rb, W, n_lut) == hipSuccess &&
	       n_lut && db.read_lut((uint64_t *)F.h_lut.get()) && hipMemcpy(F.d_lut, F.h_lut, n_lut * 8, hipMemcpyHostToDevice) == hipSuccess;
}

// a database that cannot be opened is KMX_E_IO, unless its header was read and gives a k no model takes (a KMC database of
// k = 3 is refused as kmx_build_dev refuses k = 3)
static int kmc_open_failed(const kmx::KmcListing &db, const char *db_prefix)
{
	if (db.kmer_length() >= 1 && db.kmer_length() < 4) return check_model_k((int)db.kmer_length());
	return fail(KMX_E_IO, "can't open the kmer_data_base %s: %s", db_prefix, db.error().c_str());
}

static int kmx_build_from_kmc_impl(kmx_model *m, const char *db_prefix)
{
	if (!m || !db_prefix) return fail(KMX_E_ARG, "null argument");
	const char *tr = getenv("KMX_INIT_TRACE");                       // wall-clock phase times on stderr (no extra synchronisation)
	const bool trace = tr && atoi(tr);
	const auto t_start = std::chrono::steady_clock::now();
	auto lap = [&](const char *what) { if (trace) fprintf(stderr, "[kmx] init(db) %-28s at %7.2f ms\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() * 1e3); };
	kmx::KmcListing db;
	if (!db.open(db_prefix, false)) return kmc_open_failed(db, db_prefix);
	unsigned hw = std::thread::hardware_concurrency();
	const int T = hw > 32 ? 16 : (hw > 1 ? (int)hw / 2 : 1);          // per activity: pass 1 and the producer run side by side
	db.set_threads(T);
	const int k = (int)db.kmer_length(), W = db.words();
	const size_t B = size_t(1) << 23;
	const size_t rb = db.record_bytes();
	HIPCHK(hipSetDevice(m->device));
	lap("database open");
	// ONE PASS (KMX_ONE_PASS=1 under KMX_TEST_HOOKS): the whole listing is streamed to the device and decoded there
	// once -- pread of batch b + 1 under copy + decode of batch b --, the classes are counted ON the device (k_histogram), and the
	// build runs on the resident listing (build_common = kmx_build_dev).  No host scan; but no insert can start before the last
	// batch has arrived (every length is a function of the class counts), so the stream is not hidden under the rounds any more:
	// measured 10^8 31-mers, same box, profiles/r05_one_pass_ab.txt.  Needs N * (8 W + 4) bytes of HBM beside the model; records
	// outside the header's count range (KMC never writes them) are not skipped here -- the two-pass path below is the product.
	if (const char *op = hook_env("KMX_ONE_PASS")) if (op[0] == '1') {
		const u64 N = db.records();
		if (!feed_alloc(m, B, rb, W, db)) return fail(KMX_E_NOMEM, "pinned / device buffers for the listing feed could not be allocated");
		DevBuf<u64> all_k;
		DevBuf<u32> all_c;
		HIPCHK(all_k.alloc(std::max<u64>(N, 1) * W));
		HIPCHK(all_c.alloc(std::max<u64>(N, 1)));
		auto &F = m->feed;
		hipStream_t st = m->stream;
		KmcDecode kd;
		kd.lut = F.d_lut; kd.n_lut = db.lut_entries() - 1; kd.prefix_mask = db.prefix_mask();
		kd.rec_bytes = (u32)rb; kd.suf_bytes = db.suffix_bytes(); kd.cnt_bytes = db.counter_bytes();
		HIPCHK(hipEventRecord(F.ev_free[0], st)); HIPCHK(hipEventRecord(F.ev_free[1], st));
		HIPCHK(hipEventRecord(F.ev_copied[0], F.copy)); HIPCHK(hipEventRecord(F.ev_copied[1], F.copy));
		int s2 = 0;
		for (u64 done = 0; done < N; done += B, s2 ^= 1) {
			const u64 c = std::min<u64>(B, N - done);
			HIPCHK(hipEventSynchronize(F.ev_copied[s2]));                     // the pinned slot has been read (two batches ago)
			db.copy_records(done, c, F.raw[s2]);
			HIPCHK(hipStreamWaitEvent(F.copy, F.ev_free[s2], 0));
			HIPCHK(hipMemcpyAsync(F.draw[s2], F.raw[s2], c * rb, hipMemcpyHostToDevice, F.copy));
			HIPCHK(hipEventRecord(F.ev_copied[s2], F.copy));
			HIPCHK(hipStreamWaitEvent(st, F.ev_copied[s2], 0));
			kd.recs = F.draw[s2];
			kmxk::kmc_decode(kd, W, done, c, all_k + done * W, all_c + done, st);
			HIPCHK(hipEventRecord(F.ev_free[s2], st));
		}
		if (db.io_failed()) return fail(KMX_E_IO, "reading %s.kmc_suf failed", db_prefix);
		lap("listing enqueued (one pass)");
		const int rc1 = build_common(m, k, all_k, all_c, N, db.kmer_count());
		lap("finish returned");
		hipStreamSynchronize(st);
		return rc1;
	}
	const char *force_host = hook_env("KMX_KMC_HOST_DECODE");
	bool gpu_decode = !(force_host && atoi(force_host));
	FeedSlot slot[2];
	auto &F = m->feed;
	std::mutex mu;
	std::condition_variable cv;
	bool stop = false, alloc_done = false;
	std::thread producer, allocator;
	auto cleanup = [&] {
		{ std::lock_guard<std::mutex> lk(mu); stop = true; for (auto &sl : slot) sl.full = false; }
		cv.notify_all();
		if (producer.joinable()) producer.join();
		if (allocator.joinable()) allocator.join();
		if (F.copy) hipStreamSynchronize(F.copy);
		hipStreamSynchronize(m->stream);
	};
	auto guard = scope_exit(cleanup);                                // also when something throws (bad_alloc in pass 1): threads are joined before the frame goes
	hipEventRecord(m->ev0, m->stream);
	// the buffers of pass 2 are (re)allocated beside pass 1 when this database needs larger ones than the handle holds
	bool ok = false;
	allocator = std::thread([&] {
		const bool good = feed_alloc(m, B, rb, W, db);
		{ std::lock_guard<std::mutex> lk(mu); ok = good; alloc_done = true; }
		cv.notify_all();
	});
	// The producer fills the two slots in turn: raw records (a parallel pread out of the page cache) or, in host mode, decoded
	// k-mers.  In raw mode it needs nothing pass 1 finds out, so it starts as soon as the slots exist and works BESIDE pass 1:
	// when the class counts are known the first two batches already sit in pinned memory.
	auto start_producer = [&](bool raw) {
		producer = std::thread([&, raw] {
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return alloc_done || stop; });
				if (stop || !ok) return;
			}
			for (int s = 0; s < 2; s++) { slot[s].raw = F.raw[s]; slot[s].km = F.km[s]; slot[s].cnt = F.cnt[s]; }
			uint64_t rec = 0;
			if (!raw) db.restart();                                          // kmodel.hpp:430
			for (int s = 0;; s ^= 1) {
				{
					std::unique_lock<std::mutex> lk(mu);
					cv.wait(lk, [&] { return !slot[s].full || stop; });
					if (stop) return;
				}
				size_t got;
				const uint64_t rec0 = rec;
				if (raw) {
					got = (size_t)std::min<uint64_t>(B, db.records() > rec ? db.records() - rec : 0);
					if (got) db.copy_records(rec, got, slot[s].raw);
					rec += got;
				} else got = db.next_batch((uint64_t *)slot[s].km, slot[s].cnt, B);
				{ std::lock_guard<std::mutex> lk(mu); slot[s].n = got; slot[s].rec0 = rec0; slot[s].last = got == 0; slot[s].full = true; }
				cv.notify_all();
				if (!got) return;
			}
		});
	};
	if (gpu_decode) start_producer(true);
	uint64_t nbf[3] = {0, 0, 0}, bad = 0, not_listed = 0;
	int rc = KMX_OK;
	const auto t_p1 = std::chrono::steady_clock::now();
	// pass 1 (kmodel.hpp:423-428), counts only.  Everything waits for it (the sizes depend on it), and it is a copy out of the
	// page cache + a scan: it takes as many threads as the machine has to spare beside the producer's
	const int T1 = hw > 32 ? 32 : T;
	db.count_classes((u32)m->ci, (u32)m->cs, m->bf_num, nbf, &bad, &not_listed, T1);
	const double s_p1 = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_p1).count();
	lap("pass 1 done");
	allocator.join();
	lap("buffers ready");
	if (!ok) return fail(KMX_E_NOMEM, "pinned / device buffers for the listing feed could not be allocated");
	if (not_listed && gpu_decode) {                                  // records outside [min_count, max_count]: only the host decoder skips them
		{ std::lock_guard<std::mutex> lk(mu); stop = true; }
		cv.notify_all();
		producer.join();
		{ std::lock_guard<std::mutex> lk(mu); stop = false; for (auto &sl : slot) sl = FeedSlot(); }
		gpu_decode = false;
	}
	if (!gpu_decode && F.ensure(F.HOST, B, rb, W, 0) != hipSuccess)  // host decoder: pinned k-mer / count slots
		rc = fail(KMX_E_NOMEM, "pinned buffers for the listing feed could not be allocated");
	if (!rc && !gpu_decode) start_producer(false);
	if (!rc && db.io_failed()) rc = fail(KMX_E_IO, "reading %s.kmc_suf failed during pass 1", db_prefix);
	if (!rc && bad) rc = fail(KMX_E_RANGE, "%llu k-mers with a count outside [ci=%d, cs=%d]", (unsigned long long)bad, m->ci, m->cs);
	if (!rc) rc = kmx_begin(m, k, nbf, db.kmer_count());
	lap("begin returned");
	double s_wait = 0;
	if (!rc) {
		KmcDecode kd;
		kd.lut = F.d_lut; kd.n_lut = db.lut_entries() - 1; kd.prefix_mask = db.prefix_mask();
		kd.rec_bytes = (u32)rb; kd.suf_bytes = db.suffix_bytes(); kd.cnt_bytes = db.counter_bytes();
		// pass 2 (kmodel.hpp:68-74).  Batch b travels through slot b%2 and device buffers b%2; its copy is enqueued one
		// batch ahead of its insert, so it runs under the rounds of batch b-1.
		auto enqueue_copy = [&](int s) -> bool {                               // slot s is full
			if (hipStreamWaitEvent(F.copy, F.ev_free[s], 0) != hipSuccess) return false;      // the insert that read the device buffers two batches ago
			if (gpu_decode) { if (hipMemcpyAsync(F.draw[s], slot[s].raw, slot[s].n * rb, hipMemcpyHostToDevice, F.copy) != hipSuccess) return false; }
			else {
				if (hipMemcpyAsync(F.dk[s], slot[s].km, slot[s].n * W * 8, hipMemcpyHostToDevice, F.copy) != hipSuccess) return false;
				if (hipMemcpyAsync(F.dc[s], slot[s].cnt, slot[s].n * 4, hipMemcpyHostToDevice, F.copy) != hipSuccess) return false;
			}
			return hipEventRecord(F.ev_copied[s], F.copy) == hipSuccess;
		};
		auto wait_full = [&](int s) {
			const auto t0 = std::chrono::steady_clock::now();
			std::unique_lock<std::mutex> lk(mu);
			cv.wait(lk, [&] { return slot[s].full; });
			s_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		};
		auto release = [&](int s) {
			{ std::lock_guard<std::mutex> lk(mu); slot[s].full = false; }
			cv.notify_all();
		};
		hipEventRecord(F.ev_free[0], m->stream);
		hipEventRecord(F.ev_free[1], m->stream);
		wait_full(0);
		bool copied = !slot[0].last && enqueue_copy(0);
		if (!slot[0].last && !copied) rc = fail(KMX_E_NODEVICE, "H2D copy failed");
		for (int s = 0; !slot[s].last; s ^= 1) {
			const size_t n = slot[s].n;
			// the next batch: produced meanwhile, copied under this batch's rounds
			wait_full(s ^ 1);
			if (!rc && !slot[s ^ 1].last && !enqueue_copy(s ^ 1)) rc = fail(KMX_E_NODEVICE, "H2D copy failed");
			if (!rc) {
				if (hipStreamWaitEvent(m->stream, F.ev_copied[s], 0) != hipSuccess) rc = fail(KMX_E_NODEVICE, "stream wait failed");
				else {
					if (gpu_decode) { kd.recs = F.draw[s]; kmxk::kmc_decode(kd, W, slot[s].rec0, n, F.dk[s], F.dc[s], m->stream); }
					rc = kmx_insert_batch_dev(m, (const uint64_t *)F.dk[s].get(), F.dc[s], n);
				}
				hipEventRecord(F.ev_free[s], m->stream);                       // everything that reads the device buffers of s is enqueued by now
			}
			hipEventSynchronize(F.ev_copied[s]);                               // the pinned slot has been read
			release(s);
		}
	}
	lap("all batches enqueued");
	if (!rc && db.io_failed()) { rc = fail(KMX_E_IO, "reading %s.kmc_suf failed during pass 2: the model is dropped", db_prefix); m->state = ST_EMPTY; }
	if (!rc) rc = kmx_finish(m);
	lap("finish returned");
	if (!rc) {
		hipEventRecord(m->ev1, m->stream);
		hipEventSynchronize(m->ev1);
		float ms = 0;
		hipEventElapsedTime(&ms, m->ev0, m->ev1);
		m->t_total = ms * 1e-3;
		if (m->dbg_ctrl) fprintf(stderr, "[kmx] init(db): pass 1 %.1f ms, waited %.1f ms for the listing in pass 2, total %.1f ms (%s decode)\n", s_p1 * 1e3, s_wait * 1e3, (double)ms, gpu_decode ? "GPU" : "host");
	}
	return rc;
}

// ------------------------------------------------------------------------------------------ one model, several GPUs
// SURVEY §8e.  One process per GPU; each handle holds ONE rank's share of a single model.  What the reference does with
// n_bits OpenMP threads -- thread i walks buffer i against array (i + t) % n_bits, barrier, rotate (kmodel.hpp:560-565) --
// is done by a ring of GPUs that own the arrays whole: after a round the survivors of a list travel to the owner of the
// next array.  The order-free parts (Bloom filters, back filters, km_back: set_bit is an OR, kmodel.hpp:576-581) are
// built as per-rank partial filters and merged by OR.  The exchange itself (RCCL all-to-all / send-recv / broadcast)
// is the caller's: kmcex_amd/dist.py drives these entry points through torch.distributed.
static int kmx_count_classes_dev_impl(kmx_model *m, const uint32_t *d_counts, uint64_t n, uint64_t n_bf[3])
{
	if (!m || !n_bf) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipMemsetAsync(m->d_nbf, 0, 24, m->stream));
	HIPCHK(hipMemsetAsync(m->d_stats, 0, ST_N * 8, m->stream));
	kmxk::histogram((const u32 *)d_counts, n, m->ci, m->cs, m->bf_num, m->d_nbf, m->d_stats, m->stream);    // pass 1 (kmodel.hpp:423-428)
	u64 bad = 0;
	HIPCHK(hipMemcpyAsync(n_bf, m->d_nbf, 24, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipMemcpyAsync(&bad, m->d_stats + ST_BAD_COUNT, 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	if (bad) return fail(KMX_E_RANGE, "%llu k-mers with a count outside [ci=%d, cs=%d]", (unsigned long long)bad, m->ci, m->cs);
	return KMX_OK;
}

static int kmx_shard_begin_impl(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total, int rank, int world)
{
	if (world < 1 || rank < 0 || rank >= world) return fail(KMX_E_ARG, "bad rank %d of %d", rank, world);
	TRY(kmx_begin_impl(m, k, n_bf, n_total));                   // whole-model sizes (kmodel.hpp:402-456): every rank allocates every array
	m->ring = true; m->ring_rank = rank; m->ring_world = world;
	m->bd.kmers = m->d_stg_kmers;                              // the lists a rank attempts are imported into the block staging area
	m->bd.counts = m->d_stg_counts;
	return KMX_OK;
}

// Front end of this rank's slice of the listing (kmodel.hpp:70-73): Bloom-class k-mers go into this rank's PARTIAL
// filters; coupled-array k-mers are compacted, in listing order, into the caller's buffers (capacity >= n).
static int kmx_shard_classify_dev_impl(kmx_model *m, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint64_t *d_out_kmers, uint32_t *d_out_counts, uint64_t *n_out)
{
	if (!m || !n_out) return fail(KMX_E_ARG, "null argument");
	if (m->state != ST_BUILDING || !m->ring) return fail(KMX_E_STATE, "shard_classify before shard_begin");
	*n_out = 0;
	if (!n) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	TRY(ensure_front_end(m, n));
	const u64 n_chunks = (n + kChunk - 1) / kChunk;
	kmxk::classify_count(m->md, (const u64 *)d_kmers, (const u32 *)d_counts, n, kChunk, m->d_tile_cnt, m->d_tile_off, m->d_totals, m->d_stats, m->blm, m->blm_sweep_every, m->stream, &m->prof);
	HIPCHK(hipMemcpyAsync(m->h_totals, m->d_totals, n_chunks * 4, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	u64 base = 0;
	for (u64 ci = 0, done = 0; ci < n_chunks; ci++) {
		const u64 c = std::min<u64>(kChunk, n - done);
		kmxk::classify_scatter(m->md, (const u64 *)d_kmers + done * m->W, (const u32 *)d_counts + done, c, m->d_tile_off + ci * (kChunk / KMX_CLS_TILE),
		                       (u64 *)d_out_kmers, (u32 *)d_out_counts, base, m->stream);
		base += (u64)m->h_totals[ci];
		done += c;
	}
	HIPCHK(hipGetLastError());
	*n_out = base;
	return KMX_OK;
}

static uint64_t ring_msg_bytes(int k) { return 8ull * KMX_MSG_HDR + (u64)KMX_BUCKET * (8ull * ((k + 31) / 32) + 4); }

// One round t on the lists this rank holds: import, A/B/S/R (the same kernels as the single-GPU build; the lists that
// are elsewhere in the ring are empty here), then every list leaves as a message or, after the last round, goes to the
// rest table (kmodel.hpp:567-571).
static int kmx_ring_round_dev_impl(kmx_model *m, int t, const kmx_ring_list *lists, int n_lists)
{
	if (!m || (n_lists && !lists)) return fail(KMX_E_ARG, "null argument");
	if (m->state != ST_BUILDING || !m->ring) return fail(KMX_E_STATE, "ring_round before shard_begin");
	const int nb = m->nb;
	if (t < 0 || t >= nb || n_lists < 0 || n_lists > nb) return fail(KMX_E_ARG, "bad round %d / %d lists", t, n_lists);
	if (m->km_byte_size == 0) return KMX_OK;                      // divergence D2: no arrays to insert into
	HIPCHK(hipSetDevice(m->device));
	RingLists rl;
	memset(&rl, 0, sizeof rl);
	for (int e = 0; e < n_lists; e++) {
		const kmx_ring_list &l = lists[e];
		if (l.list < 0 || l.list >= nb || rl.e[l.list].active) return fail(KMX_E_ARG, "bad or repeated list %d", l.list);
		if (l.n_host > (int)KMX_BUCKET) return fail(KMX_E_ARG, "list %d longer than a buffer", l.list);
		if (l.n_host >= 0 ? (l.n_host > 0 && (!l.src_kmers || !l.src_counts)) : !l.src_msg) return fail(KMX_E_ARG, "list %d has no source", l.list);
		RingList &r = rl.e[l.list];
		r.active = 1; r.n_host = l.n_host;
		r.src_kmers = (const u64 *)l.src_kmers; r.src_counts = (const u32 *)l.src_counts; r.src_msg = (const u64 *)l.src_msg;
		r.dst_msg = (u64 *)l.dst_msg;
	}
	if (t == 0) steer_passes(m);
	// The winners of a list commit beside the NEXT round's check on this rank, like in the single-GPU build: arrays are owned
	// whole, so the list that visits array a in round t+1 is examined by the rank that committed round t on a -- the claims its
	// detect needs as settled positions are this rank's own (kernels.hip, "A: check + emit claims").
	// (A rank that had no list in the round before -- the short final block -- was not called for it: what it still owes would
	// be committed a round late, beside a check whose detect looks for the delta in the wrong list.  Commit it first.)
	if (m->pending && t != (m->pending_t + 1) % nb) TRY(flush_pending_commit(m));
	const int pp = m->pp;
	kmxk::ring_import(m->md, m->bd, pp, rl, m->d_stg_kmers, m->d_stg_counts, m->stream);
	TRY(run_round(m, t, m->defer, nullptr));
	TRY(kmback_emit(m, t, pp, -1, (u64)n_lists * KMX_BUCKET));
	bool any_out = false;
	for (int i = 0; i < nb; i++) any_out |= rl.e[i].active && rl.e[i].dst_msg;
	if (any_out) kmxk::ring_export(m->md, m->bd, pp ^ 1, rl, m->d_feedback, m->stream);
	for (int i = 0; i < nb; i++)
		if (rl.e[i].active && !rl.e[i].dst_msg) {
			TRY(ensure_rest_capacity(m, (u64)KMX_BUCKET + (u64)nb));
			kmxk::rest_append(m->md, m->bd, pp ^ 1, i, 1, m->d_rest_kmers, m->d_rest_counts, m->d_rest_n, m->d_stale_kmers, m->d_stale_counts, m->d_feedback, m->stream);
		}
	if (t == nb - 1) m->blocks++;
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// Quirk Q1 in the ring: the rank that retired list i in the previous block holds its stale slot 0 (kmodel.hpp:520-527, :539)
static int kmx_ring_stale_dup_dev_impl(kmx_model *m, int first_unused_row)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (m->state != ST_BUILDING || !m->ring) return fail(KMX_E_STATE, "ring_stale_dup before shard_begin");
	if (first_unused_row < 0 || first_unused_row >= m->nb || m->km_byte_size == 0) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	TRY(ensure_rest_capacity(m, (u64)m->nb));
	hipLaunchKernelGGL(k_stale_dup, dim3(1), dim3(64), 0, m->stream, first_unused_row, m->nb, m->W, (const u64 *)m->d_stale_kmers,
	                   (const int *)m->d_stale_counts, m->d_rest_kmers.get(), m->d_rest_counts.get(), m->d_rest_n.get(), m->d_stats.get());
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// this rank's share when its last round is enqueued: statistics and the survivors it retired (device pointers)
static int kmx_shard_local_impl(kmx_model *m, kmx_stats *partial, void **d_rest_kmers, void **d_rest_counts)
{
	if (!m || !partial) return fail(KMX_E_ARG, "null argument");
	if (m->state != ST_BUILDING || !m->ring) return fail(KMX_E_STATE, "shard_local before shard_begin");
	HIPCHK(hipSetDevice(m->device));
	TRY(flush_pending_commit(m));                                 // the arrays are about to be read by the caller's broadcasts
	TRY(kmback_flush(m));
	unsigned long long n_rest = 0;
	int range_ovf = 0;
	HIPCHK(hipMemcpyAsync(m->h_stats, m->d_stats, ST_N * 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipMemcpyAsync(&n_rest, m->d_rest_n, 8, hipMemcpyDeviceToHost, m->stream));
	if (m->range.on && m->range.d_ovf) HIPCHK(hipMemcpyAsync(&range_ovf, m->range.d_ovf, sizeof(int), hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	if (m->h_stats[ST_BAD_COUNT]) return fail(KMX_E_RANGE, "%llu k-mers with a count outside [ci=%d, cs=%d]", (unsigned long long)m->h_stats[ST_BAD_COUNT], m->ci, m->cs);
	if (m->prof.on) prof_collect(m);
	memset(partial, 0, sizeof *partial);
	partial->attempts = m->h_stats[ST_ATTEMPTS]; partial->successes = m->h_stats[ST_SUCCESSES];
	partial->fast_commits = m->h_stats[ST_SUCCESSES] - m->h_stats[ST_SLOW_SUCC];
	partial->contended = m->h_stats[ST_CONTENDED]; partial->finisher_iters = m->h_stats[ST_FIN_ITERS];
	partial->rest_entries = n_rest; partial->blocks = m->blocks; partial->rounds = m->rounds;
	partial->reserved = range_ovf;                                // a fixed-size region of the range partition dropped words: this build is void
	if (d_rest_kmers) *d_rest_kmers = m->d_rest_kmers;
	if (d_rest_counts) *d_rest_counts = m->d_rest_counts;
	return KMX_OK;
}

// The merged model: the caller has OR-merged the filters and broadcast the arrays into this handle's memory
// (kmx_dev_view); `d_rest_*` hold the survivors of ALL ranks (any order: KRestData::build sorts, rest.hpp:95-135).
static int kmx_shard_complete_impl(kmx_model *m, const uint64_t *d_rest_kmers, const int32_t *d_rest_counts, uint64_t n_rest, const kmx_stats *totals)
{
	if (!m || !totals) return fail(KMX_E_ARG, "null argument");
	if (m->state != ST_BUILDING || !m->ring) return fail(KMX_E_STATE, "shard_complete before shard_begin");
	if (n_rest && (!d_rest_kmers || !d_rest_counts)) return fail(KMX_E_ARG, "null rest list");
	HIPCHK(hipSetDevice(m->device));
	if (n_rest && (const u64 *)d_rest_kmers != m->d_rest_kmers) {
		HIPCHK(m->d_rest_kmers.ensure(n_rest * m->W, m->stream));
		HIPCHK(m->d_rest_counts.ensure(n_rest, m->stream));
		HIPCHK(hipMemcpyAsync(m->d_rest_kmers, d_rest_kmers, n_rest * m->W * 8, hipMemcpyDeviceToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(m->d_rest_counts, d_rest_counts, n_rest * 4, hipMemcpyDeviceToDevice, m->stream));
	}
	TRY(build_rest(m, n_rest));
	m->h_stats[ST_ATTEMPTS] = totals->attempts; m->h_stats[ST_SUCCESSES] = totals->successes;
	m->h_stats[ST_SLOW_SUCC] = totals->successes - totals->fast_commits;
	m->h_stats[ST_CONTENDED] = totals->contended; m->h_stats[ST_FIN_ITERS] = totals->finisher_iters;
	m->blocks = totals->blocks; m->rounds = totals->rounds;
	fill_model_dev(m);
	m->ring = false;
	m->range.on = false;
	m->state = ST_READY;
	return KMX_OK;
}

#include "multi_build.h"

#include "range_host.h"

// ------------------------------------------------------------------------------------------ KMC listing (host only)
static int kmx_kmc_info_impl(const char *db_prefix, int *k, uint64_t *total_kmers)
{
	if (!db_prefix) return fail(KMX_E_ARG, "null argument");
	kmx::KmcListing db;
	if (!db.open(db_prefix)) return fail(KMX_E_IO, "can't open the kmer_data_base %s: %s", db_prefix, db.error().c_str());
	if (k) *k = (int)db.kmer_length();
	if (total_kmers) *total_kmers = db.kmer_count();
	return KMX_OK;
}

static int kmx_kmc_read_impl(const char *db_prefix, uint64_t *kmers, uint32_t *counts, uint64_t capacity, uint64_t *n_read)
{
	if (!db_prefix || !kmers || !counts || !n_read) return fail(KMX_E_ARG, "null argument");
	kmx::KmcListing db;
	if (!db.open(db_prefix)) return fail(KMX_E_IO, "can't open the kmer_data_base %s: %s", db_prefix, db.error().c_str());
	const int W = db.words();
	uint64_t n = 0;
	for (size_t got; n < capacity && (got = db.next_batch(kmers + n * W, counts + n, (size_t)(capacity - n))) > 0;) n += got;
	*n_read = n;
	if (db.io_failed()) return fail(KMX_E_IO, "reading %s.kmc_suf failed", db_prefix);
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ query
// Every query entry point holds m->query_mu from its first look at the handle to its return: the slots of m->qfeed (and
// ensure_query_feed's reallocation of them), m->prof's event and span vectors and h_stats[ST_QUERY_*] are used by one
// caller at a time.  The *_locked functions below expect the caller to hold it and to have found the model ST_READY (query_enter).
// The entry of every query call: null model, then the lock (lk holds it until the caller returns), then the state.
static int query_enter(kmx_model *m, std::unique_lock<std::mutex> &lk)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	lk = std::unique_lock<std::mutex>(m->query_mu);
	if (m->state != ST_READY) return fail(KMX_E_STATE, "query before the model is built or loaded");
	return KMX_OK;
}

static int query_packed_dev_locked(kmx_model *m, const uint64_t *d_kmers, uint64_t n, int32_t *d_out)
{
	HIPCHK(hipSetDevice(m->device));
	if (m->prof.count && m->d_stats) {                            // accounting (kmx_set_profile(m, 2)): never the timed kernel
		kmxk::query(m->md, (const u64 *)d_kmers, n, d_out, m->stream, &m->prof, m->d_stats + ST_QUERY_NEIGH);
		u64 got = 0;
		HIPCHK(hipMemcpyAsync(&got, m->d_stats + ST_QUERY_NEIGH, 8, hipMemcpyDeviceToHost, m->stream));
		HIPCHK(hipStreamSynchronize(m->stream));
		m->h_stats[ST_QUERY_NEIGH] = got; m->h_stats[ST_QUERY_N] += n;
		return KMX_OK;
	}
	kmxk::query(m->md, (const u64 *)d_kmers, n, d_out, m->stream, &m->prof);
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

static int kmx_query_packed_dev_impl(kmx_model *m, const uint64_t *d_kmers, uint64_t n, int32_t *d_out)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	return query_packed_dev_locked(m, d_kmers, n, d_out);
}

static int kmx_query_packed_impl(kmx_model *m, const uint64_t *kmers, uint64_t n, int32_t *out)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	if (!n) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	DevBuf<uint64_t> dk;
	DevBuf<int32_t> dout;
	HIPCHK(dk.alloc(n * m->W));
	HIPCHK(dout.alloc(n));
	int rc = hipMemcpyAsync(dk, kmers, n * m->W * 8, hipMemcpyHostToDevice, m->stream) == hipSuccess ? KMX_OK : fail(KMX_E_NODEVICE, "H2D copy failed");
	if (!rc) rc = query_packed_dev_locked(m, dk, n, dout);
	if (!rc && hipMemcpyAsync(out, dout, n * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess) rc = fail(KMX_E_NODEVICE, "D2H copy failed");
	if (hipStreamSynchronize(m->stream) != hipSuccess && !rc) rc = fail(KMX_E_NODEVICE, "query failed");
	return rc;
}

// vector<string> front door (kmodel.hpp:90-116).  The reference splits the vector over t_num threads (:93-96); here the
// batch flows through a three-slot pipeline in chunks: worker threads turn chunk c into packed k-mers inside a pinned slot
// (strpack.cpp: 8 bytes per string over the link instead of k), a copy stream moves it (hipMemcpyAsync), the model's stream
// answers it (k_query), a second copy stream brings the answers back, and the workers hand them to the caller's array --
// chunk c is packed while c-1 is on the GPU and c-2 is copied out.  The work is dealt in tasks of 2^14 strings from one
// atomic counter (pack tasks of chunk c, then copy-out tasks of chunk c-2, and so on): no barrier between the threads.
// A string the packed form cannot express (other characters) is remembered by its index and answered afterwards by the
// byte-string kernel, which hashes the bytes as they are, exactly like the reference does -- the cost of dirty strings is
// proportional to their number; a batch of another length than the model's k travels as bytes altogether.
static const u64 kQuerySub = u64(1) << 14;                     // strings per task
static const size_t kQuerySlotBytes = size_t(32) << 20;        // input bytes per slot

// (caller holds m->query_mu: without it, another caller's copies could still be using the slots freed here)
static int ensure_query_feed(kmx_model *m, size_t in_bytes, size_t answers)
{
	auto &F = m->qfeed;
	HIPCHK(F.to_dev.ensure());
	HIPCHK(F.to_host.ensure());
	for (int s = 0; s < F.S; s++) {
		HIPCHK(F.ev_in[s].ensure());
		HIPCHK(F.ev_k[s].ensure());
		HIPCHK(F.ev_out[s].ensure());
		HIPCHK(F.h_in[s].ensure(in_bytes, m->stream));
		HIPCHK(F.d_in[s].ensure(in_bytes, m->stream));
		if (!answers) continue;                                    // (kmx_count_seqs: the kernels answer nothing)
		HIPCHK(F.h_out[s].ensure(answers, m->stream));
		HIPCHK(F.d_out[s].ensure(answers, m->stream));
	}
	return KMX_OK;
}

// A caller whose slots hold more than the items (kmx_query_seqs: a halo of bases and the chunk's sequence boundaries) fixes
// the chunk, the slot size and the bytes copied in per chunk; in_bytes(c) is asked only after chunk c is staged.
struct SlotShape {
	u64 chunk;
	size_t slot_bytes;
	std::function<size_t(u64)> in_bytes;
	// a caller whose kernels leave something else than one answer per item in d_out[slot] (kmx_correct_seqs: a sparse list):
	// int32 words a slot's output takes, the bytes of it copied back with every chunk, and what the driving thread does with
	// h_out[slot] once chunk c's copy has arrived (non-zero: the call fails with that code)
	size_t answers = 0;
	size_t out_bytes = 0;
	std::function<int(u64, int)> consume;
};

// n items of item_bytes each through the pipeline.  stage(worker, lo, hi, dst): items [lo, hi) -> dst (their place in the
// slot); launch(slot, count) or launch(slot, count, chunk): the kernel from d_in[slot] to d_out[slot] on the model's
// stream, chunk by chunk in order; answers -> out[0 .. n).  out == nullptr: the kernels answer nothing (kmx_count_seqs),
// and a slot is free again once its kernel has run.
// The caller holds m->query_mu.
template <typename STAGE, typename LAUNCH>
static int query_pipeline(kmx_model *m, u64 n, size_t item_bytes, int T, STAGE stage, LAUNCH launch, int32_t *out, const SlotShape *shape = nullptr)
{
	auto &F = m->qfeed;
	u64 C = std::max<u64>(kQuerySub, (kQuerySlotBytes / item_bytes) & ~(kQuerySub - 1));
	C = std::min<u64>(C, (n + kQuerySub - 1) & ~(kQuerySub - 1));
	if (shape) C = shape->chunk;
	const u64 nc = (n + C - 1) / C;
	TRY(ensure_query_feed(m, shape ? shape->slot_bytes : (size_t)C * item_bytes, out ? (size_t)C : (shape ? shape->answers : 0)));
	auto count_of = [&](u64 c) { return std::min<u64>(C, n - c * C); };
	auto subs_of = [&](u64 c) { return (count_of(c) + kQuerySub - 1) / kQuerySub; };
	auto enqueue = [&](u64 c) -> bool {
		const int s = (int)(c % F.S);
		const u64 cn = count_of(c);
		if (hipMemcpyAsync(F.d_in[s], F.h_in[s], shape ? shape->in_bytes(c) : cn * item_bytes, hipMemcpyHostToDevice, F.to_dev) != hipSuccess || hipEventRecord(F.ev_in[s], F.to_dev) != hipSuccess ||
		    hipStreamWaitEvent(m->stream, F.ev_in[s], 0) != hipSuccess) return false;
		if constexpr (std::is_invocable_v<LAUNCH, int, u64, u64>) launch(s, cn, c);
		else launch(s, cn);
		return hipEventRecord(F.ev_k[s], m->stream) == hipSuccess && hipStreamWaitEvent(F.to_host, F.ev_k[s], 0) == hipSuccess &&
		       (!out || hipMemcpyAsync(F.h_out[s], F.d_out[s], cn * 4, hipMemcpyDeviceToHost, F.to_host) == hipSuccess) &&
		       (!(shape && shape->out_bytes) || hipMemcpyAsync(F.h_out[s], F.d_out[s], shape->out_bytes, hipMemcpyDeviceToHost, F.to_host) == hipSuccess) && hipEventRecord(F.ev_out[s], F.to_host) == hipSuccess;
	};
	if (nc == 1 && T == 1) {                                      // a handful of strings: no threads
		stage(0, 0, n, F.h_in[0]);
		if (!enqueue(0) || hipEventSynchronize(F.ev_out[0]) != hipSuccess) return fail(KMX_E_NODEVICE, "query failed");
		if (out) memcpy(out, F.h_out[0], n * 4);
		if (shape && shape->consume) TRY(shape->consume(0, 0));
		return KMX_OK;
	}
	// phase p = the pack tasks of chunk p, then the copy-out tasks of chunk p - 2
	const u64 lag = F.S - 1, n_phase = nc + lag;
	std::vector<u64> first(n_phase + 1, 0);
	for (u64 p = 0; p < n_phase; p++) first[p + 1] = first[p] + (p < nc ? subs_of(p) : 0) + (p >= lag ? subs_of(p - lag) : 0);
	std::unique_ptr<std::atomic<u32>[]> packed(new std::atomic<u32>[nc]), copied(new std::atomic<u32>[nc]), ready(new std::atomic<u32>[nc]);
	for (u64 c = 0; c < nc; c++) { packed[c] = 0; copied[c] = 0; ready[c] = 0; }
	std::atomic<u64> next{0};
	std::atomic<bool> abort{false};
	auto wait_for = [&](auto cond) {                              // short waits: spin, then give the core away
		for (unsigned spins = 0; !cond(); spins++) {
			if (abort.load(std::memory_order_relaxed)) return false;
			if (spins < 256) __builtin_ia32_pause(); else std::this_thread::yield();
		}
		return true;
	};
	std::atomic<bool> worker_threw{false};
	auto worker = [&](int t) {
		u64 p = 0;
		try {                                                        // (`stage` may grow a vector: a worker that throws ends the pipeline with KMX_E_NOMEM, not the process)
		for (;;) {
			const u64 id = next.fetch_add(1, std::memory_order_relaxed);
			if (id >= first[n_phase]) return;
			while (id >= first[p + 1]) p++;
			u64 s = id - first[p];
			const u64 n_pack = p < nc ? subs_of(p) : 0;
			if (s < n_pack) {                                        // pack sub-piece s of chunk p
				const u64 c = p;
				if (c >= (u64)F.S && !wait_for([&] { return copied[c - F.S].load(std::memory_order_acquire) == subs_of(c - F.S); })) return;
				const u64 lo = c * C + s * kQuerySub, hi = std::min<u64>(lo + kQuerySub, c * C + count_of(c));
				stage(t, lo, hi, F.h_in[c % F.S] + (lo - c * C) * item_bytes);
				packed[c].fetch_add(1, std::memory_order_release);
			} else {                                                 // hand sub-piece s of chunk p - lag's answers to the caller
				s -= n_pack;
				const u64 c = p - lag;
				if (!wait_for([&] { return ready[c].load(std::memory_order_acquire) != 0; })) return;
				const u64 lo = c * C + s * kQuerySub, hi = std::min<u64>(lo + kQuerySub, c * C + count_of(c));
				if (out) memcpy(out + lo, F.h_out[c % F.S] + (lo - c * C), (hi - lo) * 4);
				copied[c].fetch_add(1, std::memory_order_release);
			}
		}
		} catch (...) { worker_threw = true; abort = true; }
	};
	// the tasks come from one counter, so the pipeline works with however many workers could be started (a pid-limited
	// container may refuse some of up to 32); with none at all the calling thread cannot both pack and drive: an error
	std::vector<std::thread> th;
	try { th.reserve((size_t)T); } catch (...) { return fail(KMX_E_NOMEM, "out of memory"); }
	for (int t = 0; t < T; t++) {
		try { th.emplace_back(worker, t); } catch (...) { break; }
	}
	if (th.empty()) return fail(KMX_E_NOMEM, "cannot start a worker thread for the query pipeline");
	int rc = KMX_OK;
	auto publish = [&](u64 c) {                                   // chunk c's answers are in its pinned slot
		hipError_t e;
		while ((e = hipEventQuery(F.ev_out[c % F.S])) == hipErrorNotReady) std::this_thread::yield();
		if (e != hipSuccess && !rc) rc = fail(KMX_E_NODEVICE, "query failed");
		if (!rc && shape && shape->consume) rc = shape->consume(c, (int)(c % F.S));
		if (rc) abort = true;
		ready[c].store(1, std::memory_order_release);
	};
	for (u64 c = 0; c < nc && !rc; c++) {
		if (!wait_for([&] { return packed[c].load(std::memory_order_acquire) == subs_of(c); })) { rc = fail(KMX_E_NOMEM, "out of memory in a query worker"); break; }
		if (!enqueue(c)) { rc = fail(KMX_E_NODEVICE, "query pipeline: enqueue failed"); break; }
		if (c >= 1) publish(c - 1);
	}
	if (!rc) publish(nc - 1);
	else abort = true;
	for (auto &x : th) x.join();
	hipStreamSynchronize(F.to_dev); hipStreamSynchronize(F.to_host);
	if (worker_threw && !rc) rc = fail(KMX_E_NOMEM, "out of memory in a query worker");
	if (hipStreamSynchronize(m->stream) != hipSuccess && !rc) rc = fail(KMX_E_NODEVICE, "query failed");
	if (!rc && hipGetLastError() != hipSuccess) rc = fail(KMX_E_NODEVICE, "query kernel failed");
	return rc;
}

static int query_text(kmx_model *m, const KmxStrBatch &sb, uint64_t n, int32_t *out)
{
	std::unique_lock<std::mutex> lk;                              // both passes (packed, then the dirty strings' bytes) under one hold
	TRY(query_enter(m, lk));
	const int len = sb.len, W = m->W;
	if (len < 2 || len > 64 || sb.stride < len) return fail(KMX_E_ARG, "k-mer strings must hold 2..64 characters (got %d, stride %d)", len, sb.stride);
	if (!n) return KMX_OK;
	HIPCHK(hipSetDevice(m->device));
	const int T = (int)std::max<u64>(1, std::min<u64>(std::min(kmx_host_cpus(), 32), n / 8192 + 1));
	auto bytes_pass = [&](const KmxStrBatch &b, u64 cnt, int32_t *dst) {   // the strings as they are -> k_query_ascii
		return query_pipeline(m, cnt, (size_t)len, (int)std::max<u64>(1, std::min<u64>(T, cnt / 8192 + 1)),
		                      [&](int, u64 lo, u64 hi, unsigned char *d) { kmx_gather_strings(b, lo, hi, d); },
		                      [&](int s, u64 cn) { kmxk::query_ascii(m->md, len, m->qfeed.d_in[s], len, cn, m->qfeed.d_out[s], m->stream); }, dst);
	};
	if (len != m->k) return bytes_pass(sb, n, out);              // (another length hashes differently from any k-mer of the model)
	std::vector<std::vector<uint64_t>> dirty((size_t)T);
	TRY(query_pipeline(m, n, (size_t)W * 8, T,
	                   [&](int t, u64 lo, u64 hi, unsigned char *d) { kmx_pack_strings(sb, W, lo, hi, (uint64_t *)d, &dirty[(size_t)t]); },
	                   [&](int s, u64 cn) { kmxk::query(m->md, (const u64 *)m->qfeed.d_in[s].get(), cn, m->qfeed.d_out[s], m->stream, &m->prof); }, out));
	std::vector<const char *> dptr;
	std::vector<uint64_t> didx;
	for (auto &v : dirty) for (uint64_t i : v) { didx.push_back(i); dptr.push_back(sb.ptrs ? sb.ptrs[i] : sb.flat + i * (uint64_t)sb.stride); }
	if (didx.empty()) return KMX_OK;
	std::vector<int32_t> ans(didx.size());
	TRY(bytes_pass(KmxStrBatch{dptr.data(), nullptr, len, len}, (u64)didx.size(), ans.data()));
	for (size_t j = 0; j < didx.size(); j++) out[didx[j]] = ans[j];
	return KMX_OK;
}

static int kmx_query_ascii_impl(kmx_model *m, const char *strs, int len, int stride, uint64_t n, int32_t *out)
{
	if (n && (!strs || !out)) return fail(KMX_E_ARG, "null argument");
	return query_text(m, KmxStrBatch{nullptr, strs, stride, len}, n, out);
}

// the same for n separate strings of `len` characters each (what a vector<string> holds), without concatenating them
static int kmx_query_strings_impl(kmx_model *m, const char *const *strs, int len, uint64_t n, int32_t *out)
{
	if (n && (!strs || !out)) return fail(KMX_E_ARG, "null argument");
	return query_text(m, KmxStrBatch{strs, nullptr, len, len}, n, out);
}

// ------------------------------------------------------------------------------------------ query along sequences
// kmx_query_seqs: the window at every base of n_seqs sequences stored back to back.  The bases travel as they are (1 byte
// per window); k_query_seq builds the windows on the device and answers the clean ones, k_query_ascii_at the ones it
// listed (kernels.hip).  The device list of those positions holds one piece of at most kSeqPiece windows: a longer input
// runs in pieces, two launches each on the model's stream, with no host wait between them.
static const u64 kSeqPiece = u64(1) << 24;                     // windows per piece (the dirty list: 64 MB of u32)
static const u64 kSeqChunk = u64(1) << 22;                     // bases per pinned slot of the host variant

// KMX_SEQ_CHUNK_BASES (test hook): pieces and host chunks of this many windows, so a test crosses many of their boundaries.
// Read at every call (a test sets it after the library is loaded).
static u64 seq_size(u64 dflt)
{
	const char *e = hook_env("KMX_SEQ_CHUNK_BASES");
	const long long x = e ? atoll(e) : 0;
	return x > 0 ? std::min<u64>((u64)x, kSeqPiece) : dflt;
}
static u64 seq_piece() { return seq_size(kSeqPiece); }          // windows per piece of a device variant
static u64 seq_chunk() { return seq_size(kSeqChunk); }          // bases per chunk of a host variant
// worker threads that stage the chunks of n_bases bases
static int seq_workers(u64 n_bases) { return (int)std::max<u64>(1, std::min<u64>(std::min(kmx_host_cpus(), 16), n_bases / 65536 + 1)); }

// The SeqDirty (kmx_types.h) of one piece after the other: the owner of the parity of the two counters.  Only
// ensure_seq_scratch can make one (a call site holds an empty optional until then), so none exists whose counters were not zeroed.
class SeqDirtyCursor;
static int ensure_seq_scratch(kmx_model *m, u64 piece, std::optional<SeqDirtyCursor> &dirty);
class SeqDirtyCursor {
	u32 *list, cap, *cnt;
	int odd = 1;
	SeqDirtyCursor(u32 *l, u32 c, u32 *n) : list(l), cap(c), cnt(n) {}
	friend int ensure_seq_scratch(kmx_model *, u64, std::optional<SeqDirtyCursor> &);

public:
	SeqDirty next() { odd ^= 1; return SeqDirty{list, cap, cnt + odd, cnt + (odd ^ 1)}; }
};

// (caller holds m->query_mu) the dirty list for pieces of `piece` windows + its two counters, both zeroed on the model's stream
static int ensure_seq_scratch(kmx_model *m, u64 piece, std::optional<SeqDirtyCursor> &dirty)
{
	auto &F = m->qfeed;
	HIPCHK(F.d_seq_list.ensure(piece, m->stream));             // (waits first: an earlier _dev call may still be using the old list)
	TRY(ensure(F.d_seq_cnt, 2, true, m->stream));
	dirty = SeqDirtyCursor(F.d_seq_list, (u32)F.d_seq_list.cap(), F.d_seq_cnt);
	return KMX_OK;
}

static int kmx_query_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t *d_out)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	if (!n_seqs || !n_bases) return KMX_OK;
	if (!d_seq || !d_offsets || !d_out) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const u64 piece = seq_piece();
	std::optional<SeqDirtyCursor> dirty;
	TRY(ensure_seq_scratch(m, piece, dirty));
	const SeqView v{(const unsigned char *)d_seq, 0, n_bases, n_bases, (const u64 *)d_offsets, n_seqs};
	for (u64 p0 = 0; p0 < n_bases; p0 += piece)
		kmxk::query_seq(m->md, v, p0, std::min<u64>(piece, n_bases - p0), d_out, dirty->next(), m->stream, &m->prof);
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// The host variants (kmx_query_seqs, kmx_count_seqs) stream the bases through the slots of m->qfeed (query_pipeline):
// chunk c takes the windows [c * C, c * C + cn) and carries the bases [c * C, c * C + nbytes), nbytes = min(cn + k - 1,
// n_bases - c * C), then, at byte off_at, the sequence boundaries that fall inside those bytes, rebased to the chunk and
// deduplicated, between 0 and nbytes.  A sequence cut by the chunk's edges ends at nbytes there, which changes no
// window: a window of the chunk that fits in its sequence also fits in the chunk's bytes.
struct SeqChunks {
	const char *seq;
	const uint64_t *offsets;
	u64 n_seqs, n_bases, k, C, nc;
	size_t off_at;
	std::vector<u64> n_bnd;                                        // boundaries chunk c carries (written by the worker that stages its end)
	SeqChunks(const char *seq_, const uint64_t *offsets_, u64 n_seqs_, u64 k_, u64 chunk)
		: seq(seq_), offsets(offsets_), n_seqs(n_seqs_), n_bases(offsets_[n_seqs_]), k(k_), C(std::min<u64>(chunk, n_bases)),
		  nc((n_bases + C - 1) / C), off_at((size_t)((C + 64 + 7) & ~u64(7))), n_bnd(nc, 0) {}
	u64 nbytes_of(u64 c) const { const u64 c0 = c * C, cn = std::min<u64>(C, n_bases - c0); return std::min<u64>(cn + k - 1, n_bases - c0); }
	SlotShape shape() { return SlotShape{C, off_at + 8 * (size_t)(C + 64), [this](u64 c) { return off_at + 8 * (size_t)n_bnd[c]; }}; }
	// bases [lo, hi) of one chunk -> dst; the task holding the chunk's last window adds the chunk's halo and gets the slot back
	unsigned char *stage_bases(u64 lo, u64 hi, unsigned char *dst) const
	{
		memcpy(dst, seq + lo, hi - lo);
		const u64 c = lo / C, c0 = c * C;
		if (hi != c0 + std::min<u64>(C, n_bases - c0)) return nullptr;
		unsigned char *slot = dst - (lo - c0);
		const u64 cn = hi - c0;
		memcpy(slot + cn, seq + hi, nbytes_of(c) - cn);
		return slot;
	}
	// slots of bases and halo alone (kmx_summarise_seqs: its kernels search the caller's offsets, uploaded once)
	SlotShape bases_shape() { return SlotShape{C, (size_t)(C + 64), [this](u64 c) { return (size_t)nbytes_of(c); }}; }
	// the pipeline's stage: the bases, and with the chunk's last window its boundaries
	void stage(u64 lo, u64 hi, unsigned char *dst)
	{
		unsigned char *slot = stage_bases(lo, hi, dst);
		if (!slot) return;
		const u64 c = lo / C, c0 = c * C, nbytes = nbytes_of(c);
		u64 *bnd = (u64 *)(slot + off_at), nb = 0;
		bnd[nb++] = 0;
		for (u64 i = (u64)(std::upper_bound(offsets, offsets + n_seqs + 1, c0) - offsets); i <= n_seqs && offsets[i] < c0 + nbytes; i++)
			if (offsets[i] - c0 != bnd[nb - 1]) bnd[nb++] = offsets[i] - c0;
		bnd[nb++] = nbytes;
		n_bnd[c] = nb;
	}
	// chunk c in device slot d_slot: its bases, its boundaries (n_seqs_of(c) sequences)
	const u64 *bounds(const unsigned char *d_slot) const { return (const u64 *)(d_slot + off_at); }
	u64 seqs_of(u64 c) const { return n_bnd[c] - 1; }
};

// Every device buffer a host variant of summarise, correct, edit or polish owns for the length of the call: the caller's
// offsets, one record per sequence (want_rec), the bases when the call needs them whole (null: they stream through the
// pinned slots instead), n_aux words of the call's own (the edit list; the offsets of the polished reads) and out (the
// polished bases, allocated when their length is known).  upload allocates (failing is KMX_E_NOMEM) and enqueues the copies;
// records enqueues the copy back.  However the call ends, the model's stream is drained before any of them goes.
template <typename REC>
struct SeqOnDevice {
	kmx_model *m;
	DevBuf<unsigned char> seq, out;
	DevBuf<u64> offs, aux;
	DevBuf<REC> rec;
	~SeqOnDevice() { (void)hipStreamSynchronize(m->stream); }
	int upload(const char *bases, const uint64_t *offsets, u64 n_seqs, bool want_rec, u64 n_aux = 0)
	{
		const u64 n_bases = bases ? offsets[n_seqs] : 0;
		if ((bases && seq.alloc(n_bases) != hipSuccess) || offs.alloc(n_seqs + 1) != hipSuccess || (want_rec && rec.alloc(n_seqs) != hipSuccess) || (n_aux && aux.alloc(n_aux) != hipSuccess))
			return fail(KMX_E_NOMEM, "device memory for %llu bases of %llu sequences could not be allocated", (unsigned long long)n_bases, (unsigned long long)n_seqs);
		if (bases) HIPCHK(hipMemcpyAsync(seq, bases, n_bases, hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(offs, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, m->stream));
		return KMX_OK;
	}
	int records(void *out, u64 n_seqs) { if (out) HIPCHK(hipMemcpyAsync(out, rec.get(), n_seqs * sizeof(REC), hipMemcpyDeviceToHost, m->stream)); return KMX_OK; }   // (null: none asked for)
};

static int kmx_query_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t *out)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	const u64 n_bases = offsets[n_seqs];
	if (!n_bases) return KMX_OK;
	if (!seq || !out) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	SeqChunks sc(seq, offsets, n_seqs, (u64)m->k, seq_chunk());
	std::optional<SeqDirtyCursor> dirty;
	TRY(ensure_seq_scratch(m, sc.C, dirty));
	const SlotShape shape = sc.shape();
	auto &F = m->qfeed;
	return query_pipeline(m, n_bases, 1, seq_workers(n_bases),
		[&](int, u64 lo, u64 hi, unsigned char *dst) { sc.stage(lo, hi, dst); },
		[&](int s, u64 cn, u64 c) {
			kmxk::query_seq(m->md, SeqView{F.d_in[s], 0, sc.nbytes_of(c), sc.nbytes_of(c), sc.bounds(F.d_in[s]), sc.seqs_of(c)}, 0, cn, F.d_out[s], dirty->next(), m->stream, &m->prof);
		}, out, &shape);
}

// kmx_summarise_seqs: kmx_query_seqs' windows and answers, folded per sequence on the device (kernels.hip: k_summarise_seq).
static_assert(sizeof(kmx_seq_summary) == 64 && sizeof(SeqSummary) == 64 && KMX_SEQ_THRESHOLDS == 3, "kmx_seq_summary is 64 bytes");
static_assert(offsetof(kmx_seq_summary, min) == offsetof(SeqSummary, mn) && offsetof(kmx_seq_summary, n_ge) == offsetof(SeqSummary, n_ge) &&
              offsetof(kmx_seq_summary, first_below) == offsetof(SeqSummary, first_below), "SeqSummary (kmx_types.h) is the layout of kmx_seq_summary");

static int seq_thresholds(const int32_t *thr, int n_thr, kmx_seq_summary *recs, SeqSumDev &sd)
{
	if (n_thr < 0 || n_thr > KMX_SEQ_THRESHOLDS) return fail(KMX_E_ARG, "n_thr = %d, not in [0, %d]", n_thr, KMX_SEQ_THRESHOLDS);
	if (n_thr && !thr) return fail(KMX_E_ARG, "null thresholds");
	sd = SeqSumDev{(SeqSummary *)recs, {0, 0, 0}, n_thr};
	for (int j = 0; j < n_thr; j++) sd.thr[j] = thr[j];
	return KMX_OK;
}

// the handle's shared buffers for pieces / chunks of `piece` windows (the dirty list; slot_bytes != 0: the pinned slots too).
// They only ever fail to allocate, and for this call that is KMX_E_NOMEM like its own buffers.
static int ensure_summary_buffers(kmx_model *m, u64 piece, size_t slot_bytes, std::optional<SeqDirtyCursor> &dirty)
{
	if (ensure_seq_scratch(m, piece, dirty) == KMX_OK && (!slot_bytes || ensure_query_feed(m, slot_bytes, 0) == KMX_OK)) return KMX_OK;
	const std::string why = g_err;
	return fail(KMX_E_NOMEM, "the buffers of a sequence summary could not be allocated (%s)", why.c_str());
}

static int kmx_summarise_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, const int32_t *thr, int n_thr, kmx_seq_summary *d_out)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	SeqSumDev sd;
	TRY(seq_thresholds(thr, n_thr, d_out, sd));
	if (!n_seqs) return KMX_OK;
	if (!d_offsets || !d_out || (n_bases && !d_seq)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const u64 piece = seq_piece();
	std::optional<SeqDirtyCursor> dirty;
	TRY(ensure_summary_buffers(m, piece, 0, dirty));
	kmxk::seq_summary_init(sd.rec, n_seqs, m->stream, &m->prof);
	const SeqView v{(const unsigned char *)d_seq, 0, n_bases, n_bases, (const u64 *)d_offsets, n_seqs};
	for (u64 p0 = 0; p0 < n_bases; p0 += piece)
		kmxk::summarise_seq(m->md, v, p0, std::min<u64>(piece, n_bases - p0), sd, dirty->next(), m->stream, &m->prof);
	kmxk::seq_summary_finish(sd.rec, (const u64 *)d_offsets, n_seqs, n_bases, m->k, m->stream, &m->prof);
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// The host variant: the bases go through the pinned slots like kmx_query_seqs' and nothing per base comes back.  A slot holds
// bases and halo only: SeqChunks' rebased, deduplicated boundaries would lose the empty sequences and the true start of a
// sequence cut by a chunk's edge, so the caller's offsets are uploaded once and chunk c's kernels work in the positions of
// the whole input, of which they hold the bases [c * C, c * C + nbytes).  The records stay on the device until the end.
static int kmx_summarise_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, const int32_t *thr, int n_thr, kmx_seq_summary *out)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	SeqSumDev sd;
	TRY(seq_thresholds(thr, n_thr, nullptr, sd));
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	if (!out) return fail(KMX_E_ARG, "null argument");
	const u64 n_bases = offsets[n_seqs];
	if (!n_bases) {
		for (u64 i = 0; i < n_seqs; i++) out[i] = kmx_seq_summary{0, 0, -1, -1, {0, 0, 0}, 0, 0};
		return KMX_OK;
	}
	if (!seq) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	SeqOnDevice<SeqSummary> dev{m};
	TRY(dev.upload(nullptr, offsets, n_seqs, true));
	sd.rec = dev.rec;
	SeqChunks sc(seq, offsets, n_seqs, (u64)m->k, seq_chunk());
	const SlotShape shape = sc.bases_shape();
	std::optional<SeqDirtyCursor> dirty;
	TRY(ensure_summary_buffers(m, sc.C, shape.slot_bytes, dirty));
	kmxk::seq_summary_init(sd.rec, n_seqs, m->stream, &m->prof);
	auto &F = m->qfeed;
	TRY(query_pipeline(m, n_bases, 1, seq_workers(n_bases),
		[&](int, u64 lo, u64 hi, unsigned char *dst) { sc.stage_bases(lo, hi, dst); },
		[&](int s, u64 cn, u64 c) {
			kmxk::summarise_seq(m->md, SeqView{F.d_in[s], c * sc.C, c * sc.C + sc.nbytes_of(c), n_bases, dev.offs, n_seqs}, c * sc.C, cn, sd, dirty->next(), m->stream, &m->prof);
		}, (int32_t *)nullptr, &shape));
	kmxk::seq_summary_finish(sd.rec, dev.offs, n_seqs, n_bases, m->k, m->stream, &m->prof);
	TRY(dev.records(out, n_seqs));
	HIPCHK(hipStreamSynchronize(m->stream));
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ correction along sequences
// kmx_correct_seqs: substitution errors corrected from the answers of kmx_query_seqs (the rule: include/kmx.h; the kernels:
// correct_kernels.h).  A piece of windows needs the weak bits of KMX_CORR_HALO(k) windows beyond each end, so its kernels
// answer [p0 - halo, p0 + n + halo) and decide the sites of [p0, p0 + n): every run edge belongs to exactly one piece, and
// positions, run shapes and records are those of the whole input whatever the cut.
static_assert(sizeof(kmx_seq_correction) == 64 && sizeof(SeqCorrection) == 64, "kmx_seq_correction is 64 bytes");
static_assert(offsetof(kmx_seq_correction, n_weak) == offsetof(SeqCorrection, n_weak) && offsetof(kmx_seq_correction, n_unfixable) == offsetof(SeqCorrection, n_unfixable),
              "SeqCorrection (kmx_types.h) is the layout of kmx_seq_correction");

// the handle's buffers for pieces / chunks of `piece` windows: dirty list and weak bits with both halos, a flag per
// workgroup (slot_bytes != 0: the pinned slots too, `answers` int32 words of output each).  Failing is KMX_E_NOMEM.
static int ensure_correct_buffers(kmx_model *m, u64 piece, size_t slot_bytes, size_t answers, std::optional<SeqDirtyCursor> &dirty)
{
	auto &F = m->qfeed;
	const u64 ext = piece + 2 * KMX_CORR_HALO(64);
	if (ensure_seq_scratch(m, ext, dirty) == KMX_OK && F.d_corr_bits.ensure((size_t)((ext + 255) / 256 * 4), m->stream) == hipSuccess &&
	    F.d_corr_flags.ensure((size_t)((piece + 255) / 256), m->stream) == hipSuccess && (!slot_bytes || ensure_query_feed(m, slot_bytes, answers) == KMX_OK)) return KMX_OK;
	return fail(KMX_E_NOMEM, "the buffers of a sequence correction could not be allocated");
}

static int kmx_correct_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, char *d_seq_out, kmx_seq_correction *d_rec)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	if (min_support < 1 || min_support > 64) return fail(KMX_E_ARG, "min_support = %d, not in [1, 64]", min_support);
	if (!n_seqs) return KMX_OK;
	if (!d_offsets || (n_bases && (!d_seq || !d_seq_out))) return fail(KMX_E_ARG, "null argument");
	if (spans_share(Span{d_seq, n_bases, false}, Span{d_seq_out, n_bases, true})) return fail(KMX_E_ARG, "d_seq_out overlaps d_seq");
	HIPCHK(hipSetDevice(m->device));
	const u64 piece = seq_piece(), H = KMX_CORR_HALO(m->k);
	std::optional<SeqDirtyCursor> dirty;
	TRY(ensure_correct_buffers(m, piece, 0, 0, dirty));
	auto &F = m->qfeed;
	kmxk::seq_correction_init((SeqCorrection *)d_rec, (const u64 *)d_offsets, n_seqs, n_bases, m->k, m->stream, &m->prof);
	if (n_bases) HIPCHK(hipMemcpyAsync(d_seq_out, d_seq, n_bases, hipMemcpyDeviceToDevice, m->stream));
	const CorrDev cd{(SeqCorrection *)d_rec, (unsigned char *)d_seq_out, nullptr, 0, thr, min_support};
	const SeqView v{(const unsigned char *)d_seq, 0, n_bases, n_bases, (const u64 *)d_offsets, n_seqs};
	for (u64 p0 = 0; p0 < n_bases; p0 += piece) {
		const u64 cn = std::min<u64>(piece, n_bases - p0);
		kmxk::correct_piece(m->md, v, p0, cn, p0 > H ? p0 - H : 0, std::min<u64>(p0 + cn + H, n_bases), F.d_corr_bits, cd, F.d_corr_flags, dirty->next(), m->stream, &m->prof);
	}
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// The host variant: the bases go through the pinned slots with a halo on BOTH sides (a slot = kCorrPad bytes, of which the
// last min(halo, c0) hold the bases before the chunk, then the chunk and halo + k - 1 bases behind it); the caller's offsets
// are uploaded once and the kernels work in the positions of the whole input (DESIGN.md 3.7's chunk trap).  What comes back
// is sparse: chunk c's kernels append (position - c0) << 2 | code to a list in d_out[slot], sized for the worst case of a
// chunk (a tried site needs a run edge, runs lie >= 2 windows apart and two sites need a run longer than k: fewer than one
// site per 3 windows; the list takes cn / 2 + 8); the count and the first cn / 16 + 16 entries travel with every chunk, the
// rare longer list is fetched when its count arrives.  The corrections are applied to seq_out after the last chunk, so an
// in-place call never feeds a corrected base to a later chunk.
static const size_t kCorrPad = 256;
static int kmx_correct_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, char *seq_out, kmx_seq_correction *rec)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	if (min_support < 1 || min_support > 64) return fail(KMX_E_ARG, "min_support = %d, not in [1, 64]", min_support);
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	const u64 n_bases = offsets[n_seqs];
	if (!n_bases) {
		if (rec) memset(rec, 0, n_seqs * sizeof *rec);
		return KMX_OK;
	}
	if (!seq || !seq_out) return fail(KMX_E_ARG, "null argument");
	if (seq_out != seq && spans_share(Span{seq, n_bases, false}, Span{seq_out, n_bases, true})) return fail(KMX_E_ARG, "seq_out overlaps seq (only seq_out == seq is allowed)");
	HIPCHK(hipSetDevice(m->device));
	SeqOnDevice<SeqCorrection> dev{m};
	TRY(dev.upload(nullptr, offsets, n_seqs, rec != nullptr));
	const u64 C = std::min<u64>(seq_chunk(), n_bases), k = (u64)m->k, H = KMX_CORR_HALO(k);
	const u32 fix_cap = (u32)(C / 2 + 8), eager = (u32)std::min<u64>(C / 16 + 16, fix_cap);
	auto g1_of = [&](u64 c0, u64 cn) { return std::min<u64>(c0 + cn + H + k - 1, n_bases); };
	SlotShape shape{C, kCorrPad + (size_t)(C + H + k + 8), [&](u64 c) { const u64 c0 = c * C; return kCorrPad + (size_t)(g1_of(c0, std::min<u64>(C, n_bases - c0)) - c0); }};
	shape.answers = 2 + (size_t)fix_cap;
	shape.out_bytes = (2 + (size_t)eager) * 4;
	std::optional<SeqDirtyCursor> dirty;
	TRY(ensure_correct_buffers(m, C, shape.slot_bytes, shape.answers, dirty));
	auto &F = m->qfeed;
	std::vector<u64> fixes;                                        // position << 2 | code
	shape.consume = [&](u64 c, int s) -> int {
		u32 *h = (u32 *)F.h_out[s].get();
		const u32 n = h[0];
		if (n > fix_cap) return fail(KMX_E_STATE, "the correction list of a chunk overflowed (%u > %u)", n, fix_cap);
		if (n > eager && (hipMemcpyAsync(h + 2 + eager, (u32 *)F.d_out[s].get() + 2 + eager, (size_t)(n - eager) * 4, hipMemcpyDeviceToHost, F.to_host) != hipSuccess ||
		                  hipStreamSynchronize(F.to_host) != hipSuccess)) return fail(KMX_E_NODEVICE, "D2H copy failed");
		try { for (u32 i = 0; i < n; i++) fixes.push_back(((c * C + (h[2 + i] >> 2)) << 2) | (h[2 + i] & 3)); }
		catch (...) { return fail(KMX_E_NOMEM, "out of host memory"); }
		return KMX_OK;
	};
	kmxk::seq_correction_init(dev.rec, dev.offs, n_seqs, n_bases, m->k, m->stream, &m->prof);
	CorrDev cd{dev.rec, nullptr, nullptr, fix_cap, thr, min_support};
	TRY(query_pipeline(m, n_bases, 1, seq_workers(n_bases),
		[&](int, u64 lo, u64 hi, unsigned char *dst) {
			const u64 c0 = lo / C * C, cn = std::min<u64>(C, n_bases - c0);
			unsigned char *slot = dst - (lo - c0);
			memcpy(dst + kCorrPad, seq + lo, hi - lo);
			if (seq_out != seq) memcpy(seq_out + lo, seq + lo, hi - lo);
			if (lo == c0) { const u64 hl = std::min<u64>(H, c0); memcpy(slot + kCorrPad - hl, seq + c0 - hl, hl); }
			if (hi == c0 + cn) memcpy(slot + kCorrPad + cn, seq + hi, g1_of(c0, cn) - hi);
		},
		[&](int s, u64 cn, u64 c) {
			const u64 c0 = c * C, hl = std::min<u64>(H, c0);
			(void)hipMemsetAsync(F.d_out[s], 0, 8, m->stream);
			cd.fix = (u32 *)F.d_out[s].get();
			const SeqView v{F.d_in[s] + (kCorrPad - hl), c0 - hl, g1_of(c0, cn), n_bases, dev.offs, n_seqs};
			kmxk::correct_piece(m->md, v, c0, cn, c0 - hl, std::min<u64>(c0 + cn + H, n_bases), F.d_corr_bits, cd, F.d_corr_flags, dirty->next(), m->stream, &m->prof);
		}, (int32_t *)nullptr, &shape));
	TRY(dev.records(rec, n_seqs));
	HIPCHK(hipStreamSynchronize(m->stream));
	HIPCHK(hipGetLastError());
	for (u64 f : fixes) seq_out[f >> 2] = "ACGT"[f & 3];
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ edits along sequences
// kmx_edit_seqs: substitutions and single-base insertions / deletions from the answers of kmx_query_seqs (the rule:
// include/kmx.h; the kernels: edit_kernels.h, edit_device.hip).  A run that touches an end of its sequence takes other
// candidates than one inside, however long it is, so no halo of fixed width decides a site: the weak bits of the whole input
// are written first (n_bases / 8 bytes on the handle), piece by piece, then the sites are decided piece by piece.  Both passes
// need the bases on the device, so the host variant uploads them whole instead of streaming them through the pinned slots.
static_assert(sizeof(kmx_seq_edits) == 80 && sizeof(SeqEdits) == 80 && sizeof(kmx_edit) == 8, "kmx_seq_edits is 80 bytes");
static_assert(offsetof(kmx_seq_edits, n_sub) == offsetof(SeqEdits, n_sub) && offsetof(kmx_seq_edits, n_ins) == offsetof(SeqEdits, n_ins) &&
              offsetof(kmx_seq_edits, out_len) == offsetof(SeqEdits, out_len), "SeqEdits (kmx_types.h) is the layout of kmx_seq_edits");

static int edit_args(int min_support, int ops)
{
	if (min_support < 1 || min_support > 64) return fail(KMX_E_ARG, "min_support = %d, not in [1, 64]", min_support);
	if (ops < 1 || ops > 7) return fail(KMX_E_ARG, "ops = %d, not a non-empty subset of KMX_EDIT_OPS_SUB | _DEL | _INS", ops);
	return KMX_OK;
}

// records, weak bits and sites of a batch on device buffers, enqueued: the edits lie unsorted in d_edits, their number in
// d_edit_cnt[0].  Arguments checked, the handle's query lock held, n_seqs and n_bases > 0.
static int edit_seqs_enqueue(kmx_model *m, const unsigned char *d_seq, const u64 *d_offs, u64 n_seqs, u64 n_bases, int32_t thr, int min_support, int ops, u64 *d_edits, u64 capacity, SeqEdits *d_rec)
{
	const u64 piece = seq_piece(), pa = (piece + 255) / 256 * 256;
	auto &F = m->qfeed;
	std::optional<SeqDirtyCursor> dirty;
	if (ensure_correct_buffers(m, pa, 0, 0, dirty) != KMX_OK || F.d_edit_bits.ensure((size_t)((n_bases + 255) / 256 * 4 + 2), m->stream) != hipSuccess ||
	    F.d_edit_cnt.ensure(2, m->stream) != hipSuccess)
		return fail(KMX_E_NOMEM, "the buffers of a sequence edit could not be allocated");
	kmxk::seq_edits_init(d_rec, d_offs, n_seqs, n_bases, m->k, m->stream, &m->prof);
	HIPCHK(hipMemsetAsync(F.d_edit_cnt.get(), 0, 8, m->stream));
	const SeqView v{d_seq, 0, n_bases, n_bases, d_offs, n_seqs};
	for (u64 w0 = 0; w0 < n_bases; w0 += pa)
		kmxk::edit_weak_piece(m->md, v, w0, std::min<u64>(pa, n_bases - w0), thr, F.d_edit_bits, dirty->next(), m->stream, &m->prof);
	const EditDev ed{d_rec, d_edits, d_edits ? capacity : 0, F.d_edit_cnt.get(), thr, min_support, ops};
	for (u64 p0 = 0; p0 < n_bases; p0 += piece)
		kmxk::edit_sites_piece(m->md, v, p0, std::min<u64>(piece, n_bases - p0), F.d_edit_bits, ed, F.d_corr_flags, m->stream, &m->prof);
	return KMX_OK;
}

// the list of `found` edits sorted (enqueued)
static int edit_seqs_sort(kmx_model *m, u64 *d_edits, u64 found)
{
	auto &F = m->qfeed;
	if (found > 1) {
		if (F.d_edit_alt.ensure((size_t)found, m->stream) != hipSuccess) return fail(KMX_E_NOMEM, "the buffers of a sequence edit could not be allocated");
		KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
		const hipError_t e = kmxk::edit_sort(d_edits, F.d_edit_alt, found, F.d_edit_tmp, m->stream);
		KPROF_END(&m->prof, m->stream);
		if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of a sequence edit could not be allocated"); }
		HIPCHK(e);
	}
	return KMX_OK;
}

// the call on device buffers: waits once, where the count reaches the host
static int edit_seqs_core(kmx_model *m, const unsigned char *d_seq, const u64 *d_offs, u64 n_seqs, u64 n_bases, int32_t thr, int min_support, int ops, u64 *d_edits, u64 capacity, u64 *n_edits, SeqEdits *d_rec)
{
	TRY(edit_seqs_enqueue(m, d_seq, d_offs, n_seqs, n_bases, thr, min_support, ops, d_edits, capacity, d_rec));
	unsigned long long found = 0;
	HIPCHK(hipMemcpyAsync(&found, m->qfeed.d_edit_cnt.get(), 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	HIPCHK(hipGetLastError());
	if (n_edits) *n_edits = found;
	if (found > capacity || (found && !d_edits)) return fail(KMX_E_RANGE, "%llu edits were found, the list has room for %llu", found, (unsigned long long)capacity);
	return edit_seqs_sort(m, d_edits, found);
}

static int kmx_edit_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, int ops,
                                  kmx_edit *d_edits, uint64_t capacity, uint64_t *n_edits, kmx_seq_edits *d_rec)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	TRY(edit_args(min_support, ops));
	if (!n_seqs) return KMX_OK;
	if (!d_offsets || !n_edits || (n_bases && !d_seq) || (capacity && !d_edits)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	*n_edits = 0;
	if (!n_bases) {
		kmxk::seq_edits_init((SeqEdits *)d_rec, (const u64 *)d_offsets, n_seqs, 0, m->k, m->stream, &m->prof);
		return KMX_OK;
	}
	return edit_seqs_core(m, (const unsigned char *)d_seq, (const u64 *)d_offsets, n_seqs, n_bases, thr, min_support, ops, (u64 *)d_edits, capacity, (u64 *)n_edits, (SeqEdits *)d_rec);
}

static int kmx_edit_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, int ops,
                              kmx_edit *edits, uint64_t capacity, uint64_t *n_edits, kmx_seq_edits *rec)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	TRY(edit_args(min_support, ops));
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	if (!n_edits || (capacity && !edits)) return fail(KMX_E_ARG, "null argument");
	const u64 n_bases = offsets[n_seqs];
	*n_edits = 0;
	if (!n_bases) {
		if (rec) for (u64 i = 0; i < n_seqs; i++) rec[i] = kmx_seq_edits{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		return KMX_OK;
	}
	if (!seq) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const u64 cap = std::min<u64>(capacity, n_bases / 3 + 1);          // more than that is never found
	SeqOnDevice<SeqEdits> dev{m};
	TRY(dev.upload(seq, offsets, n_seqs, rec != nullptr, cap));
	const int rc = edit_seqs_core(m, dev.seq, dev.offs, n_seqs, n_bases, thr, min_support, ops, dev.aux, cap, (u64 *)n_edits, dev.rec);
	if (rc != KMX_OK && rc != KMX_E_RANGE) return rc;
	TRY(dev.records(rec, n_seqs));
	if (rc == KMX_OK && *n_edits) HIPCHK(hipMemcpyAsync(edits, dev.aux.get(), *n_edits * 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	return rc;
}

// the definition of applying a list: per input position the inserted base, then the input byte, its SUB base or nothing
static int kmx_apply_edits_impl(const char *seq, const uint64_t *offsets, uint64_t n_seqs, const kmx_edit *edits, uint64_t n_edits, char *seq_out, uint64_t out_capacity, uint64_t *offsets_out)
{
	if (!offsets || !offsets_out) return fail(KMX_E_ARG, "null argument");
	TRY(check_offsets(offsets, n_seqs));
	const u64 n_bases = offsets[n_seqs];
	if ((n_bases && !seq) || (n_edits && !edits) || (out_capacity && !seq_out)) return fail(KMX_E_ARG, "null argument");
	u64 n_ins = 0, n_del = 0;
	for (u64 i = 0; i < n_edits; i++) {
		const u64 e = edits[i], pos = e >> 8, op = (e >> 4) & 15, code = e & 15;
		if (i && e <= edits[i - 1]) return fail(KMX_E_ARG, "the edit list is not strictly ascending at entry %llu", (unsigned long long)i);
		if (pos >= n_bases || op < KMX_EDIT_SUB || op > KMX_EDIT_INS || code > 3 || (op == KMX_EDIT_DEL && code)) return fail(KMX_E_ARG, "entry %llu of the edit list is not an edit of this input", (unsigned long long)i);
		if (i && (edits[i - 1] >> 8) == pos && op != KMX_EDIT_INS) return fail(KMX_E_ARG, "two of SUB / DEL at position %llu", (unsigned long long)pos);
		n_ins += op == KMX_EDIT_INS;
		n_del += op == KMX_EDIT_DEL;
	}
	if (n_bases + n_ins - n_del > out_capacity) return fail(KMX_E_RANGE, "the edited sequences take %llu bytes, seq_out has %llu", (unsigned long long)(n_bases + n_ins - n_del), (unsigned long long)out_capacity);
	u64 i = 0, o = 0, u = 0;
	for (u64 p = 0; p <= n_bases; p++) {
		while (u <= n_seqs && offsets[u] == p) offsets_out[u++] = o;
		if (p == n_bases) break;
		char c = seq[p];
		bool drop = false;
		for (; i < n_edits && (edits[i] >> 8) == p; i++) {
			const u64 op = (edits[i] >> 4) & 15;
			if (op == KMX_EDIT_SUB) c = "ACGT"[edits[i] & 3];
			else if (op == KMX_EDIT_DEL) drop = true;
			else seq_out[o++] = "ACGT"[edits[i] & 3];
		}
		if (!drop) seq_out[o++] = c;
	}
	return KMX_OK;
}

// the same on the device; the list is not validated there: a list that is none gives wrong bytes, never a write outside
// d_seq_out[0, out_capacity) / d_offsets_out[0, n_seqs].  Waits once, for the length of the output.
static int kmx_apply_edits_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, const kmx_edit *d_edits, uint64_t n_edits,
                                    char *d_seq_out, uint64_t out_capacity, uint64_t *d_offsets_out)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	std::lock_guard<std::mutex> lk(m->query_mu);
	if (!d_offsets || !d_offsets_out || (n_bases && !d_seq) || (n_edits && !d_edits) || (out_capacity && !d_seq_out)) return fail(KMX_E_ARG, "null argument");
	if (n_edits >> 32) return fail(KMX_E_ARG, "more than 2^32 edits");
	HIPCHK(hipSetDevice(m->device));
	auto &F = m->qfeed;
	if (F.d_edit_alt.ensure((size_t)(2 * (n_edits + 1)), m->stream) != hipSuccess || F.d_edit_cnt.ensure(2, m->stream) != hipSuccess)
		return fail(KMX_E_NOMEM, "the buffers of an edit application could not be allocated");
	KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
	const hipError_t e = kmxk::edit_apply((const unsigned char *)d_seq, (const u64 *)d_offsets, n_seqs, n_bases, (const u64 *)d_edits, n_edits, F.d_edit_alt, (unsigned char *)d_seq_out, out_capacity,
	                                      (u64 *)d_offsets_out, F.d_edit_cnt.get() + 1, F.d_edit_tmp, m->stream);
	KPROF_END(&m->prof, m->stream);
	if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(KMX_E_NOMEM, "the buffers of an edit application could not be allocated"); }
	HIPCHK(e);
	unsigned long long tot = 0;
	HIPCHK(hipMemcpyAsync(&tot, F.d_edit_cnt.get() + 1, 8, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	const u64 need = n_bases + (tot & 0xFFFFFFFFULL) - (tot >> 32);
	if (need > out_capacity) return fail(KMX_E_RANGE, "the edited sequences take %llu bytes, d_seq_out has %llu", (unsigned long long)need, (unsigned long long)out_capacity);
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ polishing to a fixed point
// kmx_polish_seqs: kmx_edit_seqs' rule iterated per read until a pass finds nothing in it (the rule: include/kmx.h; what runs
// between two passes: polish_device.hip).  Pass 1 reads the caller's buffers in place; pass p > 1 runs the same edit pipeline
// on the reads pass p - 1 edited, compacted into one of two batches on the handle.  A pass waits once: the edit count and the
// totals of the compaction's scan (reads that go on, their bytes, bytes parked) reach the host together, and size the sort,
// the next batch and the parking area of the pass.
static_assert(sizeof(kmx_seq_polish) == 96 && sizeof(SeqPolish) == 96, "kmx_seq_polish is 96 bytes");
static_assert(offsetof(kmx_seq_polish, converged) == offsetof(SeqPolish, converged) && offsetof(kmx_seq_polish, out_len) == offsetof(SeqPolish, out_len) &&
              offsetof(kmx_seq_polish, n_unfixable) == offsetof(SeqPolish, n_unfixable), "SeqPolish (kmx_types.h) is the layout of kmx_seq_polish");
static_assert(KMX_POLISH_MAX_PASSES == POLISH_MAX_PASSES, "the pass limit of kmx_types.h is that of kmx.h");

static int polish_args(int min_support, int ops, int max_passes)
{
	TRY(edit_args(min_support, ops));
	if (max_passes < 1 || max_passes > KMX_POLISH_MAX_PASSES) return fail(KMX_E_ARG, "max_passes = %d, not in [1, %d]", max_passes, KMX_POLISH_MAX_PASSES);
	return KMX_OK;
}

// The passes and the gather on device buffers, n_seqs and n_bases > 0.  d_rec[n_seqs] and d_offs_out[n_seqs + 1] are complete
// and *total = d_offs_out[n_seqs] is on the host when it returns KMX_OK; out_of(total) is asked once, when the length is known,
// for the output buffer (null: the call fails with what out_of reported), of which [0, min(total, out_cap)) is written by
// kernels that are enqueued, not awaited.  A pass waits once: the edit count and the scan's totals arrive together.  When the
// last pass is pass max_passes every length is final after its fold, so the offsets and the total ride on that wait too and
// the pass writes its reads straight to their places in the output: no parking, no scan, no second wait.
template <typename OutOf>
static int polish_passes(kmx_model *m, const unsigned char *d_seq, const u64 *d_offs, u64 n_seqs, u64 n_bases, int32_t thr, int min_support, int ops, int max_passes,
                         SeqPolish *d_rec, u64 *d_offs_out, u64 out_cap, OutOf out_of, u64 *total, int *passes)
{
	auto &F = m->qfeed;
	auto nomem = [] { return fail(KMX_E_NOMEM, "the buffers of a sequence polish could not be allocated"); };
	auto rchk = [&](hipError_t e) { if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return nomem(); } HIPCHK(e); return (int)KMX_OK; };
	auto timed = [&](hipError_t e) { KPROF_END(&m->prof, m->stream); return rchk(e); };
	if (F.d_pol_home.ensure((size_t)n_seqs, m->stream) != hipSuccess || F.d_pol_len.ensure((size_t)(n_seqs + 1), m->stream) != hipSuccess) return nomem();
	if (!F.h_pol_cnt.get() && F.h_pol_cnt.alloc(8) != hipSuccess) return nomem();
	PolishHomes hm;
	for (auto &a : hm.area) a = nullptr;
	hm.area[0] = d_seq;
	const unsigned char *act = d_seq;
	const u64 *offs = d_offs, *ids = nullptr;
	u64 n_act = n_seqs, n_bytes = n_bases, grown = 0;
	u64 *h = F.h_pol_cnt;                                              // pinned: found, the three totals, the output's length
	unsigned char *out = nullptr;
	bool have_out = false;
	// offsets that are none (the device variant does not validate them) can claim more bytes than there are, and more edits
	auto bad_offsets = [] { return fail(KMX_E_ARG, "d_offsets are not the offsets of n_bases bases"); };
	auto take_out = [&]() -> int {
		*total = h[4];
		if (*total > n_bases + grown) return bad_offsets();
		out = out_of(*total);
		have_out = true;
		return out || !std::min<u64>(*total, out_cap) ? (int)KMX_OK : (int)KMX_E_NOMEM;
	};
	int p = 1;
	for (;; p++) {
		const bool last = p == max_passes;
		const u64 cap = n_bytes / 3 + 1;                                // (always enough: include/kmx.h)
		if (F.d_pol_edits.ensure((size_t)cap, m->stream) != hipSuccess || F.d_pol_re.ensure((size_t)n_act, m->stream) != hipSuccess ||
		    F.d_pol_tri.ensure((size_t)(2 * (n_act + 1)), m->stream) != hipSuccess || F.d_pol_kind.ensure((size_t)n_act, m->stream) != hipSuccess ||
		    F.d_pol_delta.ensure((size_t)n_act, m->stream) != hipSuccess) return nomem();
		TRY(edit_seqs_enqueue(m, act, offs, n_act, n_bytes, thr, min_support, ops, F.d_pol_edits, cap, F.d_pol_re));
		PolishTri *tri = last ? nullptr : F.d_pol_tri.get(), *sc = last ? nullptr : tri + (n_act + 1);
		KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
		hipError_t e = kmxk::polish_fold(F.d_pol_re, offs, ids, n_act, n_bytes, d_rec, p, last, tri, sc, F.d_pol_kind, F.d_pol_home, F.d_pol_len, F.d_edit_tmp, m->stream);
		if (e == hipSuccess && last) e = kmxk::polish_offsets(F.d_pol_len, n_seqs, d_offs_out, F.d_edit_tmp, m->stream);
		TRY(timed(e));
		HIPCHK(hipMemcpyAsync(h, F.d_edit_cnt.get(), 8, hipMemcpyDeviceToHost, m->stream));
		if (last) HIPCHK(hipMemcpyAsync(h + 4, d_offs_out + n_seqs, 8, hipMemcpyDeviceToHost, m->stream));
		else HIPCHK(hipMemcpyAsync(h + 1, sc + n_act, sizeof(PolishTri), hipMemcpyDeviceToHost, m->stream));
		HIPCHK(hipStreamSynchronize(m->stream));                        // the pass's one wait
		HIPCHK(hipGetLastError());
		const u64 found = h[0];
		const PolishTri tot = last ? PolishTri{0, 0, 0} : PolishTri{h[1], h[2], h[3]};
		if (found > cap || tot.n > n_act || tot.next > n_bytes + found || tot.park > n_bytes + found) return bad_offsets();
		grown += found;
		if (last) TRY(take_out());
		else if (!found && !tot.park) break;                            // pass 1 found nothing: every read stays where it is
		TRY(edit_seqs_sort(m, F.d_pol_edits, found));
		const int nb = p & 1;
		if (F.d_pol_escan.ensure((size_t)(2 * (found + 1)), m->stream) != hipSuccess || (tot.park && F.d_pol_park[p].ensure((size_t)tot.park, m->stream) != hipSuccess) ||
		    (tot.n && (F.d_pol_act[nb].ensure((size_t)tot.next, m->stream) != hipSuccess || F.d_pol_offs[nb].ensure((size_t)(tot.n + 1), m->stream) != hipSuccess ||
		               F.d_pol_ids[nb].ensure((size_t)tot.n, m->stream) != hipSuccess))) return nomem();
		if (tot.park) hm.area[p] = F.d_pol_park[p];
		unsigned char *park = last ? out : (tot.park ? F.d_pol_park[p].get() : nullptr);
		KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
		TRY(timed(kmxk::polish_apply(act, offs, ids, n_act, n_bytes, F.d_pol_kind, sc, F.d_pol_edits, found, F.d_pol_escan, p, last ? d_offs_out : nullptr, F.d_pol_delta,
		                             tot.n ? F.d_pol_act[nb].get() : nullptr, tot.n ? tot.next : 0, tot.n ? F.d_pol_offs[nb].get() : nullptr, tot.n ? F.d_pol_ids[nb].get() : nullptr,
		                             park, last ? std::min<u64>(*total, out_cap) : tot.park, F.d_pol_home, F.d_edit_tmp, m->stream)));
		if (!tot.n) break;
		act = F.d_pol_act[nb];
		offs = F.d_pol_offs[nb];
		ids = F.d_pol_ids[nb];
		n_act = tot.n;
		n_bytes = tot.next;
	}
	*passes = p;
	if (!have_out) {
		KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
		TRY(timed(kmxk::polish_offsets(F.d_pol_len, n_seqs, d_offs_out, F.d_edit_tmp, m->stream)));
		HIPCHK(hipMemcpyAsync(h + 4, d_offs_out + n_seqs, 8, hipMemcpyDeviceToHost, m->stream));
		HIPCHK(hipStreamSynchronize(m->stream));                        // the final length
		TRY(take_out());
	}
	if (p > 1 || p != max_passes) {                                     // (max_passes = 1: pass 1 has placed every read)
		KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
		kmxk::polish_gather(hm, F.d_pol_home, d_offs_out, n_seqs, out, std::min<u64>(*total, out_cap), m->stream);
		KPROF_END(&m->prof, m->stream);
	}
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

static int kmx_polish_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, int ops, int max_passes,
                                    char *d_seq_out, uint64_t out_capacity, uint64_t *d_offsets_out, kmx_seq_polish *d_rec, uint64_t *passes_run)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	TRY(polish_args(min_support, ops, max_passes));
	if (!n_seqs) return KMX_OK;
	if (!d_offsets || !d_offsets_out || (n_bases && !d_seq) || (out_capacity && !d_seq_out)) return fail(KMX_E_ARG, "null argument");
	if (spans_share(Span{d_seq, n_bases, false}, Span{d_seq_out, out_capacity, true})) return fail(KMX_E_ARG, "d_seq_out overlaps d_seq");
	HIPCHK(hipSetDevice(m->device));
	if (passes_run) *passes_run = 1;
	if (!n_bases) {
		KPROF_BEGIN(&m->prof, KC_QUERY, m->stream);
		kmxk::polish_empty((SeqPolish *)d_rec, (u64 *)d_offsets_out, n_seqs, m->stream);
		KPROF_END(&m->prof, m->stream);
		HIPCHK(hipGetLastError());
		return KMX_OK;
	}
	auto &F = m->qfeed;
	if (!d_rec && F.d_pol_rec.ensure((size_t)n_seqs, m->stream) != hipSuccess) return fail(KMX_E_NOMEM, "the buffers of a sequence polish could not be allocated");
	u64 total = 0;
	int passes = 0;
	TRY(polish_passes(m, (const unsigned char *)d_seq, (const u64 *)d_offsets, n_seqs, n_bases, thr, min_support, ops, max_passes, d_rec ? (SeqPolish *)d_rec : F.d_pol_rec.get(),
	                  (u64 *)d_offsets_out, out_capacity, [&](u64) { return (unsigned char *)d_seq_out; }, &total, &passes));
	if (passes_run) *passes_run = (u64)passes;
	if (total > out_capacity) return fail(KMX_E_RANGE, "the polished sequences take %llu bytes, d_seq_out has %llu", (unsigned long long)total, (unsigned long long)out_capacity);
	return KMX_OK;
}

// The host variant: bases and offsets go up once, reads, offsets and records come down once; the passes are the device variant's.
static int kmx_polish_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, int ops, int max_passes,
                                char *seq_out, uint64_t out_capacity, uint64_t *offsets_out, kmx_seq_polish *rec, uint64_t *passes_run)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	TRY(polish_args(min_support, ops, max_passes));
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	const u64 n_bases = offsets[n_seqs];
	if (!offsets_out || (n_bases && !seq) || (out_capacity && !seq_out)) return fail(KMX_E_ARG, "null argument");
	if (spans_share(Span{seq, n_bases, false}, Span{seq_out, out_capacity, true})) return fail(KMX_E_ARG, "seq_out overlaps seq");
	if (passes_run) *passes_run = 1;
	if (!n_bases) {
		for (u64 i = 0; i <= n_seqs; i++) offsets_out[i] = 0;
		if (rec) for (u64 i = 0; i < n_seqs; i++) rec[i] = kmx_seq_polish{1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		return KMX_OK;
	}
	HIPCHK(hipSetDevice(m->device));
	SeqOnDevice<SeqPolish> dev{m};
	TRY(dev.upload(seq, offsets, n_seqs, true, n_seqs + 1));
	u64 total = 0;
	int passes = 0;
	const int rc = polish_passes(m, dev.seq, dev.offs, n_seqs, n_bases, thr, min_support, ops, max_passes, dev.rec, dev.aux, out_capacity,
	                             [&](u64 t) { const u64 n = std::min<u64>(t, out_capacity); return n && dev.out.alloc(n) == hipSuccess ? dev.out.get() : nullptr; }, &total, &passes);
	if (rc == KMX_E_NOMEM) return fail(KMX_E_NOMEM, "device memory for the polished bases could not be allocated");
	TRY(rc);
	if (passes_run) *passes_run = (u64)passes;
	const u64 n_out = std::min<u64>(total, out_capacity);
	if (n_out) HIPCHK(hipMemcpyAsync(seq_out, dev.out.get(), n_out, hipMemcpyDeviceToHost, m->stream));
	HIPCHK(hipMemcpyAsync(offsets_out, dev.aux.get(), (n_seqs + 1) * 8, hipMemcpyDeviceToHost, m->stream));
	TRY(dev.records(rec, n_seqs));
	HIPCHK(hipStreamSynchronize(m->stream));
	if (total > out_capacity) return fail(KMX_E_RANGE, "the polished sequences take %llu bytes, seq_out has %llu", (unsigned long long)total, (unsigned long long)out_capacity);
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ extension along unique paths
// kmx_extend_seqs: seeds walked to the right through the model's de Bruijn graph (the rule: include/kmx.h; the kernels:
// extend_kernels.h).  The seeds run in chunks of at most kExtChunk: the walk states and live lists on the handle are one
// chunk's.  A chunk is one k_extend_init and ceil(max_ext / steps) launches of k_extend_step, all enqueued at once: the host
// does not read the live count, a launch whose list is empty ends at once.
static_assert(sizeof(kmx_seq_extension) == 32 && sizeof(SeqExtension) == 32 && sizeof(ExtWalk) == 64, "kmx_seq_extension is 32 bytes");
static_assert(offsetof(kmx_seq_extension, seed_occ) == offsetof(SeqExtension, seed_occ) && offsetof(kmx_seq_extension, n_lookahead) == offsetof(SeqExtension, n_lookahead) &&
              offsetof(kmx_seq_extension, sum_occ) == offsetof(SeqExtension, sum_occ), "SeqExtension (kmx_types.h) is the layout of kmx_seq_extension");
static_assert(EXT_DEAD_END == KMX_EXT_DEAD_END && EXT_BRANCH == KMX_EXT_BRANCH && EXT_JOIN == KMX_EXT_JOIN && EXT_CYCLE == KMX_EXT_CYCLE && EXT_MAX_EXT == KMX_EXT_MAX_EXT &&
              EXT_BAD_SEED == KMX_EXT_BAD_SEED, "the stop codes of kmx_types.h are those of kmx.h");

static const u64 kExtChunk = u64(1) << 20;                     // seeds per chunk (64 MB of walk states)
static const u64 kExtRowBytes = u64(1) << 28;                  // device bytes of ext rows a chunk of the host variant may take
static const int kExtSteps = 256;                              // steps of a walk per launch

// KMX_EXTEND_STEPS: steps per launch, read at every call like KMX_SEQ_CHUNK_BASES; KMX_EXTEND_CHUNK_SEEDS (test hook): seeds
// per chunk, so a test crosses many chunk boundaries
static int extend_steps()
{
	const char *e = hook_env("KMX_EXTEND_STEPS");
	const long long x = e ? atoll(e) : 0;
	return x > 0 ? (int)std::min<long long>(x, KMX_EXT_MAX_EXT_LIMIT) : kExtSteps;
}
static u64 extend_chunk(u64 dflt)
{
	const char *e = hook_env("KMX_EXTEND_CHUNK_SEEDS");
	const long long x = e ? atoll(e) : 0;
	return x > 0 ? std::min<u64>((u64)x, kExtChunk) : dflt;
}

static int extend_args(int max_ext, int depth)
{
	if (max_ext < 1 || max_ext > KMX_EXT_MAX_EXT_LIMIT) return fail(KMX_E_ARG, "max_ext = %d, not in [1, %d]", max_ext, KMX_EXT_MAX_EXT_LIMIT);
	if (depth < 0 || depth > KMX_EXT_MAX_DEPTH) return fail(KMX_E_ARG, "depth = %d, not in [0, %d]", depth, KMX_EXT_MAX_DEPTH);
	return KMX_OK;
}

// (caller holds m->query_mu) the handle's buffers for chunks of n seeds.  Failing is KMX_E_NOMEM.
static int ensure_extend_buffers(kmx_model *m, u64 n)
{
	auto &F = m->qfeed;
	if (F.d_ext_walk.ensure((size_t)n, m->stream) == hipSuccess && F.d_ext_lists.ensure((size_t)(2 * n), m->stream) == hipSuccess && F.d_ext_cnt.ensure(3, m->stream) == hipSuccess) return KMX_OK;
	return fail(KMX_E_NOMEM, "the walk states of %llu seeds could not be allocated", (unsigned long long)n);
}

static int kmx_extend_seqs_dev_impl(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int max_ext, int depth, char *d_ext, kmx_seq_extension *d_rec)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	TRY(extend_args(max_ext, depth));
	if (!n_seqs) return KMX_OK;
	if (!d_offsets || !d_ext || (n_bases && !d_seq)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const u64 C = std::min<u64>(extend_chunk(kExtChunk), n_seqs);
	TRY(ensure_extend_buffers(m, C));
	auto &F = m->qfeed;
	HIPCHK(hipMemsetAsync(d_ext, 0, (size_t)(n_seqs * (u64)max_ext), m->stream));
	const int steps = extend_steps();
	for (u64 s0 = 0; s0 < n_seqs; s0 += C) {
		const u64 cn = std::min<u64>(C, n_seqs - s0);
		const ExtDev xd{F.d_ext_walk, d_rec ? (SeqExtension *)d_rec + s0 : nullptr, (unsigned char *)d_ext + s0 * (u64)max_ext, thr, (u32)max_ext, depth};
		kmxk::extend_walks(m->md, SeqView{(const unsigned char *)d_seq, 0, n_bases, n_bases, (const u64 *)d_offsets + s0, cn}, xd, F.d_ext_lists, F.d_ext_cnt, steps, m->stream, &m->prof);
	}
	HIPCHK(hipGetLastError());
	return KMX_OK;
}

// The host variant: of every seed only its last min(length, k) bytes are staged (pinned) and sent, with offsets of their own,
// so a seed shorter than k is still one on the device; a chunk's rows and records come back before the next chunk is staged.
// A chunk holds as many seeds as keep its rows within kExtRowBytes.
static int kmx_extend_seqs_impl(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int max_ext, int depth, char *ext, kmx_seq_extension *rec)
{
	std::unique_lock<std::mutex> lk;
	TRY(query_enter(m, lk));
	TRY(extend_args(max_ext, depth));
	if (!n_seqs) return KMX_OK;
	TRY(check_offsets(offsets, n_seqs));
	if (!ext || (offsets[n_seqs] && !seq)) return fail(KMX_E_ARG, "null argument");
	HIPCHK(hipSetDevice(m->device));
	const u64 k = (u64)m->k, C = std::min<u64>(extend_chunk(std::min<u64>(kExtChunk, std::max<u64>(1, kExtRowBytes / (u64)max_ext))), n_seqs);
	TRY(ensure_extend_buffers(m, C));
	auto &F = m->qfeed;
	PinBuf<unsigned char> h_tail;
	PinBuf<u64> h_offs;
	DevBuf<unsigned char> d_tail, d_rows;
	DevBuf<u64> d_offs;
	DevBuf<SeqExtension> d_rec;
	if (h_tail.alloc((size_t)(C * k)) != hipSuccess || h_offs.alloc((size_t)(C + 1)) != hipSuccess || d_tail.alloc((size_t)(C * k)) != hipSuccess || d_rows.alloc((size_t)(C * (u64)max_ext)) != hipSuccess ||
	    d_offs.alloc((size_t)(C + 1)) != hipSuccess || (rec && d_rec.alloc((size_t)C) != hipSuccess))
		return fail(KMX_E_NOMEM, "the buffers of a chunk of %llu seeds could not be allocated", (unsigned long long)C);
	auto drained = scope_exit([&] { (void)hipStreamSynchronize(m->stream); });   // (the chunk's buffers go when this returns)
	const int steps = extend_steps();
	for (u64 s0 = 0; s0 < n_seqs; s0 += C) {
		const u64 cn = std::min<u64>(C, n_seqs - s0);
		u64 t = 0;
		h_offs[0] = 0;
		for (u64 i = 0; i < cn; i++) {
			const u64 b = offsets[s0 + i + 1], take = std::min<u64>(b - offsets[s0 + i], k);
			memcpy(h_tail + t, seq + (b - take), take);
			h_offs[i + 1] = t += take;
		}
		if (t) HIPCHK(hipMemcpyAsync(d_tail, h_tail, t, hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemcpyAsync(d_offs, h_offs, (cn + 1) * 8, hipMemcpyHostToDevice, m->stream));
		HIPCHK(hipMemsetAsync(d_rows, 0, (size_t)(cn * (u64)max_ext), m->stream));
		const ExtDev xd{F.d_ext_walk, d_rec, d_rows, thr, (u32)max_ext, depth};
		kmxk::extend_walks(m->md, SeqView{d_tail, 0, t, t, d_offs, cn}, xd, F.d_ext_lists, F.d_ext_cnt, steps, m->stream, &m->prof);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(ext + s0 * (u64)max_ext, d_rows.get(), (size_t)(cn * (u64)max_ext), hipMemcpyDeviceToHost, m->stream));
		if (rec) HIPCHK(hipMemcpyAsync(rec + s0, d_rec.get(), cn * sizeof *rec, hipMemcpyDeviceToHost, m->stream));
		HIPCHK(hipStreamSynchronize(m->stream));
	}
	return KMX_OK;
}

#include "count_host.h"
#include "graph_host.h"
#include "unitig_host.h"
#include "map_host.h"
#include "contig_host.h"
#include "resolve_host.h"
#include "pair_host.h"
#include "scaffold_host.h"
#include "pair_path_host.h"
#include "fill_host.h"
#include "reduce_host.h"
#include "lift_host.h"

// ------------------------------------------------------------------------------------------ persistence
static int download_array(kmx_model *m, int which, int index, std::vector<unsigned char> &out)
{
	out.clear();
	if (which == 0 || which == 1 || which == 2) {
		if (which != 2 && (index < 0 || index >= m->bf_num)) return fail(KMX_E_ARG, "bad filter index");
		const u64 nbytes = which == 0 ? m->byte_bf[index] : which == 1 ? m->byte_bf_back[index] : m->byte_km_back;
		const u32 *src = which == 0 ? m->d_bf[index] : which == 1 ? m->d_bf_back[index] : m->d_km_back;
		out.resize(nbytes);
		if (nbytes) HIPCHK(hipMemcpy(out.data(), src, nbytes, hipMemcpyDeviceToHost));
		return KMX_OK;
	}
	if (which < 3 || which > 5 || index < 0 || index >= m->nb) return fail(KMX_E_ARG, "bad array selector");
	const u64 nbytes = m->km_byte_size;
	out.resize(nbytes);
	if (!nbytes) return KMX_OK;
	DevBuf<unsigned char> tmp;
	HIPCHK(tmp.alloc(m->ncells * 2));
	kmxk::cells_to_disk(m->d_cells[index], m->ncells, nbytes, which - 3, tmp, m->stream);
	hipError_t e = hipMemcpyAsync(out.data(), tmp, nbytes, hipMemcpyDeviceToHost, m->stream);
	if (hipStreamSynchronize(m->stream) != hipSuccess || e != hipSuccess) return fail(KMX_E_NODEVICE, "D2H copy failed");
	return KMX_OK;
}

static int kmx_download_impl(kmx_model *m, int which, int index, uint8_t *dst, uint64_t capacity, uint64_t *written)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (m->state == ST_EMPTY) return fail(KMX_E_STATE, "no arrays yet");
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipStreamSynchronize(m->stream));
	std::vector<unsigned char> v;
	TRY(download_array(m, which, index, v));
	if (written) *written = v.size();
	if (v.size() > capacity) return fail(KMX_E_ARG, "buffer too small: need %llu bytes", (unsigned long long)v.size());
	if (!v.empty()) memcpy(dst, v.data(), v.size());
	return KMX_OK;
}

// km.bin (Appendix B.1): u64 n_km, u64 n_bf[bf_num], then bf / bf_back per filter, km_back, and bit_array_1 (value) /
// bit_array_2 (tag) per coupled array.  Streamed: the model's stream de-interleaves one array at a time and copies it
// into a ring of pinned chunks; writer threads pwrite the chunks at their final offsets, so the copy, the page-cache
// writes and the next array's kernel overlap.
namespace {
struct SaveChunk {
	PinBuf<unsigned char> buf;
	Event ready;
	u64 len = 0, off = 0;
	int state = 0;                                              // 0 free, 1 filled (copy enqueued), 2 being written
};
}

static int save_km_bin(kmx_model *m, const std::string &path)
{
	const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
	if (fd < 0) return fail(KMX_E_IO, "cannot write %s", path.c_str());
	u64 head[4] = {m->n_km, 0, 0, 0};
	for (int i = 0; i < m->bf_num; i++) head[1 + i] = m->n_bf[i];
	const u64 head_bytes = 8 * (1 + (u64)m->bf_num);
	bool io_ok = pwrite(fd, head, head_bytes, 0) == (ssize_t)head_bytes;
	constexpr int R = 6, T = 4;
	constexpr u64 CH = 16ull << 20;
	SaveChunk ring[R];
	DevBuf<unsigned char> tmp;
	int rc = KMX_OK;
	for (auto &c : ring)
		if (c.buf.alloc(CH) != hipSuccess || c.ready.ensure() != hipSuccess) rc = fail(KMX_E_NOMEM, "pinned buffers for save could not be allocated");
	if (!rc && m->km_byte_size && tmp.alloc(m->ncells * 2) != hipSuccess) rc = fail(KMX_E_NOMEM, "device buffer for save could not be allocated");
	std::mutex mu;
	std::condition_variable cv;
	bool done = false;
	std::vector<std::thread> writers;
	if (!rc)
		for (int t = 0; t < T; t++)
			writers.emplace_back([&] {
				for (;;) {
					SaveChunk *c = nullptr;
					{
						std::unique_lock<std::mutex> lk(mu);
						cv.wait(lk, [&] {
							for (auto &x : ring) if (x.state == 1) { c = &x; return true; }
							return done;
						});
						if (!c) return;
						c->state = 2;
					}
					bool ok = hipEventSynchronize(c->ready) == hipSuccess;
					for (u64 w = 0; ok && w < c->len;) {
						const ssize_t k = pwrite(fd, c->buf + w, c->len - w, (off_t)(c->off + w));
						if (k <= 0) ok = false; else w += (u64)k;
					}
					{ std::lock_guard<std::mutex> lk(mu); c->state = 0; if (!ok) io_ok = false; }
					cv.notify_all();
				}
			});
	u64 off = head_bytes;
	auto emit = [&](const unsigned char *dsrc, u64 nbytes) {                 // device bytes -> file at `off`
		for (u64 pos = 0; pos < nbytes && !rc; pos += CH) {
			const u64 len = std::min<u64>(CH, nbytes - pos);
			SaveChunk *c = nullptr;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { for (auto &x : ring) if (x.state == 0) { c = &x; return true; } return false; });
			}
			if (hipMemcpyAsync(c->buf, dsrc + pos, len, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipEventRecord(c->ready, m->stream) != hipSuccess) { rc = fail(KMX_E_NODEVICE, "D2H copy failed"); break; }
			c->len = len; c->off = off + pos;
			{ std::lock_guard<std::mutex> lk(mu); c->state = 1; }
			cv.notify_all();
		}
		off += nbytes;
	};
	if (!rc) {
		for (int i = 0; i < m->bf_num; i++) { emit((const unsigned char *)m->d_bf[i], m->byte_bf[i]); emit((const unsigned char *)m->d_bf_back[i], m->byte_bf_back[i]); }
		emit((const unsigned char *)m->d_km_back.get(), m->byte_km_back);
		for (int a = 0; a < m->nb && !rc && m->km_byte_size; a++)
			for (int which = 0; which < 2; which++) {                          // bit_array_1 (value), bit_array_2 (tag)
				kmxk::cells_to_disk(m->d_cells[a], m->ncells, m->km_byte_size, which, tmp, m->stream);   // waits, in stream order, for the copies out of tmp
				emit(tmp, m->km_byte_size);
			}
	}
	{ std::lock_guard<std::mutex> lk(mu); done = true; }
	cv.notify_all();
	// the writers drain what is filled before they see `done` with nothing left
	for (auto &w : writers) w.join();
	hipStreamSynchronize(m->stream);                             // (before the ring and tmp go out of scope)
	if (close(fd) != 0) io_ok = false;
	if (!rc && !io_ok) rc = fail(KMX_E_IO, "short write to %s", path.c_str());
	return rc;
}

// KModel::save (kmodel.hpp:173-206) + KRestData::save_file (rest.hpp:197-221); layouts: Appendix B.1/B.2
static int kmx_save_impl(kmx_model *m, const char *dir)
{
	if (!m || !dir) return fail(KMX_E_ARG, "null argument");
	if (m->state != ST_READY) return fail(KMX_E_STATE, "save before the model is built or loaded");
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipStreamSynchronize(m->stream));
	std::string d(dir);
	FILE *f = fopen((d + "/header").c_str(), "w");
	if (!f) return fail(KMX_E_IO, "cannot write %s/header", dir);
	const bool header_ok = fprintf(f, "number_hash %d\nnumber_bit %d\nci %d\ncs %d\n", m->nh, m->nb, m->ci, m->cs) > 0;
	if ((fclose(f) != 0) | !header_ok) return fail(KMX_E_IO, "short write to %s/header", dir);
	const auto t0 = std::chrono::steady_clock::now();
	TRY(save_km_bin(m, d + "/km.bin"));
	const auto t1 = std::chrono::steady_clock::now();
	TRY(rest_materialize_host(m));
	const auto t2 = std::chrono::steady_clock::now();
	const RestTable &r = m->rest;
	if (!(f = fopen((d + "/rest.bin").c_str(), "wb"))) return fail(KMX_E_IO, "cannot write %s/rest.bin", dir);
	int h[4] = {r.k, r.pre_len, r.map_size, r.pre_buffer_size};
	bool w_ok = fwrite(h, 4, 4, f) == 4 && fwrite(&r.suff_bin_size, 8, 1, f) == 1 && fwrite(&r.entries, 8, 1, f) == 1;
	w_ok = w_ok && fwrite(r.hash2index.data(), 4, r.hash2index.size(), f) == r.hash2index.size();
	w_ok = w_ok && fwrite(r.pre_buffer.data(), 4, r.pre_buffer.size(), f) == r.pre_buffer.size();
	w_ok = w_ok && fwrite(r.suffix_bin.data(), 1, r.suffix_bin.size(), f) == r.suffix_bin.size();
	w_ok = w_ok && fwrite(r.count_bin.data(), 4, r.count_bin.size(), f) == r.count_bin.size();
	if ((fclose(f) != 0) | !w_ok) return fail(KMX_E_IO, "short write to %s/rest.bin", dir);
	if (m->dbg_ctrl) {
		const auto t3 = std::chrono::steady_clock::now();
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
		fprintf(stderr, "[kmx] save: km.bin %.1f ms, rest table to host form %.1f ms, rest.bin %.1f ms\n", ms(t0, t1), ms(t1, t2), ms(t2, t3));
	}
	return KMX_OK;
}

// get_model(save_dir) (kmodel.hpp:680-696) + KModel::load (:209-235) + KRestData::from_file (rest.hpp:163-195)
static int kmx_load_impl(const char *dir, kmx_model **out)
{
	if (!dir || !out) return fail(KMX_E_ARG, "null argument");
	*out = nullptr;
	std::string d(dir);
	FILE *f = fopen((d + "/header").c_str(), "r");
	if (!f) return fail(KMX_E_IO, "load_model: cant't open the header of the model ! (%s/header)", dir);
	char key[64];
	int nh, nb, ci, cs;
	int got = fscanf(f, "%63s %d %63s %d %63s %d %63s %d", key, &nh, key, &nb, key, &ci, key, &cs);
	fclose(f);
	if (got != 8) return fail(KMX_E_IO, "malformed header in %s", dir);
	kmx_model *m = nullptr;
	TRY(kmx_create(ci, cs, nh, nb, &m));
	auto bail = [&](int code) { kmx_destroy(m); return code; };
	// rest.bin first: it carries k
	if (!(f = fopen((d + "/rest.bin").c_str(), "rb"))) return bail(fail(KMX_E_IO, "cannot open %s/rest.bin", dir));
	RestTable &r = m->rest;
	int h[4];
	bool ok = fread(h, 4, 4, f) == 4 && fread(&r.suff_bin_size, 8, 1, f) == 1 && fread(&r.entries, 8, 1, f) == 1;
	if (ok) {
		r.k = h[0]; r.pre_len = h[1]; r.map_size = h[2]; r.pre_buffer_size = h[3];
		if (r.k >= 1 && r.k < 4) { fclose(f); return bail(check_model_k(r.k)); }
		// the lookup takes the suffix as 2 (k - pre_len) bits in whole groups of 4 bases (rest.hpp:143-145)
		ok = r.k >= 4 && r.k <= 64 && r.pre_len >= 1 && r.pre_len <= 12 && r.pre_len <= r.k && (r.k - r.pre_len) % 4 == 0 &&
		     r.map_size == (1 << (2 * r.pre_len)) && r.pre_buffer_size >= 1;
	}
	if (ok) {
		r.suff_group = (r.k - r.pre_len) / 4;
		ok = r.suff_bin_size == r.entries * (u64)r.suff_group;
	}
	if (ok) {
		r.hash2index.resize(r.map_size); r.pre_buffer.resize(r.pre_buffer_size);
		r.suffix_bin.resize(r.suff_bin_size); r.count_bin.resize(r.entries);
		ok = fread(r.hash2index.data(), 4, r.map_size, f) == (size_t)r.map_size &&
		     fread(r.pre_buffer.data(), 4, r.pre_buffer_size, f) == (size_t)r.pre_buffer_size &&
		     fread(r.suffix_bin.data(), 1, r.suff_bin_size, f) == r.suff_bin_size &&
		     fread(r.count_bin.data(), 4, r.entries, f) == r.entries;
	}
	fclose(f);
	if (ok) {   // the device lookup indexes with these: a corrupt file must end as KMX_E_IO, not as an out-of-bounds read
		ok = r.pre_buffer[0] == 0 && (u64)r.pre_buffer[r.pre_buffer_size - 1] == r.entries && r.pre_buffer_size - 1 <= r.map_size;
		for (int g = 1; g < r.pre_buffer_size && ok; g++) ok = r.pre_buffer[g] >= r.pre_buffer[g - 1];
		int next_group = 0;                                         // groups are numbered in ascending prefix order (rest.hpp:113-127)
		for (int q = 0; q < r.map_size && ok; q++)
			if (r.hash2index[q] != -1) ok = r.hash2index[q] == next_group++;
		ok = ok && next_group == r.pre_buffer_size - 1;
		for (u64 e = 0; e < r.entries && ok; e++) ok = r.count_bin[e] >= ci && r.count_bin[e] <= cs;
	}
	if (!ok) return bail(fail(KMX_E_IO, "malformed %s/rest.bin", dir));
	m->k = r.k; m->W = (r.k + 31) / 32;
	// km.bin is mapped and copied to the device section by section, without a staging read
	const int fd = open((d + "/km.bin").c_str(), O_RDONLY);
	if (fd < 0) return bail(fail(KMX_E_IO, "cannot open %s/km.bin", dir));
	struct stat sb;
	const unsigned char *map = nullptr;
	if (fstat(fd, &sb) == 0 && sb.st_size >= 16) map = (const unsigned char *)mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
	close(fd);
	if (!map || map == (const unsigned char *)MAP_FAILED) return bail(fail(KMX_E_IO, "malformed %s/km.bin", dir));
	const u64 fsize = (u64)sb.st_size;
	auto unmap = [&] { munmap((void *)map, (size_t)fsize); };
	u64 off = 0;
	memcpy(&m->n_km, map, 8); off = 8;
	u64 nbf = 0;
	ok = fsize >= 8 * (1 + (u64)m->bf_num);
	for (int i = 0; i < m->bf_num && ok; i++) { memcpy(&m->n_bf[i], map + off, 8); off += 8; nbf += m->n_bf[i]; }
	if (!ok) { unmap(); return bail(fail(KMX_E_IO, "malformed %s/km.bin", dir)); }
	m->n_total = m->n_km + nbf;
	compute_sizes(m);
	{
		u64 need = off + m->byte_km_back + 2 * m->km_byte_size * (u64)m->nb;
		for (int i = 0; i < m->bf_num; i++) need += m->byte_bf[i] + m->byte_bf_back[i];
		if (fsize < need) { unmap(); return bail(fail(KMX_E_IO, "short or unreadable %s/km.bin", dir)); }
	}
	int rc = alloc_arrays(m);
	if (rc) { unmap(); return bail(rc); }
	auto upload = [&](void *dst, u64 nbytes) -> bool {
		const bool good = !nbytes || hipMemcpyAsync(dst, map + off, nbytes, hipMemcpyHostToDevice, m->stream) == hipSuccess;
		off += nbytes;
		return good;
	};
	for (int i = 0; i < m->bf_num && ok; i++) ok = upload(m->d_bf[i], m->byte_bf[i]) && upload(m->d_bf_back[i], m->byte_bf_back[i]);
	ok = ok && upload(m->d_km_back, m->byte_km_back);
	if (ok && m->km_byte_size) {
		DevBuf<unsigned char> dv, dt;
		ok = dv.alloc(m->ncells * 2) == hipSuccess && dt.alloc(m->ncells * 2) == hipSuccess;
		for (int a = 0; a < m->nb && ok; a++) {
			ok = upload(dv, m->km_byte_size) && upload(dt, m->km_byte_size);
			if (ok) kmxk::cells_from_disk(dv, dt, m->km_byte_size, m->d_cells[a], m->ncells, m->stream);
		}
		ok = ok && hipStreamSynchronize(m->stream) == hipSuccess;
	}
	ok = ok && hipStreamSynchronize(m->stream) == hipSuccess;
	unmap();
	if (!ok) return bail(fail(KMX_E_IO, "short or unreadable %s/km.bin", dir));
	rc = rest_to_device(m);
	if (rc) return bail(rc);
	fill_model_dev(m);
	m->state = ST_READY;
	*out = m;
	return KMX_OK;
}

static int kmx_get_stats_impl(kmx_model *m, kmx_stats *st)
{
	if (!m || !st) return fail(KMX_E_ARG, "null argument");
	std::lock_guard<std::mutex> lk(m->query_mu);                  // h_stats[ST_QUERY_*] are written by queries
	memset(st, 0, sizeof *st);
	st->n_total = m->n_total; st->n_km = m->n_km;
	for (int i = 0; i < 3; i++) { st->n_bf[i] = m->n_bf[i]; st->byte_bf[i] = m->byte_bf[i]; st->byte_bf_back[i] = m->byte_bf_back[i]; }
	st->attempts = m->h_stats[ST_ATTEMPTS]; st->successes = m->h_stats[ST_SUCCESSES];
	st->fast_commits = m->h_stats[ST_SUCCESSES] - m->h_stats[ST_SLOW_SUCC]; st->contended = m->h_stats[ST_CONTENDED]; st->finisher_iters = m->h_stats[ST_FIN_ITERS];
	st->rest_entries = m->rest.entries; st->km_byte_size = m->km_byte_size; st->byte_km_back = m->byte_km_back;
	st->blocks = m->blocks; st->rounds = m->rounds;
	st->piped_attempts = m->h_stats[ST_PIPE_ATTEMPTS]; st->piped_commits = m->h_stats[ST_PIPE_SUCC];
	st->piped_gathers = m->h_stats[ST_PIPE_GATHERS]; st->piped_atomics = m->h_stats[ST_PIPE_ATOMICS];
	st->query_neighbour_calls = m->h_stats[ST_QUERY_NEIGH]; st->query_accounted = m->h_stats[ST_QUERY_N];
	st->rest_bytes = m->rest.suff_bin_size + 4 * m->rest.entries + 4 * (u64)m->rest.pre_buffer_size + 4 * (u64)m->rest.map_size;
	st->k = m->k; st->ci = m->ci; st->cs = m->cs; st->nh = m->nh; st->nb = m->nb; st->bf_num = m->bf_num; st->device = m->device;
	return KMX_OK;
}

// the first `size` bytes of the struct: a caller built against an older (shorter) kmx_stats names its own sizeof
static int kmx_get_stats_n_impl(kmx_model *m, void *st, uint64_t size)
{
	if (!st) return fail(KMX_E_ARG, "null argument");
	kmx_stats full;
	TRY(kmx_get_stats_impl(m, &full));
	memcpy(st, &full, (size_t)std::min<uint64_t>(size, sizeof full));
	return KMX_OK;
}

static int kmx_last_build_seconds_impl(kmx_model *m, double *insert_kernels_s, double *total_s)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (insert_kernels_s) *insert_kernels_s = m->t_insert_kernels;
	if (total_s) *total_s = m->t_total;
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ KAT surface / microbench
static int kmx_debug_hash_impl(int k, const uint64_t *kmers, uint64_t n, const uint32_t *seeds, int n_seeds, int whole, uint64_t *hashes)
{
	if (k < 3 || k > 64 || n_seeds < 1) return fail(KMX_E_ARG, "bad arguments");
	const int W = (k + 31) / 32;
	DevBuf<u64> dk, dh;
	DevBuf<u32> ds;
	HIPCHK(dk.alloc(n * W + 1));
	HIPCHK(dh.alloc(n * n_seeds + 1));
	HIPCHK(ds.alloc(n_seeds));
	HIPCHK(hipMemcpy(dk, kmers, n * W * 8, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(ds, seeds, n_seeds * 4, hipMemcpyHostToDevice));
	kmxk::debug_hash(k, dk, n, ds, n_seeds, whole, dh, nullptr);
	HIPCHK(hipMemcpy(hashes, dh, n * n_seeds * 8, hipMemcpyDeviceToHost));
	return KMX_OK;
}

static int kmx_debug_min_kmer_impl(int k, const uint64_t *kmers, uint64_t n, uint64_t *out)
{
	if (k < 3 || k > 64) return fail(KMX_E_ARG, "bad arguments");
	const int W = (k + 31) / 32;
	DevBuf<u64> dk, dout;
	HIPCHK(dk.alloc(n * W + 1));
	HIPCHK(dout.alloc(n * W + 1));
	HIPCHK(hipMemcpy(dk, kmers, n * W * 8, hipMemcpyHostToDevice));
	kmxk::debug_min_kmer(k, dk, n, dout, nullptr);
	HIPCHK(hipMemcpy(out, dout, n * W * 8, hipMemcpyDeviceToHost));
	return KMX_OK;
}

static int kmx_debug_mod_impl(const uint64_t *h, uint64_t n, uint64_t d, uint64_t *out)
{
	if (!d || !n) return fail(KMX_E_ARG, "bad arguments");
	DevBuf<u64> dh, dout;
	HIPCHK(dh.alloc(n));
	HIPCHK(dout.alloc(n));
	HIPCHK(hipMemcpy(dh, h, n * 8, hipMemcpyHostToDevice));
	kmxk::debug_mod(dh, n, d, dout, nullptr);
	HIPCHK(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
	return KMX_OK;
}

// mode 20: the 4-byte gathers (mode 8) on one stream and the 32-bit atomic ORs (mode 5) on another, side by side, each on
// its own buffer; seconds = wall time until both are done.  Compared with the sum of the two alone it says whether the
// gather-bound and the atomic-bound kernels of a round could hide behind each other.
static int microbench_pair(uint64_t bytes, uint64_t touches, int iters, double *seconds)
{
	DevBuf<u64> b0, b1, sinkm;
	const u64 ncell = bytes / 8, lanes = touches / 8;
	HIPCHK(b0.alloc(ncell));
	HIPCHK(b1.alloc(ncell));
	HIPCHK(sinkm.alloc(1));
	HIPCHK(hipMemset(b0, 0, ncell * 8));
	HIPCHK(hipMemset(b1, 0, ncell * 8));
	Stream s0, s1;
	Event e0, e1, j;
	HIPCHK(s0.ensure());
	HIPCHK(s1.ensure());
	HIPCHK(e0.ensure(hipEventDefault));
	HIPCHK(e1.ensure(hipEventDefault));
	HIPCHK(j.ensure());
	kmxk::micro(8, b0, ncell, lanes, 12345, sinkm, s0);
	kmxk::micro(5, b1, ncell, lanes, 12345, sinkm, s1);
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipEventRecord(e0, s0));
	HIPCHK(hipStreamWaitEvent(s1, e0, 0));
	for (int it = 0; it < iters; it++) {
		kmxk::micro(8, b0, ncell, lanes, 1000003ULL * (it + 1), sinkm, s0);
		kmxk::micro(5, b1, ncell, lanes, 1000003ULL * (it + 1), sinkm, s1);
	}
	HIPCHK(hipEventRecord(j, s1));
	HIPCHK(hipStreamWaitEvent(s0, j, 0));
	HIPCHK(hipEventRecord(e1, s0));
	HIPCHK(hipEventSynchronize(e1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, e0, e1));
	*seconds = ms * 1e-3 / iters;
	return KMX_OK;
}

static int kmx_microbench_impl(int mode, uint64_t bytes, uint64_t touches, int iters, double *seconds)
{
	if (bytes < 4096 || touches < 8 || iters < 1 || !seconds) return fail(KMX_E_ARG, "bad arguments");
	if (mode == 20) return microbench_pair(bytes, touches, iters, seconds);
	DevBuf<u64> bufm, sinkm;
	const u64 ncell = bytes / 8, lanes = touches / 8;
	HIPCHK(bufm.alloc(ncell));
	HIPCHK(sinkm.alloc(1));
	u64 *buf = bufm, *sink = sinkm;
	HIPCHK(hipMemset(buf, 0, ncell * 8));
	Event e0, e1;
	HIPCHK(e0.ensure(hipEventDefault));
	HIPCHK(e1.ensure(hipEventDefault));
	kmxk::micro(mode, buf, ncell, lanes, 12345, sink, nullptr);            // warm-up
	HIPCHK(hipEventRecord(e0, nullptr));
	for (int it = 0; it < iters; it++) kmxk::micro(mode, buf, ncell, lanes, 1000003ULL * (it + 1), sink, nullptr);
	HIPCHK(hipEventRecord(e1, nullptr));
	HIPCHK(hipEventSynchronize(e1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, e0, e1));
	*seconds = ms * 1e-3 / iters;
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ kernel-class timing
static int kmx_set_profile_impl(kmx_model *m, int on)
{
	if (!m) return fail(KMX_E_ARG, "null model");
	if (on < 0 || on > 2) return fail(KMX_E_ARG, "kmx_set_profile: 0 (off), 1 (timing) or 2 (accounting), got %d", on);
	std::lock_guard<std::mutex> lk(m->query_mu);                  // a running query reads prof.on / prof.count
	m->prof.on = on == 1;                                         // 1: per-class timing of the product's kernels
	m->prof.count = on == 2;                                      // 2: no timing; the fused launches run their accounting variant (kmx_stats piped_*)
	return KMX_OK;
}

static int kmx_get_kernel_times_impl(kmx_model *m, double *seconds, uint64_t *launches, int reset)
{
	if (!m || !seconds || !launches) return fail(KMX_E_ARG, "null argument");
	std::lock_guard<std::mutex> lk(m->query_mu);                  // prof_collect empties the span vector queries push to
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipStreamSynchronize(m->stream));
	prof_collect(m);
	for (int c = 0; c < KC_N; c++) { seconds[c] = m->kc_seconds[c]; launches[c] = m->kc_launches[c]; }
	if (reset) for (int c = 0; c < KC_N; c++) { m->kc_seconds[c] = 0; m->kc_launches[c] = 0; }
	return KMX_OK;
}

// ------------------------------------------------------------------------------------------ exception firewall
// Nothing may unwind through the C ABI: every entry point runs its implementation inside this guard.
// (KMX_FAIL_ALLOC, test hook: the outermost entry point of a thread -- they call each other, kmx_build_host -> kmx_begin --
// arms the countdown of hip_owned.h for its own length)
static thread_local int g_entry_depth = 0;
template <typename F> static int guarded(F f)
{
	if (g_entry_depth++ == 0) if (const char *e = hook_env("KMX_FAIL_ALLOC")) kmx_fail_alloc = atoll(e);
	auto leave = scope_exit([] { if (--g_entry_depth == 0 && kmx_fail_alloc.load(std::memory_order_relaxed)) kmx_fail_alloc = 0; });
	try { return f(); }
	catch (const std::bad_alloc &) { return fail(KMX_E_NOMEM, "out of host memory"); }
	catch (const std::exception &e) { return fail(KMX_E_ARG, "internal error: %s", e.what()); }
	catch (...) { return fail(KMX_E_ARG, "internal error"); }
}

extern "C" int kmx_device_count(void) { return guarded([&] { return kmx_device_count_impl(); }); }
extern "C" int kmx_occubin(int cs, int nh, uint32_t *bin_of_occ, uint32_t *mean_of_bin) { return guarded([&] { return kmx_occubin_impl(cs, nh, bin_of_occ, mean_of_bin); }); }
extern "C" int kmx_create(int ci, int cs, int nh, int nb, kmx_model **out) { return guarded([&] { return kmx_create_impl(ci, cs, nh, nb, out); }); }
extern "C" int kmx_destroy(kmx_model *m) { return guarded([&] { return kmx_destroy_impl(m); }); }
extern "C" int kmx_set_stream(kmx_model *m, void *s) { return guarded([&] { return kmx_set_stream_impl(m, s); }); }
extern "C" int kmx_begin(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total) { return guarded([&] { return kmx_begin_impl(m, k, n_bf, n_total); }); }
extern "C" int kmx_insert_batch_dev(kmx_model *m, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n) { return guarded([&] { return kmx_insert_batch_dev_impl(m, d_kmers, d_counts, n); }); }
extern "C" int kmx_insert_batch(kmx_model *m, const uint64_t *kmers, const uint32_t *counts, uint64_t n) { return guarded([&] { return kmx_insert_batch_impl(m, kmers, counts, n); }); }
extern "C" int kmx_finish(kmx_model *m) { return guarded([&] { return kmx_finish_impl(m); }); }
extern "C" int kmx_build_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n) { return guarded([&] { return kmx_build_dev_impl(m, k, d_kmers, d_counts, n); }); }
extern "C" int kmx_build_host(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n) { return guarded([&] { return kmx_build_host_impl(m, k, kmers, counts, n); }); }
extern "C" int kmx_build_from_kmc(kmx_model *m, const char *db_prefix) { return guarded([&] { return kmx_build_from_kmc_impl(m, db_prefix); }); }
extern "C" int kmx_count_classes_dev(kmx_model *m, const uint32_t *d_counts, uint64_t n, uint64_t n_bf[3]) { return guarded([&] { return kmx_count_classes_dev_impl(m, d_counts, n, n_bf); }); }
extern "C" int kmx_shard_begin(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total, int rank, int world) { return guarded([&] { return kmx_shard_begin_impl(m, k, n_bf, n_total, rank, world); }); }
extern "C" int kmx_shard_classify_dev(kmx_model *m, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint64_t *d_out_kmers, uint32_t *d_out_counts, uint64_t *n_out) { return guarded([&] { return kmx_shard_classify_dev_impl(m, d_kmers, d_counts, n, d_out_kmers, d_out_counts, n_out); }); }
extern "C" uint64_t kmx_ring_msg_bytes(int k) { return ring_msg_bytes(k); }
extern "C" int kmx_ring_round_dev(kmx_model *m, int t, const kmx_ring_list *lists, int n_lists) { return guarded([&] { return kmx_ring_round_dev_impl(m, t, lists, n_lists); }); }
extern "C" int kmx_ring_stale_dup_dev(kmx_model *m, int first_unused_row) { return guarded([&] { return kmx_ring_stale_dup_dev_impl(m, first_unused_row); }); }
extern "C" int kmx_shard_local(kmx_model *m, kmx_stats *partial, void **d_rest_kmers, void **d_rest_counts) { return guarded([&] { return kmx_shard_local_impl(m, partial, d_rest_kmers, d_rest_counts); }); }
extern "C" int kmx_shard_complete(kmx_model *m, const uint64_t *d_rest_kmers, const int32_t *d_rest_counts, uint64_t n_rest, const kmx_stats *totals) { return guarded([&] { return kmx_shard_complete_impl(m, d_rest_kmers, d_rest_counts, n_rest, totals); }); }
extern "C" int kmx_create_on(int device, int ci, int cs, int nh, int nb, kmx_model **out) { return guarded([&] { return kmx_create_on_impl(device, ci, cs, nh, nb, out); }); }
extern "C" int kmx_build_from_kmc_multi(kmx_model **models, int n_models, const char *db_prefix) { return guarded([&] { return kmx_build_from_kmc_multi_ex_impl(models, n_models, db_prefix, KMX_PARTITION_RING); }); }
extern "C" int kmx_build_from_kmc_multi_ex(kmx_model **models, int n_models, const char *db_prefix, int partition) { return guarded([&] { return kmx_build_from_kmc_multi_ex_impl(models, n_models, db_prefix, partition); }); }
extern "C" int kmx_range_begin(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total, int rank, int world) { return guarded([&] { return kmx_range_begin_impl(m, k, n_bf, n_total, rank, world); }); }
extern "C" int kmx_range_buffers(kmx_model *m, void **d_send, uint64_t *cap_words, uint64_t *cell_lo) { return guarded([&] { return kmx_range_buffers_impl(m, d_send, cap_words, cell_lo); }); }
extern "C" int kmx_range_emit_dev(kmx_model *m, int t, const kmx_ring_list *lists, int n_lists, uint64_t *counts) { return guarded([&] { return kmx_range_emit_dev_impl(m, t, lists, n_lists, counts); }); }
extern "C" int kmx_range_verdict_dev(kmx_model *m, int t, const uint64_t *d_words, const uint64_t *totals, const uint64_t *commits, int n_src, uint8_t *d_verdict) { return guarded([&] { return kmx_range_verdict_dev_impl(m, t, d_words, totals, commits, n_src, d_verdict); }); }
extern "C" int kmx_range_resolve_dev(kmx_model *m, int t, const uint8_t *d_verdict) { return guarded([&] { return kmx_range_resolve_dev_impl(m, t, d_verdict); }); }
extern "C" int kmx_range_inband(kmx_model *m, void **d_send, uint64_t *region_words, uint64_t *capx_words) { return guarded([&] { return kmx_range_inband_impl(m, d_send, region_words, capx_words); }); }
extern "C" int kmx_range_verdict_inband_dev(kmx_model *m, int t, const uint64_t *d_recv, int n_src, uint8_t *d_verdict) { return guarded([&] { return kmx_range_verdict_inband_dev_impl(m, t, d_recv, n_src, d_verdict); }); }
extern "C" int kmx_range_commit_inband_dev(kmx_model *m, const uint64_t *d_recv, int n_src) { return guarded([&] { return kmx_range_commit_inband_dev_impl(m, d_recv, n_src); }); }
extern "C" int kmx_range_commit_dev(kmx_model *m, const uint64_t *d_commits, uint64_t n) { return guarded([&] { return kmx_range_commit_dev_impl(m, d_commits, n); }); }
extern "C" int kmx_range_flush_dev(kmx_model *m, uint64_t *counts) { return guarded([&] { return kmx_range_flush_dev_impl(m, counts); }); }
extern "C" int kmx_dev_view(kmx_model *m, int which, int index, void **ptr, uint64_t *bytes) { return guarded([&] { return kmx_dev_view_impl(m, which, index, ptr, bytes); }); }
extern "C" int kmx_or_words_dev(kmx_model *m, void *d_dst, const void *d_src, uint64_t n_words) { return guarded([&] { return kmx_or_words_dev_impl(m, d_dst, d_src, n_words); }); }
extern "C" int kmx_kmc_info(const char *db_prefix, int *k, uint64_t *total_kmers) { return guarded([&] { return kmx_kmc_info_impl(db_prefix, k, total_kmers); }); }
extern "C" int kmx_kmc_read(const char *db_prefix, uint64_t *kmers, uint32_t *counts, uint64_t capacity, uint64_t *n_read) { return guarded([&] { return kmx_kmc_read_impl(db_prefix, kmers, counts, capacity, n_read); }); }
extern "C" int kmx_query_packed_dev(kmx_model *m, const uint64_t *d_kmers, uint64_t n, int32_t *d_out) { return guarded([&] { return kmx_query_packed_dev_impl(m, d_kmers, n, d_out); }); }
extern "C" int kmx_query_packed(kmx_model *m, const uint64_t *kmers, uint64_t n, int32_t *out) { return guarded([&] { return kmx_query_packed_impl(m, kmers, n, out); }); }
extern "C" int kmx_query_ascii(kmx_model *m, const char *strs, int len, int stride, uint64_t n, int32_t *out) { return guarded([&] { return kmx_query_ascii_impl(m, strs, len, stride, n, out); }); }
extern "C" int kmx_query_strings(kmx_model *m, const char *const *strs, int len, uint64_t n, int32_t *out) { return guarded([&] { return kmx_query_strings_impl(m, strs, len, n, out); }); }
extern "C" int kmx_query_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t *out) { return guarded([&] { return kmx_query_seqs_impl(m, seq, offsets, n_seqs, out); }); }
extern "C" int kmx_query_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t *d_out) { return guarded([&] { return kmx_query_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, d_out); }); }
extern "C" int kmx_count_begin(kmx_model *m, int k) { return guarded([&] { return kmx_count_begin_impl(m, k); }); }
extern "C" int kmx_summarise_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, const int32_t *thr, int n_thr, kmx_seq_summary *out) { return guarded([&] { return kmx_summarise_seqs_impl(m, seq, offsets, n_seqs, thr, n_thr, out); }); }
extern "C" int kmx_summarise_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, const int32_t *thr, int n_thr, kmx_seq_summary *d_out) { return guarded([&] { return kmx_summarise_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, thr, n_thr, d_out); }); }
extern "C" int kmx_correct_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, char *seq_out, kmx_seq_correction *rec) { return guarded([&] { return kmx_correct_seqs_impl(m, seq, offsets, n_seqs, thr, min_support, seq_out, rec); }); }
extern "C" int kmx_correct_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, char *d_seq_out, kmx_seq_correction *d_rec) { return guarded([&] { return kmx_correct_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, thr, min_support, d_seq_out, d_rec); }); }
extern "C" int kmx_edit_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, int ops, kmx_edit *edits, uint64_t capacity, uint64_t *n_edits, kmx_seq_edits *rec) { return guarded([&] { return kmx_edit_seqs_impl(m, seq, offsets, n_seqs, thr, min_support, ops, edits, capacity, n_edits, rec); }); }
extern "C" int kmx_edit_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, int ops, kmx_edit *d_edits, uint64_t capacity, uint64_t *n_edits, kmx_seq_edits *d_rec) { return guarded([&] { return kmx_edit_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, thr, min_support, ops, d_edits, capacity, n_edits, d_rec); }); }
extern "C" int kmx_apply_edits(const char *seq, const uint64_t *offsets, uint64_t n_seqs, const kmx_edit *edits, uint64_t n_edits, char *seq_out, uint64_t out_capacity, uint64_t *offsets_out) { return guarded([&] { return kmx_apply_edits_impl(seq, offsets, n_seqs, edits, n_edits, seq_out, out_capacity, offsets_out); }); }
extern "C" int kmx_apply_edits_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, const kmx_edit *d_edits, uint64_t n_edits, char *d_seq_out, uint64_t out_capacity, uint64_t *d_offsets_out) { return guarded([&] { return kmx_apply_edits_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, d_edits, n_edits, d_seq_out, out_capacity, d_offsets_out); }); }
extern "C" int kmx_polish_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, int ops, int max_passes, char *seq_out, uint64_t out_capacity, uint64_t *offsets_out, kmx_seq_polish *rec, uint64_t *passes_run) { return guarded([&] { return kmx_polish_seqs_impl(m, seq, offsets, n_seqs, thr, min_support, ops, max_passes, seq_out, out_capacity, offsets_out, rec, passes_run); }); }
extern "C" int kmx_polish_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, int ops, int max_passes, char *d_seq_out, uint64_t out_capacity, uint64_t *d_offsets_out, kmx_seq_polish *d_rec, uint64_t *passes_run) { return guarded([&] { return kmx_polish_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, thr, min_support, ops, max_passes, d_seq_out, out_capacity, d_offsets_out, d_rec, passes_run); }); }
extern "C" int kmx_extend_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int max_ext, int depth, char *ext, kmx_seq_extension *rec) { return guarded([&] { return kmx_extend_seqs_impl(m, seq, offsets, n_seqs, thr, max_ext, depth, ext, rec); }); }
extern "C" int kmx_extend_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int max_ext, int depth, char *d_ext, kmx_seq_extension *d_rec) { return guarded([&] { return kmx_extend_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, thr, max_ext, depth, d_ext, d_rec); }); }
extern "C" int kmx_count_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs) { return guarded([&] { return kmx_count_seqs_impl(m, seq, offsets, n_seqs); }); }
extern "C" int kmx_count_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases) { return guarded([&] { return kmx_count_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases); }); }
extern "C" int kmx_count_finish(kmx_model *m, uint64_t *n_listed) { return guarded([&] { return kmx_count_finish_impl(m, n_listed); }); }
extern "C" int kmx_count_listing(kmx_model *m, uint64_t *kmers, uint32_t *counts, uint64_t capacity, uint64_t *n) { return guarded([&] { return kmx_count_listing_impl(m, kmers, counts, capacity, n); }); }
extern "C" int kmx_unitigs_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out) { return guarded([&] { return kmx_unitigs_dev_impl(m, k, d_kmers, d_counts, n, thr, d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, n_unitigs, n_bases_out); }); }
extern "C" int kmx_unitigs(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out) { return guarded([&] { return kmx_unitigs_impl(m, k, kmers, counts, n, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, n_unitigs, n_bases_out); }); }
extern "C" int kmx_count_unitigs(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out) { return guarded([&] { return kmx_count_unitigs_impl(m, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, n_unitigs, n_bases_out); }); }
extern "C" int kmx_count_unitigs_dev(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out) { return guarded([&] { return kmx_count_unitigs_dev_impl(m, thr, d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, n_unitigs, n_bases_out); }); }
extern "C" int kmx_unitigs_last_phases(kmx_model *m, double *seconds, uint64_t *rounds) { return guarded([&] { return kmx_unitigs_last_phases_impl(m, seconds, rounds); }); }
extern "C" int kmx_unitig_graph_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links) { return guarded([&] { return kmx_unitig_graph_dev_impl(m, k, d_kmers, d_counts, n, thr, d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity, n_unitigs, n_bases_out, n_links); }); }
extern "C" int kmx_unitig_graph(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links) { return guarded([&] { return kmx_unitig_graph_impl(m, k, kmers, counts, n, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out, n_links); }); }
extern "C" int kmx_count_unitig_graph(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links) { return guarded([&] { return kmx_count_unitig_graph_impl(m, thr, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out, n_links); }); }
extern "C" int kmx_count_unitig_graph_dev(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links) { return guarded([&] { return kmx_count_unitig_graph_dev_impl(m, thr, d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity, n_unitigs, n_bases_out, n_links); }); }
extern "C" int kmx_unitig_graph_last_phases(kmx_model *m, double *seconds, uint64_t *rounds) { return guarded([&] { return kmx_unitig_graph_last_phases_impl(m, seconds, rounds); }); }
extern "C" int kmx_unitig_graph_clean_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, const kmx_clean_params *params, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *d_removed, kmx_clean_stats *stats) { return guarded([&] { return kmx_unitig_graph_clean_dev_impl(m, k, d_kmers, d_counts, n, thr, params, d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity, n_unitigs, n_bases_out, n_links, d_removed, stats); }); }
extern "C" int kmx_unitig_graph_clean(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, const kmx_clean_params *params, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *removed, kmx_clean_stats *stats) { return guarded([&] { return kmx_unitig_graph_clean_impl(m, k, kmers, counts, n, thr, params, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out, n_links, removed, stats); }); }
extern "C" int kmx_count_unitig_graph_clean(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity, uint64_t *link_offsets, uint32_t *links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *removed, kmx_clean_stats *stats) { return guarded([&] { return kmx_count_unitig_graph_clean_impl(m, thr, params, seq_out, seq_capacity, offsets_out, rec, rec_capacity, link_offsets, links, link_capacity, n_unitigs, n_bases_out, n_links, removed, stats); }); }
extern "C" int kmx_count_unitig_graph_clean_dev(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets, uint32_t *d_links, uint64_t link_capacity, uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *d_removed, kmx_clean_stats *stats) { return guarded([&] { return kmx_count_unitig_graph_clean_dev_impl(m, thr, params, d_seq_out, seq_capacity, d_offsets_out, d_rec, rec_capacity, d_link_offsets, d_links, link_capacity, n_unitigs, n_bases_out, n_links, d_removed, stats); }); }
extern "C" int kmx_unitig_clean_last_phases(kmx_model *m, double *seconds, uint64_t *rounds) { return guarded([&] { return kmx_unitig_clean_last_phases_impl(m, seconds, rounds); }); }
extern "C" int kmx_unitig_map_begin_dev(kmx_model *m, int k, const uint64_t *d_kmers, uint64_t n, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases) { return guarded([&] { return kmx_unitig_map_begin_dev_impl(m, k, d_kmers, n, d_useq, d_uoffsets, n_unitigs, n_ubases); }); }
extern "C" int kmx_unitig_map_begin(kmx_model *m, int k, const uint64_t *kmers, uint64_t n, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs) { return guarded([&] { return kmx_unitig_map_begin_impl(m, k, kmers, n, useq, uoffsets, n_unitigs); }); }
extern "C" int kmx_count_unitig_map_begin_dev(kmx_model *m, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases) { return guarded([&] { return kmx_count_unitig_map_begin_dev_impl(m, d_useq, d_uoffsets, n_unitigs, n_ubases); }); }
extern "C" int kmx_count_unitig_map_begin(kmx_model *m, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs) { return guarded([&] { return kmx_count_unitig_map_begin_impl(m, useq, uoffsets, n_unitigs); }); }
extern "C" int kmx_unitig_map_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, kmx_map_segment *d_segs, uint64_t capacity, uint64_t *n_segs, uint64_t *d_seg_offsets, kmx_seq_map *d_rec, uint64_t *d_hits) { return guarded([&] { return kmx_unitig_map_seqs_dev_impl(m, d_seq, d_offsets, n_seqs, n_bases, d_segs, capacity, n_segs, d_seg_offsets, d_rec, d_hits); }); }
extern "C" int kmx_unitig_map_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, kmx_map_segment *segs, uint64_t capacity, uint64_t *n_segs, uint64_t *seg_offsets, kmx_seq_map *rec, uint64_t *hits) { return guarded([&] { return kmx_unitig_map_seqs_impl(m, seq, offsets, n_seqs, segs, capacity, n_segs, seg_offsets, rec, hits); }); }
extern "C" int kmx_unitig_map_end(kmx_model *m) { return guarded([&] { return kmx_unitig_map_end_impl(m); }); }
extern "C" int kmx_unitig_walk_segs(kmx_model *m, const kmx_map_segment *segs, uint64_t n_segs, const uint64_t *seg_offsets, uint64_t n_seqs, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links, const kmx_walk_params *params, kmx_walk *walks, uint64_t walk_capacity, uint64_t *walk_offsets, uint32_t *steps, uint64_t step_capacity, uint64_t *link_hits, kmx_walk_stats *stats) { return guarded([&] { return kmx_unitig_walk_segs_impl(m, WalkArgs{segs, n_segs, seg_offsets, n_seqs, link_offsets, links, n_links, params, walks, walk_capacity, walk_offsets, steps, step_capacity, link_hits, stats}); }); }
extern "C" int kmx_unitig_walk_segs_dev(kmx_model *m, const kmx_map_segment *d_segs, uint64_t n_segs, const uint64_t *d_seg_offsets, uint64_t n_seqs, const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, const kmx_walk_params *params, kmx_walk *d_walks, uint64_t walk_capacity, uint64_t *d_walk_offsets, uint32_t *d_steps, uint64_t step_capacity, uint64_t *d_link_hits, kmx_walk_stats *stats) { return guarded([&] { return kmx_unitig_walk_segs_dev_impl(m, WalkArgs{d_segs, n_segs, d_seg_offsets, n_seqs, d_link_offsets, d_links, n_links, params, d_walks, walk_capacity, d_walk_offsets, d_steps, step_capacity, d_link_hits, stats}); }); }
extern "C" int kmx_unitig_contigs(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs, const kmx_unitig *urec, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links, const uint64_t *link_hits, const kmx_contig_params *params, char *cseq, uint64_t *coffsets, kmx_contig *crec, uint32_t *steps, kmx_contig_place *place, uint64_t *clink_offsets, uint32_t *clinks, uint64_t *csupport, uint64_t *n_contigs, uint64_t *n_cbases, uint64_t *n_clinks, kmx_contig_stats *stats) { return guarded([&] { return kmx_unitig_contigs_impl(m, CtgArgs{k, useq, uoffsets, n_unitigs, 0, urec, link_offsets, links, n_links, link_hits, params, cseq, coffsets, crec, steps, place, clink_offsets, clinks, csupport, n_contigs, n_cbases, n_clinks, stats}); }); }
extern "C" int kmx_unitig_contigs_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_unitig *d_urec, const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, const uint64_t *d_link_hits, const kmx_contig_params *params, char *d_cseq, uint64_t *d_coffsets, kmx_contig *d_crec, uint32_t *d_steps, kmx_contig_place *d_place, uint64_t *d_clink_offsets, uint32_t *d_clinks, uint64_t *d_csupport, uint64_t *n_contigs, uint64_t *n_cbases, uint64_t *n_clinks, kmx_contig_stats *stats) { return guarded([&] { return kmx_unitig_contigs_dev_impl(m, CtgArgs{k, d_useq, d_uoffsets, n_unitigs, n_ubases, d_urec, d_link_offsets, d_links, n_links, d_link_hits, params, d_cseq, d_coffsets, d_crec, d_steps, d_place, d_clink_offsets, d_clinks, d_csupport, n_contigs, n_cbases, n_clinks, stats}); }); }
extern "C" int kmx_unitig_contigs_last_phases(kmx_model *m, double *seconds, uint64_t *rounds) { return guarded([&] { return kmx_unitig_contigs_last_phases_impl(m, seconds, rounds); }); }
extern "C" int kmx_unitig_walk_through(kmx_model *m, const kmx_walk *walks, uint64_t n_walks, const uint32_t *steps, uint64_t n_steps, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links, uint64_t n_unitigs, uint64_t *through, kmx_through_stats *stats) { return guarded([&] { return kmx_unitig_walk_through_impl(m, ThroughArgs{walks, n_walks, steps, n_steps, link_offsets, links, n_links, n_unitigs, through, stats}); }); }
extern "C" int kmx_unitig_walk_through_dev(kmx_model *m, const kmx_walk *d_walks, uint64_t n_walks, const uint32_t *d_steps, uint64_t n_steps, const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, uint64_t n_unitigs, uint64_t *d_through, kmx_through_stats *stats) { return guarded([&] { return kmx_unitig_walk_through_dev_impl(m, ThroughArgs{d_walks, n_walks, d_steps, n_steps, d_link_offsets, d_links, n_links, n_unitigs, d_through, stats}); }); }
extern "C" int kmx_unitig_pair_walks(kmx_model *m, const kmx_walk *walks, uint64_t n_walks, const uint64_t *walk_offsets, uint64_t n_seqs, const uint32_t *steps, uint64_t n_steps, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links, const kmx_pair_params *params, kmx_pair *pairs, uint64_t *hist, uint64_t *pair_hits, kmx_pair_link *plinks, uint64_t capacity, uint64_t *n_plinks, kmx_pair_stats *stats) { return guarded([&] { return kmx_unitig_pair_walks_impl(m, PairArgs{walks, n_walks, walk_offsets, n_seqs, steps, n_steps, link_offsets, links, n_links, params, pairs, hist, pair_hits, plinks, capacity, n_plinks, stats}); }); }
extern "C" int kmx_unitig_pair_walks_dev(kmx_model *m, const kmx_walk *d_walks, uint64_t n_walks, const uint64_t *d_walk_offsets, uint64_t n_seqs, const uint32_t *d_steps, uint64_t n_steps, const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, const kmx_pair_params *params, kmx_pair *d_pairs, uint64_t *d_hist, uint64_t *d_pair_hits, kmx_pair_link *d_plinks, uint64_t capacity, uint64_t *n_plinks, kmx_pair_stats *stats) { return guarded([&] { return kmx_unitig_pair_walks_dev_impl(m, PairArgs{d_walks, n_walks, d_walk_offsets, n_seqs, d_steps, n_steps, d_link_offsets, d_links, n_links, params, d_pairs, d_hist, d_pair_hits, d_plinks, capacity, n_plinks, stats}); }); }
extern "C" int kmx_unitig_scaffold(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs, const kmx_unitig *urec, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_scaffold_params *params, char *sseq, uint64_t seq_capacity, uint64_t *soffsets, kmx_scaffold *srec, kmx_scaffold_step *steps, kmx_scaffold_place *place, uint64_t *n_scaffolds, uint64_t *n_sbases, kmx_scaffold_stats *stats) { return guarded([&] { return kmx_unitig_scaffold_impl(m, ScfArgs{k, useq, uoffsets, n_unitigs, 0, urec, plinks, n_plinks, params, sseq, seq_capacity, soffsets, srec, steps, place, n_scaffolds, n_sbases, stats}); }); }
extern "C" int kmx_unitig_scaffold_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_unitig *d_urec, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_scaffold_params *params, char *d_sseq, uint64_t seq_capacity, uint64_t *d_soffsets, kmx_scaffold *d_srec, kmx_scaffold_step *d_steps, kmx_scaffold_place *d_place, uint64_t *n_scaffolds, uint64_t *n_sbases, kmx_scaffold_stats *stats) { return guarded([&] { return kmx_unitig_scaffold_dev_impl(m, ScfArgs{k, d_useq, d_uoffsets, n_unitigs, n_ubases, d_urec, d_plinks, n_plinks, params, d_sseq, seq_capacity, d_soffsets, d_srec, d_steps, d_place, n_scaffolds, n_sbases, stats}); }); }
extern "C" int kmx_unitig_scaffold_last_phases(kmx_model *m, double *seconds, uint64_t *rounds) { return guarded([&] { return kmx_unitig_scaffold_last_phases_impl(m, seconds, rounds); }); }
extern "C" int kmx_unitig_pair_paths(kmx_model *m, int k, const uint64_t *uoffsets, uint64_t n_unitigs, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_path_params *params, kmx_pair_path *precs, uint32_t *psteps, uint64_t capacity, uint64_t *n_psteps, uint64_t *through, uint64_t *path_hits, kmx_pair_path_stats *stats) { return guarded([&] { return kmx_unitig_pair_paths_impl(m, PathArgs{k, uoffsets, n_unitigs, link_offsets, links, n_links, plinks, n_plinks, params, precs, psteps, capacity, n_psteps, through, path_hits, stats}); }); }
extern "C" int kmx_unitig_pair_paths_dev(kmx_model *m, int k, const uint64_t *d_uoffsets, uint64_t n_unitigs, const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_pair_path_params *params, kmx_pair_path *d_precs, uint32_t *d_psteps, uint64_t capacity, uint64_t *n_psteps, uint64_t *d_through, uint64_t *d_path_hits, kmx_pair_path_stats *stats) { return guarded([&] { return kmx_unitig_pair_paths_dev_impl(m, PathArgs{k, d_uoffsets, n_unitigs, d_link_offsets, d_links, n_links, d_plinks, n_plinks, params, d_precs, d_psteps, capacity, n_psteps, d_through, d_path_hits, stats}); }); }
extern "C" int kmx_unitig_pair_paths_last_phases(kmx_model *m, double *seconds) { return guarded([&] { return kmx_unitig_pair_paths_last_phases_impl(m, seconds); }); }
extern "C" int kmx_unitig_scaffold_fill(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs, const kmx_scaffold *srec, uint64_t n_scaffolds, const kmx_scaffold_step *steps, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_path *precs, const uint32_t *psteps, uint64_t n_psteps, const kmx_fill_params *params, char *fseq, uint64_t seq_capacity, uint64_t *foffsets, kmx_scaffold_fill *frec, kmx_fill_step *fsteps, uint32_t *pieces, uint64_t piece_capacity, uint64_t *n_fbases, uint64_t *n_pieces, kmx_fill_stats *stats) { return guarded([&] { return kmx_unitig_scaffold_fill_impl(m, FillArgs{k, useq, uoffsets, n_unitigs, 0, srec, n_scaffolds, steps, plinks, n_plinks, precs, psteps, n_psteps, params, fseq, seq_capacity, foffsets, frec, fsteps, pieces, piece_capacity, n_fbases, n_pieces, stats}); }); }
extern "C" int kmx_unitig_scaffold_fill_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_scaffold *d_srec, uint64_t n_scaffolds, const kmx_scaffold_step *d_steps, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_pair_path *d_precs, const uint32_t *d_psteps, uint64_t n_psteps, const kmx_fill_params *params, char *d_fseq, uint64_t seq_capacity, uint64_t *d_foffsets, kmx_scaffold_fill *d_frec, kmx_fill_step *d_fsteps, uint32_t *d_pieces, uint64_t piece_capacity, uint64_t *n_fbases, uint64_t *n_pieces, kmx_fill_stats *stats) { return guarded([&] { return kmx_unitig_scaffold_fill_dev_impl(m, FillArgs{k, d_useq, d_uoffsets, n_unitigs, n_ubases, d_srec, n_scaffolds, d_steps, d_plinks, n_plinks, d_precs, d_psteps, n_psteps, params, d_fseq, seq_capacity, d_foffsets, d_frec, d_fsteps, d_pieces, piece_capacity, n_fbases, n_pieces, stats}); }); }
extern "C" int kmx_unitig_scaffold_fill_last_phases(kmx_model *m, double *seconds) { return guarded([&] { return kmx_unitig_scaffold_fill_last_phases_impl(m, seconds); }); }
extern "C" int kmx_unitig_pair_reduce(kmx_model *m, int k, const uint64_t *uoffsets, uint64_t n_unitigs, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_reduce_params *params, kmx_pair_reduce *rrecs, kmx_pair_link *lout, uint32_t *origin, uint64_t capacity, uint64_t *n_out, kmx_pair_reduce_stats *stats) { return guarded([&] { return kmx_unitig_pair_reduce_impl(m, RedArgs{k, uoffsets, n_unitigs, 0, plinks, n_plinks, params, rrecs, lout, origin, capacity, n_out, stats}); }); }
extern "C" int kmx_unitig_pair_reduce_dev(kmx_model *m, int k, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_pair_reduce_params *params, kmx_pair_reduce *d_rrecs, kmx_pair_link *d_lout, uint32_t *d_origin, uint64_t capacity, uint64_t *n_out, kmx_pair_reduce_stats *stats) { return guarded([&] { return kmx_unitig_pair_reduce_dev_impl(m, RedArgs{k, d_uoffsets, n_unitigs, n_ubases, d_plinks, n_plinks, params, d_rrecs, d_lout, d_origin, capacity, n_out, stats}); }); }
extern "C" int kmx_unitig_pair_reduce_last_phases(kmx_model *m, double *seconds) { return guarded([&] { return kmx_unitig_pair_reduce_last_phases_impl(m, seconds); }); }
extern "C" int kmx_unitig_pair_lift(kmx_model *m, int k, const uint64_t *uoffsets, uint64_t n_unitigs, const kmx_contig_place *place, const kmx_contig *crec, uint64_t n_contigs, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_lift_params *params, kmx_pair_lift *lrec, kmx_pair_link *lout, uint64_t capacity, uint64_t *n_out, kmx_pair_lift_stats *stats) { return guarded([&] { return kmx_unitig_pair_lift_impl(m, LiftArgs{k, uoffsets, n_unitigs, 0, place, crec, n_contigs, plinks, n_plinks, params, lrec, lout, capacity, n_out, stats}); }); }
extern "C" int kmx_unitig_pair_lift_dev(kmx_model *m, int k, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_contig_place *d_place, const kmx_contig *d_crec, uint64_t n_contigs, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_pair_lift_params *params, kmx_pair_lift *d_lrec, kmx_pair_link *d_lout, uint64_t capacity, uint64_t *n_out, kmx_pair_lift_stats *stats) { return guarded([&] { return kmx_unitig_pair_lift_dev_impl(m, LiftArgs{k, d_uoffsets, n_unitigs, n_ubases, d_place, d_crec, n_contigs, d_plinks, n_plinks, params, d_lrec, d_lout, capacity, n_out, stats}); }); }
extern "C" int kmx_unitig_pair_lift_fold_variant(kmx_model *m, int variant) { return guarded([&] { return kmx_unitig_pair_lift_fold_variant_impl(m, variant); }); }
extern "C" int kmx_unitig_pair_lift_last_phases(kmx_model *m, double *seconds) { return guarded([&] { return kmx_unitig_pair_lift_last_phases_impl(m, seconds); }); }
extern "C" int kmx_unitig_resolve(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs, const kmx_unitig *urec, const uint64_t *link_offsets, const uint32_t *links, uint64_t n_links, const uint64_t *link_hits, const uint64_t *through, const kmx_resolve_params *params, char *rseq, uint64_t seq_capacity, uint64_t *roffsets, uint64_t rec_capacity, kmx_unitig *rrec, uint32_t *origin, kmx_resolve_place *rplace, uint64_t *rlink_offsets, uint32_t *rlinks, uint64_t *link_origin, uint64_t *rlink_hits, uint64_t *n_unitigs_out, uint64_t *n_bases_out, kmx_resolve_stats *stats) { return guarded([&] { return kmx_unitig_resolve_impl(m, ResArgs{k, useq, uoffsets, n_unitigs, 0, urec, link_offsets, links, n_links, link_hits, through, params, rseq, seq_capacity, roffsets, rec_capacity, rrec, origin, rplace, rlink_offsets, rlinks, link_origin, rlink_hits, n_unitigs_out, n_bases_out, stats}); }); }
extern "C" int kmx_unitig_resolve_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_unitig *d_urec, const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, const uint64_t *d_link_hits, const uint64_t *d_through, const kmx_resolve_params *params, char *d_rseq, uint64_t seq_capacity, uint64_t *d_roffsets, uint64_t rec_capacity, kmx_unitig *d_rrec, uint32_t *d_origin, kmx_resolve_place *d_rplace, uint64_t *d_rlink_offsets, uint32_t *d_rlinks, uint64_t *d_link_origin, uint64_t *d_rlink_hits, uint64_t *n_unitigs_out, uint64_t *n_bases_out, kmx_resolve_stats *stats) { return guarded([&] { return kmx_unitig_resolve_dev_impl(m, ResArgs{k, d_useq, d_uoffsets, n_unitigs, n_ubases, d_urec, d_link_offsets, d_links, n_links, d_link_hits, d_through, params, d_rseq, seq_capacity, d_roffsets, rec_capacity, d_rrec, d_origin, d_rplace, d_rlink_offsets, d_rlinks, d_link_origin, d_rlink_hits, n_unitigs_out, n_bases_out, stats}); }); }
extern "C" int kmx_unitig_resolve_last_phases(kmx_model *m, double *seconds) { return guarded([&] { return kmx_unitig_resolve_last_phases_impl(m, seconds); }); }
extern "C" int kmx_build_from_reads(kmx_model *m, int k, const char *input) { return guarded([&] { return kmx_build_from_reads_impl(m, k, input); }); }
extern "C" int kmx_download(kmx_model *m, int which, int index, uint8_t *dst, uint64_t capacity, uint64_t *written) { return guarded([&] { return kmx_download_impl(m, which, index, dst, capacity, written); }); }
extern "C" int kmx_save(kmx_model *m, const char *dir) { return guarded([&] { return kmx_save_impl(m, dir); }); }
extern "C" int kmx_load(const char *dir, kmx_model **out) { return guarded([&] { return kmx_load_impl(dir, out); }); }
extern "C" int kmx_get_stats(kmx_model *m, kmx_stats *st) { return guarded([&] { return kmx_get_stats_impl(m, st); }); }
extern "C" int kmx_last_build_seconds(kmx_model *m, double *insert_kernels_s, double *total_s) { return guarded([&] { return kmx_last_build_seconds_impl(m, insert_kernels_s, total_s); }); }
extern "C" int kmx_debug_hash(int k, const uint64_t *kmers, uint64_t n, const uint32_t *seeds, int n_seeds, int whole, uint64_t *hashes) { return guarded([&] { return kmx_debug_hash_impl(k, kmers, n, seeds, n_seeds, whole, hashes); }); }
extern "C" int kmx_debug_min_kmer(int k, const uint64_t *kmers, uint64_t n, uint64_t *out) { return guarded([&] { return kmx_debug_min_kmer_impl(k, kmers, n, out); }); }
extern "C" int kmx_debug_mod(const uint64_t *h, uint64_t n, uint64_t d, uint64_t *out) { return guarded([&] { return kmx_debug_mod_impl(h, n, d, out); }); }
extern "C" int kmx_debug_pack_strings(const char *const *strs, const char *flat, int len, int stride, uint64_t n, uint64_t *packed, int *clean)
{
	return guarded([&] {
		if (len < 2 || len > 64 || (!strs && (!flat || stride < len)) || !packed || !clean) return fail(KMX_E_ARG, "bad argument");
		*clean = kmx_pack_strings(KmxStrBatch{strs, flat, strs ? len : stride, len}, (len + 31) / 32, 0, n, packed) ? 1 : 0;
		return (int)KMX_OK;
	});
}
extern "C" int kmx_kernel_classes(void) { return KMX_KERNEL_CLASSES; }
extern "C" int kmx_abi_version(void) { return KMX_ABI_VERSION; }
extern "C" int kmx_get_stats_n(kmx_model *m, void *st, uint64_t size) { return guarded([&] { return kmx_get_stats_n_impl(m, st, size); }); }
extern "C" int kmx_microbench(int mode, uint64_t bytes, uint64_t touches, int iters, double *seconds) { return guarded([&] { return kmx_microbench_impl(mode, bytes, touches, iters, seconds); }); }
extern "C" int kmx_set_profile(kmx_model *m, int on) { return guarded([&] { return kmx_set_profile_impl(m, on); }); }
static_assert(KC_N == KMX_KERNEL_CLASSES, "include/kmx.h promises KMX_KERNEL_CLASSES entries");
extern "C" int kmx_get_kernel_times(kmx_model *m, double *seconds, uint64_t *launches, int reset) { return guarded([&] { return kmx_get_kernel_times_impl(m, seconds, launches, reset); }); }
