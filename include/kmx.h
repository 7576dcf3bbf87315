/* include/kmx.h -- C ABI of libkmx.so, the MI355X-native KModel insert/query hot path.
 *
 * The reference (lzhLab/kmcEx) has no FFI layer: its boundary is the header-only C++ class KModel plus
 * two factory functions (kmodel.hpp).  This C ABI is what a binding for that class binds; every entry
 * point cites the reference interface it replaces.  include/kmodel.hpp is the C++ facade with the
 * reference's own names (get_model / init / init_KModel / kmer_to_occ / save / load) on top of it.
 *
 * Conventions
 *   - plain C types, caller-owned buffers, no exceptions cross the boundary;
 *   - every function returns 0 on success, a negative KMX_E_* code otherwise; kmx_last_error() gives
 *     a thread-local message;
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with
 *     KMX_E_NODEVICE;
 *   - packed k-mers: W = ceil(k/32) uint64 words per k-mer, word 0 most significant, holding the
 *     2k-bit integer right-aligned, A=0 C=1 G=2 T=3, first base most significant (tools.hpp:63-76);
 *   - "_dev" variants take DEVICE pointers valid on the model's device and enqueue on the model's
 *     stream (kmx_set_stream); they synchronise that stream only where a count has to reach the host;
 *   - the k of a model or of a counting session is in [4, 64]: every entry point that builds, counts or
 *     loads one refuses k = 3 with KMX_E_ARG before anything runs, and leaves the handle as it was.  The
 *     reference's rest table is undefined there (rest.hpp:78-83 gives k = 3 a prefix of 7 bases), so it
 *     cannot build that model either.  The kmx_debug_* entry points take k in [3, 64].
 */
#ifndef KMX_H
#define KMX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMX_OK            0
#define KMX_E_ARG        -1   /* bad argument / parameter combination                         */
#define KMX_E_NODEVICE   -2   /* no HIP device, or a HIP call failed                           */
#define KMX_E_IO         -3   /* file missing / short / malformed                              */
#define KMX_E_STATE      -4   /* call out of order (e.g. insert before begin, query before build) */
#define KMX_E_RANGE      -5   /* a count outside [ci, cs] (reference: out-of-bounds index)      */
#define KMX_E_NOMEM      -6

typedef struct kmx_model kmx_model;

typedef struct kmx_stats {
	uint64_t n_total;         /* k-mers listed (CKMCFile::KmerCount, kmodel.hpp:429)            */
	uint64_t n_km;            /* k-mers routed to the coupled arrays (kmodel.hpp:433)           */
	uint64_t n_bf[3];         /* k-mers per Bloom-filter class (kmodel.hpp:425-428)             */
	uint64_t attempts;        /* coupled-array insert attempts  (insert_to_array calls, :590)   */
	uint64_t successes;       /* ... that succeeded                                             */
	uint64_t rest_entries;    /* rows of rest.bin (rest.hpp:53 suffix_bin_count)                */
	uint64_t km_byte_size;    /* bytes per tag / value array (kmodel.hpp:437)                   */
	uint64_t byte_km_back;    /* kmodel.hpp:439                                                 */
	uint64_t byte_bf[3], byte_bf_back[3];                          /* kmodel.hpp:411-416        */
	uint64_t fast_commits;    /* successes decided by the uncontended fast path                 */
	uint64_t contended;       /* attempts that went through the ordered slow path -- TIMING-DEPENDENT (a few units in 7e5 from run  */
	uint64_t finisher_iters;  /* to run, like the next one: which candidates meet in flight); iterations of the ordered finisher.   */
	                          /* Every other count of this struct is a function of the input alone.                                 */
	uint64_t blocks, rounds;  /* nb*2^18 blocks and rounds executed                             */
	int32_t  k, ci, cs, nh, nb, bf_num;
	int32_t  device, reserved;
	uint64_t rest_bytes;      /* KRestData::get_all_byte_size (rest.hpp:257-259)                */
	uint64_t piped_attempts;  /* attempts examined / successes committed inside the fused commit|check launches   */
	uint64_t piped_commits;   /* (accounting for the per-kernel roofline: collected only by builds under kmx_set_profile(m, 2)) */
	uint64_t piped_gathers;   /* random 4-byte loads / 32-bit atomic ORs those launches actually ISSUED: the check     */
	uint64_t piped_atomics;   /* stops at the first conflicting group, a winner sets only its untagged positions      */
	uint64_t query_neighbour_calls;  /* packed device queries answered under kmx_set_profile(m, 2) since the last build: how many entered   */
	uint64_t query_accounted;        /* the neighbour disambiguation (kmodel.hpp:344-359) / how many were asked                          */
} kmx_stats;

const char *kmx_last_error(void);
int kmx_device_count(void);
/* Layout version of the structs and array sizes this header declares (kmx_stats, KMX_KERNEL_CLASSES ...): a caller built
 * against an older header must not hand its smaller structs to a newer library -- compare before the first call that
 * takes one (include/kmodel.hpp does, and exits like the reference does on a bad model directory).                    */
#define KMX_ABI_VERSION 5
int kmx_abi_version(void);

/* get_model(ci, cs, num_hash, num_bit)                                     kmodel.hpp:674-677 */
int kmx_create(int ci, int cs, int nh, int nb, kmx_model **out);
/* the reference never frees a model; the handle owns all device memory                        */
int kmx_destroy(kmx_model *m);
/* stream (hipStream_t) used by every later call on this model; NULL = the default stream       */
int kmx_set_stream(kmx_model *m, void *hip_stream);

/* a handle on a given HIP device (kmx_create uses the calling thread's current device, which this call leaves as it was) */
int kmx_create_on(int device, int ci, int cs, int nh, int nb, kmx_model **out);
/* KModel::init(db_file) by several GPUs from ONE process (kmodel.hpp:57-86; main.cpp:143-149 is the caller): models[d] was
 * created on the device it is to use (devices may repeat), all with the same parameters.  One host thread per handle
 * drives the ring of whole arrays (below) with hipMemcpyPeerAsync hand-offs; on return EVERY handle holds the whole model. */
int kmx_build_from_kmc_multi(kmx_model **models, int n_models, const char *db_prefix);
/* The same with the partition chosen.  KMX_PARTITION_RANGE is the north star's: every coupled array cut by POSITION RANGE over
 * the handles (handle q owns the cells [q n/P, (q+1) n/P) of every array; list i of a block lives on handle i % P and its k-mers
 * never move).  A round of the rotation (kmodel.hpp:560-565; check :604-610, set :611-618) is words written by the list
 * handle's kernels STRAIGHT INTO the owner's inbox through a peer mapping (hipDeviceEnablePeerAccess) -- the winners' commits of
 * the round before, then one triple per position of every attempt, with the counts in a header beside them -- and one verdict
 * byte per triple written straight back into the sender's box; two events per handle order the three steps of a round and the
 * host threads only enqueue: no host wait inside a round.  Up to 16 handles; one handle is allowed (the partition's kernels
 * alone).  On return every handle holds the whole model.                                                                       */
#define KMX_PARTITION_RING  0
#define KMX_PARTITION_RANGE 1
/* the same partition with the words of a round as fixed-size RCCL messages instead of peer-mapped stores: one communicator per
 * handle (ncclCommInitAll: the handles must sit on DIFFERENT devices), every region = [header with the counts | capx words]
 * (kmx_range_inband below), a round = two groups of ncclSend / ncclRecv on each handle's stream, nothing of it on the host.
 * librccl.so is opened with dlopen when this is asked for (libkmx.so does not link it).  Should a region overflow, the build
 * is repeated with KMX_PARTITION_RANGE.                                                                                       */
#define KMX_PARTITION_RANGE_RCCL 2
int kmx_build_from_kmc_multi_ex(kmx_model **models, int n_models, const char *db_prefix, int partition);
/* KModel::init(db_file): two passes over the KMC listing + rest build      kmodel.hpp:57-86   */
int kmx_build_from_kmc(kmx_model *m, const char *db_prefix);

/* Host-only view of the KMC listing that init() consumes (CKMCFile::OpenForListing / ReadNextKmer / KmerCount /
 * KmerLength, kmc_file.cpp:66-99, :428-515, :763, :740); needs no GPU.  kmx_kmc_read fills up to `capacity`
 * k-mers (W words each) in listing order, already filtered by the header's [min_count, max_count].          */
int kmx_kmc_info(const char *db_prefix, int *k, uint64_t *total_kmers);
int kmx_kmc_read(const char *db_prefix, uint64_t *kmers, uint32_t *counts, uint64_t capacity, uint64_t *n_read);

/* The same build, streamed.  begin = get_km_kmer_count's result + init_km_bit (kmodel.hpp:423-471):
 * n_bf[i] = number of k-mers with count ci+i (i < bf_num), n_total = KmerCount().                */
int kmx_begin(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total);
/* pass 2 (kmodel.hpp:68-74): batches in LISTING ORDER; host or device pointers                   */
int kmx_insert_batch(kmx_model *m, const uint64_t *kmers, const uint32_t *counts, uint64_t n);
int kmx_insert_batch_dev(kmx_model *m, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n);
/* push_last_to_array / push_last_to_bloomfilter / kld->build()             kmodel.hpp:76-80   */
int kmx_finish(kmx_model *m);
/* one call = pass 1 (device histogram) + begin + insert + finish on a device-resident listing     */
int kmx_build_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n);
int kmx_build_host(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n);

/* ---- ONE model built by several GPUs (one process per GPU) -------------------------------------
 * The reference's insert is n_bits OpenMP threads in a rotation: thread i walks buffer i against array (i + t) % n_bits,
 * barrier, next t (insert_with_thread, kmodel.hpp:557-573).  Here the arrays are owned whole by different GPUs and the
 * survivors of a list travel round the ring as *messages*; the order-free filters (Bloom, back, km_back: set_bit is an
 * atomic OR, kmodel.hpp:576-581) are built as per-rank partial filters and merged by OR.  These entry points are the
 * per-rank compute; the exchange between them (RCCL all-to-all / send-recv / broadcast over xGMI) belongs to the caller
 * (kmcex_amd/dist.py, torch.distributed).  All pointers are DEVICE pointers; work is enqueued on the model's stream.     */
typedef struct kmx_ring_list {
	int32_t list;             /* buffer index i of the block; the round attempts array (i + t) % nb (kmodel.hpp:563) */
	int32_t n_host;           /* >= 0: entries, known on the host (round 0, fresh from the stream); -1: read it from src_msg */
	const void *src_kmers;    /* n_host >= 0: packed k-mers / uint32 counts of the list                                */
	const void *src_counts;
	const void *src_msg;      /* n_host < 0: the list as a message (kmx_ring_msg_bytes) left by kmx_ring_round_dev      */
	void *dst_msg;            /* survivors of this round, in list order, as a message; NULL = last round: rest table     */
} kmx_ring_list;
/* pass 1 on this rank's slice (get_km_kmer_count's histogram, kmodel.hpp:423-428); the caller sums over the ranks      */
int kmx_count_classes_dev(kmx_model *m, const uint32_t *d_counts, uint64_t n, uint64_t n_bf[3]);
/* kmx_begin with whole-model figures (every rank sizes and allocates the whole model, kmodel.hpp:402-456)             */
int kmx_shard_begin(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total, int rank, int world);
/* pass 2 front end on this rank's slice (kmodel.hpp:70-73): Bloom-class k-mers -> this rank's partial filters;
 * coupled-array k-mers compacted in listing order into d_out_* (capacity n); *n_out on the host                       */
int kmx_shard_classify_dev(kmx_model *m, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint64_t *d_out_kmers, uint32_t *d_out_counts, uint64_t *n_out);
/* bytes of one list message: 64-byte header (word 0 = entries) + 2^18 k-mers + 2^18 counts                             */
uint64_t kmx_ring_msg_bytes(int k);
/* insert_array(buff[i], (i + t) % nb, ...) for the lists this rank holds in round t (kmodel.hpp:543-555, :560-565)     */
int kmx_ring_round_dev(kmx_model *m, int t, const kmx_ring_list *lists, int n_lists);
/* stale-slot duplicate of the final partial block for the lists this rank retired (kmodel.hpp:520-527)                 */
int kmx_ring_stale_dup_dev(kmx_model *m, int first_unused_row);
/* this rank's statistics (attempts, successes, ..., rest_entries = survivors it holds) and its survivor list           */
int kmx_shard_local(kmx_model *m, kmx_stats *partial, void **d_rest_kmers, void **d_rest_counts);
/* kld->build() on the survivors of ALL ranks + the summed statistics; the handle becomes a full replica (kmodel.hpp:80) */
int kmx_shard_complete(kmx_model *m, const uint64_t *d_rest_kmers, const int32_t *d_rest_counts, uint64_t n_rest, const kmx_stats *totals);
/* ---- the same model with every coupled array cut by POSITION RANGE over the ranks: rank q owns the cells
 * [cell_lo[q], cell_lo[q+1]) -- 16 positions each -- of every array; list i of a block lives on rank i % world for the whole
 * block and its k-mers never move.  A round of insert_array (kmodel.hpp:543-555, :560-565; check :604-610, set :611-618) is
 * two exchanges of 64-bit words / bytes that the CALLER moves between the ranks (all-to-all over RCCL): triples out (behind the
 * commits of the round before), verdicts back.  kmx_count_classes_dev, kmx_shard_classify_dev, kmx_ring_stale_dup_dev,
 * kmx_shard_local / _complete and kmx_dev_view are shared with the ring.                                                */
int kmx_range_begin(kmx_model *m, int k, const uint64_t n_bf[3], uint64_t n_total, int rank, int world);
/* the regions: region q (cap_words 64-bit words apart) holds what the last emit left for rank q -- commits in front, triples behind  */
int kmx_range_buffers(kmx_model *m, void **d_send, uint64_t *cap_words, uint64_t *cell_lo /* [world + 1] */);
/* step 1, list rank: every position of every attempt of its lists as a triple, by owner rank, appended behind the commits
 * the last kmx_range_resolve_dev left in front of the regions; on the host counts[q] = words for rank q, counts[world + q] =
 * the commit words among them (the header of the region: the owner needs both).
 * t == 0: `lists` = the fresh buffers of the block this rank holds (list, n_host, src_kmers, src_counts)              */
int kmx_range_emit_dev(kmx_model *m, int t, const kmx_ring_list *lists, int n_lists, uint64_t *counts /* [2 world] */);
/* step 2, owner: d_words = the regions of the n_src senders back to back (totals[s] words, the first commits[s] of them commit
 * words).  Applies the commit words (the set loop :611-618 of the round before), then answers every triple with one byte at the
 * same index of d_verdict: conflict | untagged | wanted with both values this round (the bytes of commit words stay unwritten);
 * fewer than 2^27 triples per call (KMX_E_ARG beyond: a round of nb = nh = 16 holds 2^26)                                  */
int kmx_range_verdict_dev(kmx_model *m, int t, const uint64_t *d_words, const uint64_t *totals, const uint64_t *commits, int n_src, uint8_t *d_verdict);
/* step 3, list rank: verdicts in the order the words left (regions back to back, in rank order) -> winners (the contended
 * ones decided in list order); their commits go to the front of the regions for the next emit; reorder_buffer (:529-540),
 * km_back, rest.  Nothing is exchanged now, and no host wait is spent                                                   */
int kmx_range_resolve_dev(kmx_model *m, int t, const uint8_t *d_verdict);
/* FIXED-SIZE MESSAGES (no count on the host, two equal-split all-to-alls per round).  Call between kmx_range_begin and the first
 * emit: every region becomes [header: commits, triples, 0, 0 as uint32 | capx_words 64-bit words], region_words = 2 + capx apart
 * in *d_send -- capx = the mean of a round's fullest exchange + 25 % + 8192 words, far beyond what uniformly hashed positions
 * deviate.  Then kmx_range_emit_dev / kmx_range_flush_dev take counts = NULL and do not wait; the owner reads what arrived -- the
 * world regions of its senders, same layout -- with kmx_range_verdict_inband_dev (verdict byte of word j of region s at
 * d_verdict[s * capx + j]) and kmx_range_commit_inband_dev; kmx_range_resolve_dev takes the bytes that came back, capx per
 * destination.  A word that does not fit its region is DROPPED and the build is void: kmx_shard_local reports it in
 * kmx_stats.reserved (non-zero), and the caller repeats the build with counted messages (kmcex_amd/dist.py does).           */
int kmx_range_inband(kmx_model *m, void **d_send, uint64_t *region_words, uint64_t *capx_words);
int kmx_range_verdict_inband_dev(kmx_model *m, int t, const uint64_t *d_recv, int n_src, uint8_t *d_verdict);
int kmx_range_commit_inband_dev(kmx_model *m, const uint64_t *d_recv, int n_src);
/* end of the build: what is still pending in front of the regions (counts[q] = counts[world + q] = commit words) for a last exchange ... */
int kmx_range_flush_dev(kmx_model *m, uint64_t *counts /* [2 world] */);
/* ... and its application on the owner                                                                                  */
int kmx_range_commit_dev(kmx_model *m, const uint64_t *d_commits, uint64_t n);

/* device memory of filter / array storage for the caller's collectives: which 0 bf[i], 1 bf_back[i], 2 km_back
 * (bytes rounded up to 32-bit words), 3 the cells of coupled array i (value+tag interleaved, 8 bytes per 16 positions)  */
int kmx_dev_view(kmx_model *m, int which, int index, void **ptr, uint64_t *bytes);
/* dst |= src over n 32-bit words (merging partial filters)                                                              */
int kmx_or_words_dev(kmx_model *m, void *d_dst, const void *d_src, uint64_t n_words);

/* vector<int> KModel::kmer_to_occ(vector<string>, t_num)                   kmodel.hpp:90-98
 * Threads: the query functions below may be called on one handle from any number of host threads at once (the
 * reference calls kmer_to_occ from an OpenMP loop); the library serialises them per handle, one query at a time.
 * A build, load, save or destroy of a handle must not overlap anything else on that handle.                              */
int kmx_query_packed(kmx_model *m, const uint64_t *kmers, uint64_t n, int32_t *out);
int kmx_query_packed_dev(kmx_model *m, const uint64_t *d_kmers, uint64_t n, int32_t *d_out);
/* n records of `stride` bytes holding `len` characters each (not NUL-terminated), 2 <= len <= 64.  Strings of
 * the model's k over ACGT take the packed kernel; anything else is hashed byte for byte like the reference does. */
int kmx_query_ascii(kmx_model *m, const char *strs, int len, int stride, uint64_t n, int32_t *out);
/* the same for n separate strings of `len` characters each (strs[i] need not be NUL-terminated): what a
 * vector<string> holds, without concatenating it first */
int kmx_query_strings(kmx_model *m, const char *const *strs, int len, uint64_t n, int32_t *out);
/* kmer_to_occ (kmodel.hpp:100-116) of every k-mer window of n_seqs sequences stored back to back: sequence i is
 * seq[offsets[i] .. offsets[i+1]), offsets[0] = 0, n_bases = offsets[n_seqs]; out[n_bases] is aligned to the bases.
 *   out[offsets[i] + p] = kmer_to_occ(s_i.substr(p, k)) for 0 <= p <= len_i - k: bit for bit what kmx_query_ascii gives that
 *                         window (uppercase ACGT windows take the packed path, any other byte -- N, lowercase, IUPAC -- is
 *                         hashed as it is, never uppercased);
 *   out[offsets[i] + p] = -1 for the last k - 1 positions of each sequence and every position of one shorter than k.
 *                         kmer_to_occ never returns -1: its answers are rest-table counts (>= ci >= 1), OccuBin means
 *                         (occubin_tables / bin_to_mean, occu_bin.hpp:27-83: all >= 0) or 0.
 * Indices are 64-bit throughout (one sequence may be a whole genome).  KMX_E_ARG when offsets[0] != 0 or the offsets
 * decrease (checked before anything runs); n_seqs == 0 or n_bases == 0: KMX_OK, nothing written.  The bases travel as
 * they are (one byte per window) and the windows are built on the device; the answers are timed as kernel class 6 (query)
 * under kmx_set_profile(m, 1), and kmx_set_profile(m, 2)'s accounting (query_neighbour_calls) does not cover them.    */
int kmx_query_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t *out);
/* the same on DEVICE buffers: d_seq[n_bases], d_offsets[n_seqs + 1], d_out[n_bases]; enqueued on the model's stream, returns
 * without waiting.  The offsets are not validated on the host: the kernels clamp every offset into [0, n_bases] and treat
 * a decreasing pair as an empty sequence, so bad offsets give wrong answers, never an access outside d_seq / d_out.   */
int kmx_query_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t *d_out);

/* The answers of kmx_query_seqs reduced per sequence on the device: what error correction, repeat detection and read
 * filtering ask of a read (how many of its k-mers are solid, the lowest and highest count, the mean = sum / n_windows,
 * whether the median reaches a coverage target: 2 * n_ge[j] > n_windows, where the first and last weak k-mer lie).  64 bytes
 * per sequence come back instead of 4 per base, and the host reduces nothing.                                            */
#define KMX_SEQ_THRESHOLDS 3
typedef struct kmx_seq_summary {     /* one per sequence; 64 bytes, no padding */
	uint64_t n_windows;              /* max(len - k + 1, 0)                                                         */
	uint64_t sum;                    /* sum of the windows' answers (each is kmer_to_occ of that window, >= 0)       */
	int32_t  min, max;               /* over the windows; -1, -1 when n_windows == 0                                 */
	uint64_t n_ge[KMX_SEQ_THRESHOLDS]; /* windows with answer >= thr[j]; 0 for j >= n_thr                            */
	uint64_t first_below;            /* smallest window index p (0-based, inside the sequence) with answer < thr[0]; */
	uint64_t last_below;             /* largest such p.  Both = n_windows when there is none, or when n_thr == 0      */
} kmx_seq_summary;
/* Sequences in the layout of kmx_query_seqs (sequence i = seq[offsets[i] .. offsets[i+1]), offsets[0] = 0, 64-bit).
 *   The windows and their answers are EXACTLY those of kmx_query_seqs: out[i] is what a caller computes from kmx_query_seqs'
 *   out[offsets[i] .. offsets[i+1]) after dropping the -1 entries.  Windows with N, lowercase or IUPAC bytes are answered
 *   byte for byte as there, and take part in the summary.
 *   thr holds n_thr values, 0 <= n_thr <= KMX_SEQ_THRESHOLDS (KMX_E_ARG otherwise, and for n_thr > 0 with thr == NULL); any
 *   int32 is a legal threshold and they need not ascend; thr[0] also defines first_below / last_below.
 *   Every counter is 64-bit (one sequence may be a whole genome), and every field is an integer sum, count, minimum or
 *   maximum: two runs, the host and the device variant, and any chunk size give identical bytes.
 * KMX_E_ARG when offsets[0] != 0 or the offsets decrease, checked before anything runs; n_seqs == 0: KMX_OK, nothing written;
 * no bases but n_seqs > 0: every record is the empty one (n_windows = 0, min = max = -1, first_below = last_below = 0) --
 * unlike kmx_query_seqs there is something to write.  KMX_E_STATE before the model is built or loaded; KMX_E_NOMEM when the
 * call's memory (72 bytes per sequence on the device: the records and the offsets; the handle's pinned slots and dirty list,
 * shared with kmx_query_seqs) cannot be had, and the handle stays usable: the same call may be repeated.  The
 * bases travel as in kmx_query_seqs and nothing per base comes back; the call returns when out is complete.  A query-class
 * call (see the threading note of kmx_query_packed), timed as kernel class 6 under kmx_set_profile(m, 1).                */
int kmx_summarise_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs,
                       const int32_t *thr, int n_thr, kmx_seq_summary *out /* [n_seqs] */);
/* the same on DEVICE buffers d_seq[n_bases], d_offsets[n_seqs + 1], d_out[n_seqs] (thr is read on the HOST, during the call);
 * enqueued on the model's stream, returns without waiting.  d_out[0, n_seqs) is overwritten whatever it held.  The offsets
 * are not validated on the host: as in kmx_query_seqs_dev each is clamped into [0, n_bases] where it is read and a decreasing
 * pair is an empty sequence, so bad offsets give wrong records, never an access outside d_seq[0, n_bases) / d_out[0, n_seqs). */
int kmx_summarise_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                           const int32_t *thr /* HOST, n_thr values */, int n_thr, kmx_seq_summary *d_out /* [n_seqs] */);

/* Substitution errors of reads corrected from the k-mer spectrum: what kmx_query_seqs' answers are for.  Everything is
 * decided from the answers on the INPUT bases (bit for bit those of kmx_query_seqs, dirty windows hashed byte for byte as
 * there); no decision depends on another correction, so the result does not depend on the order of evaluation, the cut into
 * pieces and chunks, or the variant.  Per sequence of length L: nW = max(L - k + 1, 0) windows, window p covers the bases
 * p .. p+k-1; thr is any int32, min_support in [1, 64].
 *   1. weak(p) = answer(p) < thr; n_weak counts these.
 *   2. Gap closing: a window 0 < p < nW-1 that is not weak while p-1 and p+1 are weak (judged on weak, not on closed flags)
 *      counts as weak for run forming (the model answers about 0.7 % of erroneous k-mers with a positive count).
 *   3. A run [s, e] is a maximal stretch of (closed) weak windows, len = e-s+1; n_runs counts them.  hasL = s > 0,
 *      hasR = e < nW-1.  Its sites (base b, verification windows V = [v0, v1]):
 *        neither hasL nor hasR: none;   hasR only: b = e, V = [max(s, e-k+1), e];   hasL only: b = s+k-1, V = [s, min(e, s+k-1)];
 *        both, len < k: none;   both, len = k: b = e, V = [s, e];
 *        both, len > k: two: b = s+k-1, V = [s, min(s+k-1, e-k)]  and  b = e, V = [max(e-k+1, s+k), e].
 *      A site is tried iff v1-v0+1 >= min_support; n_sites counts the tried ones.
 *   4. The candidates of a tried site are 'A', 'C', 'G', 'T' in that order without the input byte at b (an N, IUPAC or
 *      lowercase byte has four).  A candidate passes iff every window of V, taken from the input with only base b replaced,
 *      answers >= thr (the answer kmx_query_ascii gives those k bytes).  Exactly one passes: the output byte at b is that
 *      candidate, n_corrected++; more than one: n_ambiguous++; none: n_unfixable++ (byte unchanged in both).
 *   5. Every other output byte equals the input byte.
 * Out of scope: insertions / deletions, more than the two outer errors of a long run per call (call again on the output),
 * quality values.                                                                                                         */
typedef struct kmx_seq_correction {      /* one per sequence; 64 bytes, no padding */
	uint64_t n_windows, n_weak, n_runs, n_sites, n_corrected, n_ambiguous, n_unfixable, reserved /* 0 */;
} kmx_seq_correction;
/* Sequences in the layout of kmx_query_seqs.  seq_out[n_bases] receives the corrected bases (seq_out == seq corrects in
 * place; any other overlap is KMX_E_ARG), rec[n_seqs] the records (may be NULL).  KMX_E_ARG when min_support is outside
 * [1, 64], offsets[0] != 0 or the offsets decrease, all checked before anything runs; n_seqs == 0: KMX_OK, nothing written;
 * no bases but n_seqs > 0: all-zero records.  KMX_E_STATE before the model is built or loaded; KMX_E_NOMEM leaves the handle
 * usable.  The bases travel as in kmx_query_seqs; the corrections come back as a sparse (position, base) list, not one byte
 * per base.  A query-class call, timed as kernel class 6 under kmx_set_profile(m, 1).                                      */
int kmx_correct_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs,
                     int32_t thr, int min_support, char *seq_out /* [n_bases] */, kmx_seq_correction *rec /* [n_seqs] or NULL */);
/* the same on DEVICE buffers d_seq[n_bases], d_offsets[n_seqs + 1], d_seq_out[n_bases], d_rec[n_seqs] (or NULL); enqueued on
 * the model's stream, returns without waiting.  d_seq_out must not overlap d_seq (KMX_E_ARG).  The offsets are not validated
 * on the host: each is clamped into [0, n_bases] where it is read, so bad offsets give wrong output, never an access outside
 * d_seq[0, n_bases), d_seq_out[0, n_bases), d_rec[0, n_seqs).                                                              */
int kmx_correct_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                         int32_t thr, int min_support, char *d_seq_out, kmx_seq_correction *d_rec /* or NULL */);

/* Substitutions and single-base insertions / deletions of reads found from the k-mer spectrum: kmx_correct_seqs with a wider
 * shape table, verification windows built with one base skipped or inserted, and an output that may change a read's length.
 * As there, every decision is taken from the answers on the INPUT bytes and none depends on another edit, so the result is a
 * function of the input alone: it does not depend on the order of evaluation, the cut into pieces, or the variant.  An edit
 * list in input coordinates is also a SNP / indel call list when a reference sequence is run against a sample's model.
 * Steps 1 - 3 of kmx_correct_seqs hold word for word (weak windows, gap closing, runs [s, e], len, hasL, hasR).  x = the
 * sequence's bytes, L its length, nW its window count; thr is any int32, min_support in [1, 64], ops a non-empty subset of
 * KMX_EDIT_OPS_SUB | KMX_EDIT_OPS_DEL | KMX_EDIT_OPS_INS.
 *   Candidates: an edited string t and verification windows V (start positions q in t, every window k bytes of t).
 *     SUB at p, base c: x with x[p] replaced by c;  V = [v0, v1] of kmx_correct_seqs' table for that site.
 *     DEL at p:         x without x[p] (the read has a base in excess);  V = the windows of t that hold both new neighbours,
 *                       q in [max(0, p-k+1), min(p-1, L-1-k)].
 *     INS at j, base c: x with c placed before x[j] (the read lost a base);  V = the windows of t that hold the new base,
 *                       q in [max(0, j-k+1), min(j, L+1-k)].
 *     c is one of A C G T.
 *   Sites of a run, the candidates in this order, each kind only if its ops bit is set:
 *     neither hasL nor hasR: none;
 *     hasR only: anchor a = e, junction j = e+1: SUB at a for c != x[a] with V = [max(s, e-k+1), e]; DEL at a; INS at j for all four c;
 *     hasL only: a = j = s+k-1: SUB at a with V = [s, min(e, s+k-1)]; DEL at a; INS at j for all four c;
 *     both, len > k: the two SUB sites of kmx_correct_seqs' table and nothing else;
 *     both, len <= k: one site; its core is the bytes common to all the run's windows, x[e .. s+k-1], h = k-len+1 of them:
 *       len = k: SUB at e for c != x[e], V = [s, e];
 *       DEL at e iff all h core bytes are equal (always so for h = 1; deleting any byte of a homopolymer gives the same
 *       string, the leftmost is the canonical one);
 *       h = 2: INS at e+1 for all four c;   h >= 3: the single INS at e+1 with c = x[e+1], provided x[e+1 .. s+k-2] are all
 *       that byte and it is one of ACGT.
 *     (A surplus base inside a homopolymer of h bytes makes exactly the windows holding the whole homopolymer plus a flank
 *     weak: len = k-h+1.  A lost base whose homopolymer keeps m bytes makes the windows holding flank, A^m, flank weak:
 *     len = k-1-m, the core those m+2 bytes.  At a read end only one edge of the run is visible, so all three kinds are tried.)
 *   A candidate is tried iff |V| >= min_support, a site iff one of its candidates is; n_sites counts the tried sites.  A tried
 *   candidate passes iff every window of V answers >= thr (the answer kmx_query_ascii gives those k bytes: bytes outside ACGT
 *   are hashed as they are).  Exactly one passes: it becomes an edit and n_sub / n_del / n_ins is incremented; more than one:
 *   n_ambiguous++; none: n_unfixable++.
 *   With ops = KMX_EDIT_OPS_SUB the tried sites, counts and changed bytes are exactly those of kmx_correct_seqs.  Anchors of
 *   distinct sites are distinct and junctions lie inside their sequence, so (pos, op) is unique: one position carries at most
 *   one of SUB / DEL, possibly plus one INS.
 * Out of scope: more than one base per edit; two errors within k of each other stay substitution-only (both, len > k); more
 * than the two outer errors of a long run per call (call again on the output, or kmx_polish_seqs); quality values.         */
#define KMX_EDIT_OPS_SUB 1
#define KMX_EDIT_OPS_DEL 2
#define KMX_EDIT_OPS_INS 4
#define KMX_EDIT_SUB 1
#define KMX_EDIT_DEL 2
#define KMX_EDIT_INS 3
/* pos << 8 | op << 4 | code: pos = position in the whole input (flat), op = KMX_EDIT_SUB / KMX_EDIT_DEL / KMX_EDIT_INS (insert
 * before the base at pos), code 0..3 = A C G T (0 for DEL)                                                                 */
typedef uint64_t kmx_edit;
typedef struct kmx_seq_edits {           /* one per sequence; 80 bytes, no padding; out_len = L + n_ins - n_del */
	uint64_t n_windows, n_weak, n_runs, n_sites, n_sub, n_del, n_ins, n_ambiguous, n_unfixable, out_len;
} kmx_seq_edits;
/* Sequences in the layout of kmx_query_seqs.  edits[capacity] receives the list, sorted ascending as numbers (so it is
 * byte-identical across runs, variants and piece sizes), *n_edits the number of edits found, rec[n_seqs] the records (may be
 * NULL).  More edits than capacity: KMX_E_RANGE, *n_edits is the number needed, the records are complete, the list's content
 * is unspecified; capacity >= n_bases / 3 + 1 always suffices (runs lie at least two windows apart after gap closing, and only
 * a run longer than k has two sites).  KMX_E_ARG when ops is outside 1..7, min_support outside [1, 64], offsets[0] != 0 or the
 * offsets decrease, all checked before anything runs; n_seqs == 0: KMX_OK, nothing written; no bases but n_seqs > 0: all-zero
 * records, *n_edits = 0.  KMX_E_STATE before the model is built or loaded; KMX_E_NOMEM leaves the handle usable.  A run at an
 * end of its sequence takes other candidates than one inside however long it is, so the weak bits of the whole input are kept
 * (n_bases / 8 bytes) and the bases stay on the device for the call: the host variant uploads them whole (n_bases bytes of
 * device memory).  A query-class call, timed as kernel class 6 under kmx_set_profile(m, 1).                                */
int kmx_edit_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, int ops,
                  kmx_edit *edits, uint64_t capacity, uint64_t *n_edits, kmx_seq_edits *rec /* [n_seqs] or NULL */);
/* the same on DEVICE buffers d_seq[n_bases], d_offsets[n_seqs + 1], d_edits[capacity], d_rec[n_seqs] (or NULL); n_edits is on
 * the HOST.  Enqueued on the model's stream; it waits for the stream once, where the count reaches the host, and returns with
 * the sort of the list enqueued.  The offsets are not validated on the host: each is clamped into [0, n_bases] where it is
 * read, so bad offsets give wrong edits, never an access outside d_seq[0, n_bases), d_edits[0, capacity), d_rec[0, n_seqs).   */
int kmx_edit_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, int ops,
                      kmx_edit *d_edits, uint64_t capacity, uint64_t *n_edits /* HOST */, kmx_seq_edits *d_rec /* or NULL */);
/* A list applied to the input it was found on; needs no GPU.  Walk the input positions p of a sequence in order: emit the
 * inserted base if an INS sits at p, then the input byte, or its SUB base, or nothing for a DEL.  seq_out[out_capacity]
 * receives the bytes, offsets_out[n_seqs + 1] the running sum of the output lengths (the records' out_len).  KMX_E_ARG when the
 * list is not strictly ascending, a pos >= n_bases, an unknown op or code, SUB and DEL at one pos, or bad offsets;
 * KMX_E_RANGE when out_capacity is too small (n_bases + the insertions - the deletions are needed).                         */
int kmx_apply_edits(const char *seq, const uint64_t *offsets, uint64_t n_seqs, const kmx_edit *edits, uint64_t n_edits,
                    char *seq_out, uint64_t out_capacity, uint64_t *offsets_out /* [n_seqs + 1] */);
/* the same on DEVICE buffers, enqueued on the model's stream; waits once, for the output's length (KMX_E_RANGE as above, after
 * the bytes that fit were written).  The list is not validated on the device: one that is no sorted edit list of this input gives
 * wrong bytes, never a write outside d_seq_out[0, out_capacity) and d_offsets_out[0, n_seqs].  Needs no built model.       */
int kmx_apply_edits_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, const kmx_edit *d_edits, uint64_t n_edits,
                        char *d_seq_out, uint64_t out_capacity, uint64_t *d_offsets_out);

/* Reads polished to a fixed point: kmx_edit_seqs' rule iterated per read, entirely on the device.  One pass of kmx_edit_seqs
 * fixes at most the two outer errors of a long run, leaves two errors within k of each other as they are, and cannot decide
 * an edit whose neighbour must be fixed first; the loop that handles them is this call.  kmx_edit_seqs decides everything
 * about a sequence from that sequence's own bytes and the model's answers, so the definition is per sequence and order-free.
 * For a sequence, x_0 is the input.  For p = 1 .. max_passes:
 *   1. (E_p, r_p) = the edit list and the kmx_seq_edits record that kmx_edit_seqs(thr, min_support, ops) gives x_(p-1) as a
 *      batch of its own.
 *   2. E_p is empty: stop; the sequence has converged: n_passes = p, converged = 1.
 *   3. Otherwise x_p = kmx_apply_edits(x_(p-1), E_p).
 * If pass max_passes still produced edits, n_passes = max_passes and converged = 0.  The output is the last x.  An edit always
 * changes the bytes (a SUB has c != x[a], DEL / INS change the length), so "no edits" is the fixed point: a sequence that
 * found none would find none again, and retiring it after that pass is exact.  Consequences:
 *   - the result is byte for byte that of the host loop: kmx_edit_seqs then kmx_apply_edits on the whole batch, repeated until
 *     a pass returns an empty list or max_passes passes ran;
 *   - it does not depend on the variant, the cut into pieces, or which reads share a batch;
 *   - max_passes = 1 gives the reads of kmx_edit_seqs + kmx_apply_edits, and a record whose sums are that record's;
 *   - with ops = KMX_EDIT_OPS_SUB it is iterated kmx_correct_seqs.
 * Only the reads a pass edited are examined by the next one; a read that pass 1 leaves alone is never copied until the final
 * gather.  Nothing guarantees an end in general (no read of the test data returns to a string it held before, and all have
 * converged by pass 3), hence max_passes in [1, KMX_POLISH_MAX_PASSES].
 * Out of scope: quality values; FASTQ in / out; a composed edit list in input coordinates (ambiguous once two passes touch
 * one place: run kmx_edit_seqs pass by pass for lists); several GPUs; choosing thr.                                          */
#define KMX_POLISH_MAX_PASSES 16
typedef struct kmx_seq_polish {          /* one per sequence; 96 bytes, no padding */
	uint64_t n_passes, converged;
	uint64_t n_sub, n_del, n_ins;        /* sums over the passes that examined the sequence */
	uint64_t out_len;                    /* length of the output read */
	uint64_t n_windows, n_weak, n_runs, n_sites, n_ambiguous, n_unfixable;   /* of the last pass that examined it; when converged = 1 they describe the output read itself */
} kmx_seq_polish;
/* Sequences in the layout of kmx_query_seqs.  seq_out[out_capacity] receives the polished reads in the input's order,
 * offsets_out[n_seqs + 1] the running sum of out_len, rec[n_seqs] the records (may be NULL), *passes_run (may be NULL) the
 * largest n_passes.  offsets_out[n_seqs] > out_capacity: KMX_E_RANGE; records and offsets_out are complete, the bytes that fit
 * are written, nothing is written at or behind seq_out[out_capacity].  KMX_E_ARG when max_passes is outside [1, 16], ops outside
 * 1..7, min_support outside [1, 64], offsets[0] != 0, the offsets decrease, or seq_out overlaps seq (lengths change: there is no
 * in-place form), all checked before anything runs; n_seqs == 0: KMX_OK, nothing written; no bases but n_seqs > 0: records with
 * n_passes = 1, converged = 1 and zeros elsewhere, offsets_out all 0.  KMX_E_STATE before the model is built or loaded;
 * KMX_E_NOMEM leaves the handle usable.  The bases go up once; reads, offsets and records come down once; nothing else crosses
 * the link between passes.  Device memory, kept on the handle between calls: with B_p the bytes of the reads pass p examines
 * (B_1 = n_bases, B_2 = the bytes of the reads pass 1 edited, ...), B_1 / 8 for the weak bits, 16 (B_1 / 3 + 1) for a pass's
 * list and its sort, B_2 + B_3 for the two batches the passes alternate between, and a parking area for the reads that retire
 * after pass 1 (those of pass max_passes go straight to seq_out): at most B_2 plus their insertions in all; about 150 bytes
 * per sequence for records, lengths, homes and maps.  The host
 * variant adds n_bases + min(offsets_out[n_seqs], out_capacity).  A query-class call, timed as kernel class 6 under
 * kmx_set_profile(m, 1).                                                                                                   */
int kmx_polish_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, int32_t thr, int min_support, int ops, int max_passes,
                    char *seq_out, uint64_t out_capacity, uint64_t *offsets_out /* [n_seqs + 1] */,
                    kmx_seq_polish *rec /* [n_seqs] or NULL */, uint64_t *passes_run /* or NULL */);
/* the same on DEVICE buffers d_seq[n_bases], d_offsets[n_seqs + 1], d_seq_out[out_capacity], d_offsets_out[n_seqs + 1],
 * d_rec[n_seqs] (or NULL); passes_run is on the HOST.  Pass 1 reads d_seq in place.  Enqueued on the model's stream; it waits
 * for the stream once per pass, where the pass's counts reach the host, and once for the final length (which rides on the last
 * pass's wait when that is pass max_passes), nowhere else, and returns with the last copies into d_seq_out enqueued.  The offsets are not validated on the host: each is clamped into [0, n_bases] where it is read, so bad
 * offsets give wrong reads (or KMX_E_ARG, when they claim more bytes than n_bases), never an access outside d_seq[0, n_bases),
 * d_seq_out[0, out_capacity), d_offsets_out[0, n_seqs], d_rec[0, n_seqs).                                                   */
int kmx_polish_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, int32_t thr, int min_support, int ops, int max_passes,
                        char *d_seq_out, uint64_t out_capacity, uint64_t *d_offsets_out, kmx_seq_polish *d_rec /* or NULL */, uint64_t *passes_run /* HOST, or NULL */);

/* Seeds extended to the right along unique k-mer paths: a walk through the de Bruijn graph the model implicitly holds (the
 * primitive of unitig construction, gap filling, seed-and-extend).  occ(s) is the answer kmx_query_ascii gives the k bytes s;
 * every string a walk asks about is uppercase ACGT, so it is also kmx_query_packed of its packed form.  The result is a
 * function of those answers alone and independent per seed: it does not depend on the batch, the cut into chunks and
 * launches, or the variant.  thr is any int32, max_ext in [1, KMX_EXT_MAX_EXT_LIMIT], depth in [0, KMX_EXT_MAX_DEPTH].
 * The model answers some absent k-mers with a positive count; without a tie-break a walk meets such a neighbour within a
 * dozen bases or so and stops.  The tie-break is a lookahead, defined as an existence statement so that no order of evaluation shows:
 *   sup_f(x, 0) is true; sup_f(x, d) holds iff some c in ACGT has occ(x[1:] + c) >= thr and sup_f(x[1:] + c, d - 1);
 *   sup_b(x, d) is its mirror image with c + x[:-1].
 * Per seed i (sequences in the layout of kmx_query_seqs):
 *   1. A seed shorter than k, or whose last k bytes hold anything but uppercase ACGT: stop = KMX_EXT_BAD_SEED, n_ext = 0,
 *      seed_occ = -1.  Otherwise cur = first = the last k bytes and seed_occ = occ(first); the seed need not be solid.
 *   2. Step: a_c = occ(cur[1:] + c) and b_d = occ(d + cur[1:]) for c, d in A, C, G, T (the successors of cur and the
 *      predecessors of the k-mer the walk would move to).  S = {c : a_c >= thr}; if |S| > 1 and depth > 0,
 *      S = {c in S : sup_f(cur[1:] + c, depth)}.  |S| == 0: stop = KMX_EXT_DEAD_END; |S| > 1: stop = KMX_EXT_BRANCH.
 *      Otherwise P = {d != cur[0] : b_d >= thr}; if P is not empty and depth > 0, P = {d in P : sup_b(d + cur[1:], depth)}.
 *      P not empty: stop = KMX_EXT_JOIN.  (DEAD_END and BRANCH come before JOIN.)
 *   3. nxt = cur[1:] + c for the one c in S.  nxt == first: stop = KMX_EXT_CYCLE, nothing is appended.
 *   4. Append c: n_ext++; sum_occ, min_occ, max_occ take a_c; n_lookahead++ if this step evaluated sup_f or sup_b;
 *      cur = nxt; n_ext == max_ext: stop = KMX_EXT_MAX_EXT.  Otherwise step again.
 * ext[i * max_ext .. i * max_ext + n_ext) holds the appended bases, the rest of the row is 0.
 * Leftward extension is rightward extension of the reverse complement (the Python facade's left=True does that on the
 * host); the ABI is rightward only.  For k > 32 the reference canonicalises through one 64-bit word, so the two strands of a
 * k-mer need not get the same answer there and a leftward walk need not mirror the rightward one.
 * Out of scope: marking k-mers as visited across seeds (the result would depend on the order), bubble popping, tip removal
 * beyond the tie-break.                                                                                                    */
#define KMX_EXT_DEAD_END 1
#define KMX_EXT_BRANCH 2
#define KMX_EXT_JOIN 3
#define KMX_EXT_CYCLE 4
#define KMX_EXT_MAX_EXT 5
#define KMX_EXT_BAD_SEED 6
#define KMX_EXT_MAX_EXT_LIMIT 65536
#define KMX_EXT_MAX_DEPTH 3
typedef struct kmx_seq_extension {       /* one per seed; 32 bytes, no padding */
	uint32_t n_ext, stop;
	int32_t  seed_occ, min_occ, max_occ;   /* min_occ = max_occ = -1 when n_ext == 0 */
	uint32_t n_lookahead;
	uint64_t sum_occ;
} kmx_seq_extension;
/* ext[n_seqs * max_ext] receives the rows, rec[n_seqs] the records (may be NULL).  KMX_E_ARG when max_ext or depth is out of
 * range, offsets[0] != 0 or the offsets decrease, all checked before anything runs; n_seqs == 0: KMX_OK, nothing written.
 * KMX_E_STATE before the model is built or loaded; KMX_E_NOMEM leaves the handle usable.  Only the last k bytes of every
 * seed cross the link; the seeds run in chunks, so the device memory for ext stays bounded.  A query-class call, timed as
 * kernel class 6 under kmx_set_profile(m, 1).  No kernel launch walks a seed more than a bounded number of steps; walks that
 * have not stopped are compacted and launched again.                                                                       */
int kmx_extend_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs,
                    int32_t thr, int max_ext, int depth, char *ext /* [n_seqs * max_ext] */, kmx_seq_extension *rec /* [n_seqs] or NULL */);
/* the same on DEVICE buffers d_seq[n_bases], d_offsets[n_seqs + 1], d_ext[n_seqs * max_ext], d_rec[n_seqs] (or NULL); enqueued
 * on the model's stream, returns without waiting (the host reads nothing back between the launches).  The offsets are not
 * validated on the host: each is clamped into [0, n_bases] where it is read, so bad offsets give wrong walks, never an
 * access outside d_seq[0, n_bases), d_ext[0, n_seqs * max_ext), d_rec[0, n_seqs).                                           */
int kmx_extend_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                        int32_t thr, int max_ext, int depth, char *d_ext, kmx_seq_extension *d_rec /* or NULL */);

/* ---- k-mer counting on the device: KMC's step of the pipeline, then KModel::init on what it lists
 * (main.cpp:137-146 runs KMC on the reads, then init on its database; kmodel.hpp:57-86).
 * The counting rule:
 *   - bases are A C G T and a c g t, coded A=0 C=1 G=2 T=3 (KMC's CKmerAPI::num_codes, kmc_api/kmer_api.h:264-275); every
 *     other byte (N, IUPAC letters, anything else) is not a base.  Lowercase counts as bases HERE, while kmx_query_seqs /
 *     kmer_to_occ hash a lowercase window byte for byte, as the reference does: that asymmetry is the reference pipeline's;
 *   - a window is counted when it lies wholly inside one sequence and holds k bases: k-mers never span two sequences;
 *   - its key is the canonical k-mer: the numeric minimum of the 2k-bit forward word and its reverse complement, for every k
 *     in [4, 64] (the model's own hashing keeps the reference's k > 32 quirk; it is not part of the count);
 *   - c = the windows with that key, saturating at 2^32 - 1.  A k-mer is listed iff ci <= c <= 10^9 (10^9 is KMC's default
 *     -cx, which the reference's driver keeps; tests/test_gpu_count_edges.py reaches 10^9, 10^9 + 1 and 2^32 + 5), with
 *     the count min(c, cs); ci, cs are the handle's (kmx_create);
 *   - the listing is ascending by the 2k-bit integer (word 0 most significant): the order of a KMC1-layout database.
 * The model kmx_count_finish builds is kmx_build_dev on that listing, so it is bit-identical to KModel::init on a KMC1-layout
 * database holding those k-mers and counts.  A KMC 3 database (KMC2 layout) lists the same k-mers bin-major, in an order set
 * by KMC's signature binning; the reference's model of it has the same k-mers and counts, but its arrays may differ.
 * Counting calls are build-class calls (see the threading note of kmx_query_packed).  A failure inside a session
 * (KMX_E_NOMEM, KMX_E_IO, KMX_E_NODEVICE) ends it and leaves the previous model as it was.                                */
/* start a session for k in [4, 64]; the model is untouched until finish; drops the listing of an earlier finish           */
int kmx_count_begin(kmx_model *m, int k);
/* count the windows of n_seqs sequences on HOST buffers, in the layout of kmx_query_seqs (offsets[0] = 0, non-decreasing,
 * 64-bit, checked before anything runs: KMX_E_ARG); n_seqs == 0 or no bases: KMX_OK.  Outside a session: KMX_E_STATE      */
int kmx_count_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs);
/* the same on DEVICE buffers d_seq[n_bases], d_offsets[n_seqs + 1], enqueued on the model's stream; the offsets are clamped
 * by the kernel as in kmx_query_seqs_dev (bad offsets miscount, never read outside the buffers)                          */
int kmx_count_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases);
/* filter and cap, then the build (= kmx_build_dev on the listing): the handle is READY; *n_listed (may be NULL) = n_total.
 * Nothing listed: what kmx_build_dev with n = 0 returns.  Outside a session: KMX_E_STATE                                  */
int kmx_count_finish(kmx_model *m, uint64_t *n_listed);
/* the listing the last finish built from (kept on the device until the next kmx_count_begin, build, or destroy): *n
 * entries; kmers[n * W] (packed, W = ceil(k/32)) and counts[n] (may be NULL) when kmers != NULL and capacity >= *n      */
int kmx_count_listing(kmx_model *m, uint64_t *kmers, uint32_t *counts, uint64_t capacity, uint64_t *n);
/* begin + count + finish on reads from files: a FASTQ or FASTA path (plain or gzip, detected from the content) or "@list",
 * a file of paths, one per line.  FASTQ records have their sequence on one line; FASTA records join their lines; a '\r'
 * at a line end is dropped.  A malformed or truncated record: KMX_E_IO naming the file and the record; a gzip stream that
 * ends early or is damaged: KMX_E_IO naming the file, also where the part that decodes ends on a whole record.  gzip needs
 * libz.so.1 at run time (opened with dlopen; plain input does not).                                                       */
int kmx_build_from_reads(kmx_model *m, int k, const char *input);

/* ---- unitigs: the compacted de Bruijn graph of a counted listing, on the device.  A sorted listing is an exact membership
 * structure (no tie-break, no false positives: unlike kmx_extend_seqs nothing here asks the model), and the maximal
 * non-branching paths of its graph are what an assembler calls unitigs.
 * Input: a listing of n packed k-mers (W = ceil(k/32) words each) with uint32 counts, strictly ascending as 2k-bit integers,
 * each k-mer canonical in the counting rule's sense (the numeric minimum of the forward word and its reverse complement, for
 * every k: not the model's k > 32 hashing quirk) -- what kmx_count_listing returns and what a KMC1-layout database lists -- and
 * a threshold thr (uint32).  k must be ODD, in [5, 63]: an even k has k-mers equal to their own reverse complement, where a
 * path can fold back onto itself (KMX_E_ARG).  n must be below 2^31 (KMX_E_ARG): oriented nodes are 32-bit words.
 *   Nodes: the listed k-mers with count >= thr; idx(u) is a node's index in the listing.  An oriented k-mer is a k-byte string
 *     x over ACGT whose canonical form canon(x) is a node.
 *   Degrees: succ(x) = { x[1:] + c : c in A, C, G, T and canon(x[1:] + c) is a node }, pred(x) = { c + x[:-1] : likewise }; a
 *     degree is the number of such c.  A neighbour that is x itself or rc(x) counts like any other.
 *   Links: x -> y is a link iff succ(x) = {y}, pred(y) = {x} and canon(y) != canon(x): a homopolymer's self-loop and a hairpin
 *     x -> rc(x) are edges but never links.  Links are symmetric under reverse complement (x -> y iff rc(y) -> rc(x)), and every
 *     oriented k-mer has at most one link in and one link out, so the 2 n oriented k-mers fall into disjoint paths and cycles
 *     that come in mirror pairs (P, rc(P)); for odd k, P != rc(P) and no component holds both orientations of a node.
 *   Unitigs: one per mirror pair.  A path of m >= 1 k-mers x_1 .. x_m (x_1 has no link in, x_m no link out): for m = 1 the
 *     representative is the canonical orientation; for m > 1, of P and rc(P) the one whose first node has the smaller listing
 *     index (the two end nodes are distinct).  A cycle of m >= 2 k-mers: the representative starts at the cycle's node of
 *     smallest listing index, in its canonical orientation, follows the links once round, and is spelled open with
 *     circular = 1.  The string is x_1 followed by the last byte of each of x_2 .. x_m: m + k - 1 bytes of uppercase ACGT.
 *   Order: ascending listing index of canon(x_1).  Every node lies in exactly one unitig, so the order is total.
 * Every field of the record is an integer count, sum, minimum or maximum, and the result is a function of (listing, thr) alone:
 * byte-identical across runs and variants.
 * Out of scope: even k, n >= 2^31, unsorted (KMC2-order) listings (sort them first), unitigs from the model's answers,
 * several GPUs, choosing thr.  The edges between unitigs: kmx_unitig_graph below; tip clipping, bubble popping and the
 * removal of islands: kmx_unitig_graph_clean below that.                                                                 */
typedef struct kmx_unitig {              /* one per unitig; 40 bytes, no padding */
	uint64_t n_kmers;                    /* m; the string has m + k - 1 bytes */
	uint64_t sum_count;                  /* over its nodes, of the listing's counts */
	uint32_t min_count, max_count;       /* capped at cs when the listing is a session's */
	uint64_t first_node;                 /* idx(canon(x_1)) */
	uint8_t  circular;
	uint8_t  n_pred;                     /* |pred(x_1)| */
	uint8_t  n_succ;                     /* |succ(x_m)|; both are 1 for a cycle */
	uint8_t  first_fwd;                  /* 1 iff x_1 is canonical */
	uint8_t  reserved[4];                /* 0 */
} kmx_unitig;
/* On DEVICE buffers d_kmers[n * W], d_counts[n], on the model's stream; needs no built model (like kmx_apply_edits_dev) and
 * leaves the model and a session's listing as they are.  d_seq_out[seq_capacity] and d_offsets_out[rec_capacity + 1] receive
 * the unitigs in the layout of kmx_query_seqs (unitig u = d_seq_out[offsets[u] .. offsets[u + 1]), offsets[0] = 0), d_rec
 * [rec_capacity] the records (may be NULL); *n_unitigs and *n_bases_out, on the HOST, the number of unitigs and of their bytes.
 * d_seq_out == NULL: the sizing call, only the two counts are returned.  A capacity too small: KMX_E_RANGE, both counts are
 * what is needed, nothing is written; rec_capacity = the nodes and seq_capacity = nodes * k always suffice.  The listing is
 * validated on the device by the first pass: not strictly ascending, not canonical or wider than 2k bits is KMX_E_ARG, and no
 * access ever leaves the buffers.  n == 0 or no count reaches thr: KMX_OK, 0 unitigs, offsets_out[0] = 0.  KMX_E_NOMEM leaves
 * the handle usable and the listing intact.  Device memory, kept on the handle between calls: 61 to 65 bytes per listing
 * entry (4 to 8 for the bucket index over the top bits, 2^ceil(log2 n) words; 9 for degrees and only-neighbours; 32 for the
 * two copies of pointer and rank of both orientations and 16 for the two copies of their running minimum, which the marks and
 * their scan reuse), plus the scan's scratch.  The host variants add what they stage there: the uploaded listing
 * (n (8 W + 4) bytes, kmx_unitigs only) and the output (n_bases + 8 (n_unitigs + 1) + 40 n_unitigs bytes).  It waits
 * for the stream once per doubling round (at most 2 ceil(log2 n) + 2, the second half only when the graph has a cycle), once
 * for the validation and once for the counts, and returns with the emit enqueued.  Build-class calls (see the threading
 * note of kmx_query_packed).                                                                                              */
int kmx_unitigs_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr,
                    char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out /* [rec_capacity + 1] */, kmx_unitig *d_rec /* or NULL */, uint64_t rec_capacity,
                    uint64_t *n_unitigs /* HOST */, uint64_t *n_bases_out /* HOST */);
/* the same on HOST buffers (seq_out == NULL: the sizing call); the listing is uploaded (n * (8 W + 4) bytes more) and the
 * call returns when the output is complete                                                                               */
int kmx_unitigs(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr,
                char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out /* [rec_capacity + 1] */, kmx_unitig *rec /* or NULL */, uint64_t rec_capacity,
                uint64_t *n_unitigs, uint64_t *n_bases_out);
/* the same two on the listing the last kmx_count_finish kept, read where it lies (no copy): KMX_E_STATE when there is none,
 * KMX_E_ARG for an even session k                                                                                        */
int kmx_count_unitigs(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity,
                      uint64_t *n_unitigs, uint64_t *n_bases_out);
int kmx_count_unitigs_dev(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity,
                          uint64_t *n_unitigs /* HOST */, uint64_t *n_bases_out /* HOST */);
/* where the last of these calls on the handle spent its time, measured only under kmx_set_profile(m, 1) (every phase then
 * waits for the stream): seconds[4] = adjacency (with the validation and the index), links, ranking, emit (with the marks and
 * their scan); *rounds = its doubling rounds (counted always)                                                             */
int kmx_unitigs_last_phases(kmx_model *m, double *seconds /* [4] */, uint64_t *rounds);

/* ---- the unitig graph: the edges between the unitigs of the rule above, as CSR.  Take the result of the unitig rule for
 * (listing, thr): U unitigs, strings s_u of m_u k-mers each.
 *   Oriented unitig o = 2 u + d: d = 0 is s_u as emitted, d = 1 its reverse complement.  first(o) and last(o) are the first
 *     and the last k bytes of the oriented string.
 *   Edges out of o: for c in A, C, G, T in that order, y = last(o)[1:] + c; if canon(y) is a node there is an edge o -> o',
 *     where o' is the one oriented unitig with first(o') = y.  It exists (an edge that leaves a unitig's end is no link, so y
 *     has no link in and starts its oriented path) and is unique (for odd k every oriented k-mer lies in exactly one oriented
 *     unitig, at one place).  A homopolymer's self-loop gives o -> o, a hairpin 2u -> 2u+1 or 2u+1 -> 2u, and a circular unitig
 *     has exactly 2u -> 2u and 2u+1 -> 2u+1: the closing link, once per orientation.
 *   Every edge overlaps by k - 1 bytes: the last k - 1 bytes of the source's oriented string are the first k - 1 of the target's.
 * So out-degree(2u) = n_succ and out-degree(2u+1) = n_pred of record u; n_links is the sum of n_pred + n_succ over the records;
 * a -> b is an edge iff (b ^ 1) -> (a ^ 1) is; no edge appears twice; and the oriented edges of the node graph are exactly the
 * links inside unitigs plus the edges reported here.
 * Output: link_offsets[2 U + 1] (uint64, link_offsets[0] = 0) and links[n_links] (uint32, the target o'; U <= n < 2^31): the
 * edges of o are links[link_offsets[o] .. link_offsets[o + 1]), in the order of c.  A function of (listing, thr) alone,
 * byte-identical across runs and variants.
 * The four calls take the arguments of their kmx_*unitigs* twins in the same order, with link_offsets [2 rec_capacity + 1],
 * links [link_capacity] and link_capacity in front of the counts and *n_links (HOST) behind them; strings, offsets and records
 * are byte for byte the twin's.  seq_out == NULL: the sizing call, the three counts only.  A capacity too small, link_capacity
 * included: KMX_E_RANGE, all three counts are what is needed, nothing is written; link_capacity = 8 * nodes always suffices.
 * link_offsets == NULL or links == NULL with seq_out != NULL: KMX_E_ARG (also where n_links is 0).  n == 0 or no count reaches
 * thr: KMX_OK, link_offsets[0] = 0, *n_links = 0.  The other argument checks, KMX_E_STATE, KMX_E_NOMEM (the handle stays usable,
 * the listing intact), the build-class threading note and the waits are the twins': the number of links reaches the host in the
 * wait that fetches the other two counts, so there is no wait more.  Device memory: none beside the twin's per listing entry
 * (the link counts and their scan, 16 bytes per entry, live in the copy of the rank state that the marks have left free, the
 * head and tail entry of every unitig in the two arrays of only-neighbours, which nothing reads once the ranks stand).  The
 * host variants stage 8 (2 U + 1) + 4 n_links bytes more for the two arrays.
 * Out of scope: what the unitig rule leaves out.  Tip clipping and bubble popping start from these edges:
 * kmx_unitig_graph_clean below.                                                                                          */
int kmx_unitig_graph_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr,
                         char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out /* [rec_capacity + 1] */, kmx_unitig *d_rec /* or NULL */, uint64_t rec_capacity,
                         uint64_t *d_link_offsets /* [2 * rec_capacity + 1] */, uint32_t *d_links, uint64_t link_capacity,
                         uint64_t *n_unitigs /* HOST */, uint64_t *n_bases_out /* HOST */, uint64_t *n_links /* HOST */);
int kmx_unitig_graph(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr,
                     char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out /* [rec_capacity + 1] */, kmx_unitig *rec /* or NULL */, uint64_t rec_capacity,
                     uint64_t *link_offsets /* [2 * rec_capacity + 1] */, uint32_t *links, uint64_t link_capacity,
                     uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links);
int kmx_count_unitig_graph(kmx_model *m, uint32_t thr, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec, uint64_t rec_capacity,
                           uint64_t *link_offsets /* [2 * rec_capacity + 1] */, uint32_t *links, uint64_t link_capacity,
                           uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links);
int kmx_count_unitig_graph_dev(kmx_model *m, uint32_t thr, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out, kmx_unitig *d_rec, uint64_t rec_capacity,
                               uint64_t *d_link_offsets /* [2 * rec_capacity + 1] */, uint32_t *d_links, uint64_t link_capacity,
                               uint64_t *n_unitigs /* HOST */, uint64_t *n_bases_out /* HOST */, uint64_t *n_links /* HOST */);
/* kmx_unitigs_last_phases with a fifth figure: seconds[4] = the edges between unitigs (their counts at the heads and the scan,
 * the links kernel), 0 after a call that asked for none.  kmx_unitigs_last_phases reports its four as before, after old and
 * new calls alike.                                                                                                        */
int kmx_unitig_graph_last_phases(kmx_model *m, double *seconds /* [5] */, uint64_t *rounds);

/* ---- cleaning the unitig graph: tips clipped, bubbles popped, islands dropped, round by round until nothing goes.  The input
 * is that of kmx_unitig_graph (a strictly ascending canonical listing, odd k in [5, 63], n < 2^31) with
 *   thr >= 1 (thr = 0 is KMX_E_ARG: a removed node is one whose count lies below thr);
 *   ops, a non-empty subset of KMX_CLEAN_TIPS | KMX_CLEAN_ISLANDS | KMX_CLEAN_BUBBLES;
 *   max_tip >= 1 and max_bubble >= 1, in k-mers; max_rounds in [1, KMX_CLEAN_MAX_ROUNDS]     (KMX_E_ARG otherwise).
 * N_0 is the set of nodes of (listing, thr).  For round r = 1 .. max_rounds: G_r is the unitig graph of the node set N_(r-1) (U
 * unitigs, their records, out[o] = the row of oriented unitig o), in[t] = { s ^ 1 : s in out[t ^ 1] }, and R_r the set of
 * unitigs removed this round.  R_r empty: stop, converged = 1, the output is G_r.  Otherwise N_r = N_(r-1) minus every node of
 * a unitig in R_r.  If round max_rounds still removed something, the output is the unitig graph of N_max_rounds and
 * converged = 0.  A non-circular unitig u falls into at most one class, read from its record alone:
 *   Island: n_pred == 0 && n_succ == 0 && n_kmers <= max_tip.  Removed iff ops & ISLANDS.
 *   Short tip: short_tip[u] = !circular && n_kmers <= max_tip && (n_pred == 0) != (n_succ == 0).  Let o = 2u if n_succ > 0, else
 *     2u + 1: the orientation that leaves through the attached end.  With ops & TIPS, u is removed iff EVERY t in out[o] has
 *     some s in in[t] with s >> 1 != u and tip_beats[s >> 1, u], where tip_beats[w, u] holds iff !short_tip[w], or the pair
 *     (n_kmers, sum_count) of w is lexicographically greater than u's, or the pairs are equal and w < u.
 *   Arm: arm[u] = !circular && n_kmers <= max_bubble && n_pred == 1 && n_succ == 1.  Let b be the one entry of out[2u] and a the
 *     one entry of out[2u + 1].  If b >> 1 == u or a >> 1 == u (a self-loop or a hairpin), u is not removed.  With
 *     ops & BUBBLES, u is removed iff some p in in[b] satisfies all of: v = p >> 1 != u, arm[v], out[p] == {b},
 *     out[p ^ 1] == {a}, and the pair (sum_count, n_kmers) of v is lexicographically greater than u's, or equal and v < u.
 * Circular unitigs and unitigs longer than the caps are never removed.  Every decision of a round is taken on G_r alone, so the
 * result is a function of (listing, thr, parameters): byte-identical across runs and variants.  Consequences:
 *   1. No junction is orphaned: if t is an oriented unitig of a unitig that survives round r and in[t] was not empty, in[t]
 *      still holds a survivor (the best-keyed competitor at a junction is never removed).
 *   2. The uncleaned capacities always suffice: links between surviving nodes stay links, so unitigs only merge; U, the byte
 *      count and n_links of the output never exceed those of kmx_unitig_graph on the same (listing, thr).
 *   3. Original coordinates: first_node and all records are in the ORIGINAL listing's indices; sum / min / max_count are the
 *      original counts.
 *   4. A no-op is exact: with nothing to remove the output is byte for byte that of kmx_unitig_graph, rounds_run = 1,
 *      converged = 1.
 * Out of scope: bubbles whose arms hold more than one unitig; mean-coverage criteria; several GPUs; choosing thr and the caps.
 * Low-coverage edge removal by the reads per link, with a coverage ratio: kmx_unitig_contigs below the walks.              */
#define KMX_CLEAN_TIPS        1
#define KMX_CLEAN_ISLANDS     2
#define KMX_CLEAN_BUBBLES     4
#define KMX_CLEAN_MAX_ROUNDS 64
typedef struct kmx_clean_params { uint32_t ops, max_tip, max_bubble, max_rounds; } kmx_clean_params;          /* 16 bytes */
typedef struct kmx_clean_stats  { uint64_t rounds_run, converged, n_tips, n_islands, n_bubbles,
                                  n_kmers_removed, n_unitigs_before, n_links_before; } kmx_clean_stats;       /* 64 bytes */
/* The four calls take the arguments of their kmx_*unitig_graph* twins in the same order, with params (HOST) directly behind thr
 * and, at the end, removed [n] or NULL (a DEVICE buffer in the _dev forms) and stats (HOST) or NULL.  removed[i] is the round
 * (1-based) that removed entry i, 0 for an entry that survives or never was a node.  rounds_run counts the round that found
 * nothing; n_unitigs_before / n_links_before are the counts of kmx_unitig_graph on the same (listing, thr).  The sizing call
 * (seq_out == NULL; the counts are those of the CLEANED graph), KMX_E_RANGE, KMX_E_ARG, KMX_E_STATE, KMX_E_NOMEM, the
 * build-class threading note and "nothing written on a short capacity" are the twins'; stats and the three counts are complete
 * on KMX_E_RANGE, and removed, where given, counts as written (also by the sizing call).  The caller's counts, a session's
 * listing and the model are never written: a following kmx_count_unitig_graph at the same thr returns what it did before.
 * How it runs: a working copy of the counts (4 n bytes, kept on the handle) in which removal writes 0, so a round is the
 * construction of the twin on (k-mers, working counts, thr), its records, link_offsets and links written into the handle's
 * staging buffers (40 U + 8 (2 U + 1) + 8 (U + 1) + 4 n_links bytes, in the _dev forms too; no strings), one kernel that takes
 * the verdicts (8 lanes per unitig: its record, its two rows, the rows of at most 4 targets, the records of at most 16
 * competitors; U verdict bytes) and one per listing entry that zeroes the working counts.  Device memory beside the twin's:
 * these 4 n + U bytes and the staging; the host variants stage removed (n bytes) when it is asked for.  Waits: those of the
 * twin once per round, plus ONE per round for the round's four counters; the round that removes nothing is the final graph and
 * is emitted from the rank state that stands.  When round max_rounds still removed something the construction runs once more. */
int kmx_unitig_graph_clean_dev(kmx_model *m, int k, const uint64_t *d_kmers, const uint32_t *d_counts, uint64_t n, uint32_t thr, const kmx_clean_params *params /* HOST */,
                               char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out /* [rec_capacity + 1] */, kmx_unitig *d_rec /* or NULL */, uint64_t rec_capacity,
                               uint64_t *d_link_offsets /* [2 * rec_capacity + 1] */, uint32_t *d_links, uint64_t link_capacity,
                               uint64_t *n_unitigs /* HOST */, uint64_t *n_bases_out /* HOST */, uint64_t *n_links /* HOST */,
                               uint8_t *d_removed /* [n] or NULL */, kmx_clean_stats *stats /* HOST, or NULL */);
int kmx_unitig_graph_clean(kmx_model *m, int k, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t thr, const kmx_clean_params *params,
                           char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out /* [rec_capacity + 1] */, kmx_unitig *rec /* or NULL */, uint64_t rec_capacity,
                           uint64_t *link_offsets /* [2 * rec_capacity + 1] */, uint32_t *links, uint64_t link_capacity,
                           uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *removed /* [n] or NULL */, kmx_clean_stats *stats /* or NULL */);
int kmx_count_unitig_graph_clean(kmx_model *m, uint32_t thr, const kmx_clean_params *params, char *seq_out, uint64_t seq_capacity, uint64_t *offsets_out, kmx_unitig *rec,
                                 uint64_t rec_capacity, uint64_t *link_offsets /* [2 * rec_capacity + 1] */, uint32_t *links, uint64_t link_capacity,
                                 uint64_t *n_unitigs, uint64_t *n_bases_out, uint64_t *n_links, uint8_t *removed /* [n] or NULL */, kmx_clean_stats *stats /* or NULL */);
int kmx_count_unitig_graph_clean_dev(kmx_model *m, uint32_t thr, const kmx_clean_params *params /* HOST */, char *d_seq_out, uint64_t seq_capacity, uint64_t *d_offsets_out,
                                     kmx_unitig *d_rec, uint64_t rec_capacity, uint64_t *d_link_offsets /* [2 * rec_capacity + 1] */, uint32_t *d_links, uint64_t link_capacity,
                                     uint64_t *n_unitigs /* HOST */, uint64_t *n_bases_out /* HOST */, uint64_t *n_links /* HOST */,
                                     uint8_t *d_removed /* [n] or NULL */, kmx_clean_stats *stats /* HOST, or NULL */);
/* the five figures of kmx_unitig_graph_last_phases summed over the rounds of the last cleaning call on the handle (a round's
 * emit is the one into the staging buffers; the emit of the final graph into the caller's buffers is not added), then
 * seconds[5] = the decisions and the removal; *rounds = its doubling rounds, summed likewise.  After a cleaning call the two
 * older phase calls report these sums.                                                                                    */
int kmx_unitig_clean_last_phases(kmx_model *m, double *seconds /* [6] */, uint64_t *rounds);

/* ---- mapping reads onto the unitigs: where every window of a read lies in the graph, as runs along oriented unitigs.
 * The index.  Input: a listing of n packed canonical k-mers, strictly ascending, odd k in [5, 63], n < 2^31 (the conditions of
 *   kmx_unitigs; counts are not needed), and a set of U sequences in the layout of kmx_query_seqs (useq, uoffsets); sequence u
 *   has m_u = len_u - k + 1 >= 1 windows.  Window j of sequence u, the k bytes y, gives entry idx(canon(y)) the PLACE (u, j, f),
 *   f = 0 iff y is canonical.  The set is valid iff every byte is uppercase ACGT, every window is a listed k-mer, and no entry
 *   receives two places; anything else is KMX_E_ARG, found on the device (a compare-and-swap from "no place" that raises an
 *   error word) without ever leaving the buffers.  An entry that receives no place has none: a thresholded-out or cleaned-away
 *   k-mer.  The output of every kmx_*unitigs*, kmx_*unitig_graph* and kmx_*unitig_graph_clean* call on that listing is a valid set.
 * A window.  Reads are in the layout of kmx_query_seqs; bases follow the COUNTING rule (ACGT and acgt are bases, every other
 *   byte is not; windows never span two sequences).  The window x at flat position p is MAPPED iff its k bytes are bases and
 *   canon(x) has a place (u, j, f).  With d = f ^ (x is not canonical) it lies on oriented unitig o = 2 u + d, the o of
 *   kmx_unitig_graph, at offset off = j for d = 0 and m_u - 1 - j for d = 1: one base further along the read inside a unitig is
 *   off + 1 in either orientation.
 * Segments.  Window p STARTS a segment iff it is mapped and it is the first window of its read, or p - 1 is unmapped, or
 *   o(p - 1) != o(p), or off(p - 1) + 1 != off(p); it ENDS one under the mirror condition on p + 1.  A segment is the record below;
 *   segments are listed in ascending pos, and seg_offsets[n_seqs + 1] is their CSR by read.  Going once round a circular unitig
 *   starts a new segment at off = 0.
 * Every decision looks at one window and its neighbour, so the list is a function of (listing, unitig set, reads) alone:
 * byte-identical across runs, variants and piece sizes.  Consequences:
 *   (a) for every segment, the bytes [off, off + n_windows + k - 1) of the oriented unitig string are the read's bytes
 *       [pos, pos + n_windows + k - 1), upper-cased;
 *   (b) with the unitig set of kmx_count_unitigs(thr = 1) of a session with ci = 1 whose counts stay below cs, and the reads
 *       that were counted: n_mapped is the number of counted windows of every read, and hits[u] == rec[u].sum_count;
 *   (c) on a cleaned graph, a window whose k-mer is listed is unmapped exactly when its entry has removed[i] != 0 or a count
 *       below thr.
 * Out of scope: even k; mismatches or indels between read and graph (a read with an error maps on both sides of it, with a
 * gap of unmapped windows between: polish first, or let kmx_unitig_walk_segs below bridge the gap); paired reads; several
 * GPUs.                                                                                                                   */
typedef struct kmx_map_segment {         /* 24 bytes, no padding */
	uint64_t pos;                        /* flat position of its first window */
	uint32_t n_windows;
	uint32_t o;                          /* 2 u + d */
	uint32_t off;                        /* of the window at pos */
	uint32_t reserved;                   /* 0 */
} kmx_map_segment;
typedef struct kmx_seq_map {             /* one per read; 64 bytes */
	uint64_t n_windows;                  /* max(len - k + 1, 0) */
	uint64_t n_mapped;
	uint64_t n_segments;
	uint64_t n_gaps;                     /* mapped windows whose predecessor in the read exists and is unmapped, the first mapped window not counted */
	uint64_t first_mapped, last_mapped;  /* window indices inside the read; both n_windows when nothing maps */
	uint64_t longest;                    /* the largest n_windows of its segments, 0 if none */
	uint64_t reserved;                   /* 0 */
} kmx_seq_map;
/* A session on the handle, in the style of kmx_count_begin / _seqs / _finish; it needs no built model.  begin borrows the
 * caller's DEVICE listing d_kmers[n * W], which must stay valid and unchanged until kmx_unitig_map_end; the unitig set is read
 * during begin only.  It builds a bucket index of the listing (4 to 8 bytes per entry), the place table (8 bytes per entry:
 * u << 32 | f << 31 | j, all ones for none) and m_u (4 U bytes), and waits once, for the error words.  A begin inside a session
 * ends that session first; a begin that fails leaves none.  Build-class calls (see the threading note of kmx_query_packed). */
int kmx_unitig_map_begin_dev(kmx_model *m, int k, const uint64_t *d_kmers, uint64_t n, const char *d_useq, const uint64_t *d_uoffsets /* [n_unitigs + 1] */,
                             uint64_t n_unitigs, uint64_t n_ubases);
/* the same on HOST buffers: the listing is uploaded and the session keeps its own copy (uoffsets are checked on the host) */
int kmx_unitig_map_begin(kmx_model *m, int k, const uint64_t *kmers, uint64_t n, const char *useq, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs);
/* the same two on the listing the last kmx_count_finish kept, read where it lies: KMX_E_STATE when there is none, KMX_E_ARG for
 * an even session k.  Whatever drops that listing (kmx_count_begin, a build from other data, kmx_destroy) ends the session.   */
int kmx_count_unitig_map_begin(kmx_model *m, const char *useq, const uint64_t *uoffsets, uint64_t n_unitigs);
int kmx_count_unitig_map_begin_dev(kmx_model *m, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases);
/* One batch of reads.  segs[capacity] receives the segments, *n_segs (HOST in both forms) their number, seg_offsets
 * [n_seqs + 1] the CSR, rec[n_seqs] the records (or NULL), and hits[n_unitigs] (or NULL) is ADDED to: hits[u] += the mapped
 * windows on unitig u in either orientation, so a caller accumulates over batches and zeroes the array itself.  segs == NULL:
 * the sizing call.  More segments than capacity: KMX_E_RANGE; *n_segs is the number needed, seg_offsets, records and hits are
 * complete, the content of segs is unspecified and nothing is written at or behind segs[capacity]; capacity = n_bases always
 * suffices.  The host form checks the offsets (KMX_E_ARG); the _dev form clamps them where they are read, exactly as
 * kmx_query_seqs_dev does, so bad offsets give wrong segments and never an access outside the buffers.  Outside a session:
 * KMX_E_STATE.  KMX_E_NOMEM leaves the handle and the session usable.  n_seqs == 0: KMX_OK, nothing written.  Reads without
 * bases: empty records, all-zero seg_offsets.  Device memory beside the index: 20 bytes per window of a chunk of 2^22 windows
 * plus the scan's scratch, whatever n_bases is; the host form also stages its output there.  The _dev form enqueues everything
 * on the model's stream and waits once, for *n_segs; the host form sends the bases through the handle's pinned slots in pieces
 * of one chunk (so it shares them with the query calls: one such call at a time) and only segments, offsets, records and hits
 * come back.                                                                                                              */
int kmx_unitig_map_seqs(kmx_model *m, const char *seq, const uint64_t *offsets, uint64_t n_seqs, kmx_map_segment *segs /* or NULL */, uint64_t capacity, uint64_t *n_segs,
                        uint64_t *seg_offsets /* [n_seqs + 1] */, kmx_seq_map *rec /* or NULL */, uint64_t *hits /* [n_unitigs] or NULL */);
int kmx_unitig_map_seqs_dev(kmx_model *m, const char *d_seq, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t n_bases, kmx_map_segment *d_segs /* or NULL */, uint64_t capacity,
                            uint64_t *n_segs /* HOST */, uint64_t *d_seg_offsets /* [n_seqs + 1] */, kmx_seq_map *d_rec /* or NULL */, uint64_t *d_hits /* [n_unitigs] or NULL */);
/* ends the session and frees its index; KMX_E_STATE outside one */
int kmx_unitig_map_end(kmx_model *m);

/* ---- walks: the segments of every read threaded through the unitig graph.  A post-pass on what kmx_unitig_map_seqs[_dev]
 * wrote, inside the map session, which holds k, U and m_u; it reads no bases.
 * Input: the segments of a batch (segs[n_segs], seg_offsets[n_seqs + 1]) exactly as the map call wrote them; the CSR of the graph
 *   the session's unitig set came from (link_offsets[2 U + 1], links[n_links]; out[o] is the row of oriented unitig o); and
 *   kmx_walk_params, with max_indel in [0, 255] and reserved = 0 (KMX_E_ARG otherwise).
 * Joins.  For two consecutive segments A, B of one read, in signed 64-bit arithmetic: mA = m_(A.o >> 1),
 *   endA = A.off + A.n_windows - 1, g = B.pos - A.pos - A.n_windows (the unmapped windows between them), row = out[A.o].
 *   g == 0: the join is an EDGE iff endA == mA - 1, B.off == 0 and B.o occurs in row, at link index e; otherwise there is no join
 *     and n_unlinked counts it.
 *   1 <= g <= max_gap: it is INSIDE iff B.o == A.o, B.off > endA and |d| <= max_indel with d = (B.off - endA - 1) - g; else
 *     ACROSS iff B.o occurs in row, at link index e, and |d| <= max_indel with d = (mA - 1 - endA) + B.off - g; else there is no
 *     join and n_breaks counts it.  d is the number of path windows in the gap minus the number of read windows: a base the read
 *     lost gives d = +1, a surplus base d = -1, a substitution d = 0.
 *   g > max_gap or g < 0: no join, counted by n_breaks.
 * A WALK is a maximal chain of joined segments of one read.  A STEP is an oriented unitig of its path: one for the walk's first
 *   segment and one more for every EDGE or ACROSS join; INSIDE adds none.  Going round a circular unitig is an EDGE join o -> o.
 *   With max_gap = 0 only exact traversals join.
 * Every decision looks at one segment, its predecessor and one row of at most 4 entries, and all outputs are integer sums: a
 * function of (segments, CSR, m_u, parameters) alone, byte-identical across runs and variants.  Consequences:
 *   (a) with the CSR of the session's own graph n_unlinked is 0: two segments with g == 0 are neighbouring mapped windows, so
 *       their k-mers are joined by an oriented edge of the node graph, and "the oriented edges of the node graph are exactly the
 *       links inside unitigs plus the edges reported here" (the unitig graph above); a link inside a unitig does not start a
 *       segment, so the edge is a reported one, leaving the last window of A.o for the first of B.o;
 *   (b) a walk without INSIDE or ACROSS joins spells its read: the steps' oriented strings, concatenated with k - 1 bytes of
 *       overlap, hold the read's bytes [pos, pos + n_span + k - 1), upper-cased, from off_first on, and n_covered is that length;
 *   (c) the walks of the reverse complement of a read are the read's own, mirrored: in reverse order, steps reversed with o ^ 1,
 *       and every +1 of link_hits on the mirror edge (b ^ 1) -> (a ^ 1) of a -> b; link_hits counts the traversed edge only, the
 *       mirror edge is the caller's to add.
 * Out of scope: gaps that span a whole unitig (a bridge crosses at most one edge); comparing the bases inside a gap (a bridge
 * is accepted on its geometry alone); paired reads (kmx_unitig_pair_walks below places the two mates of a pair from these walks);
 * several GPUs.  What consumes link_hits: kmx_unitig_contigs below.                                                        */
typedef struct kmx_walk_params { uint32_t max_gap, max_indel, reserved[2]; } kmx_walk_params;                  /* 16 bytes */
typedef struct kmx_walk {                /* one per walk, in ascending pos; 80 bytes */
	uint64_t pos;                        /* flat position of its first window */
	uint64_t n_span;                     /* windows from its first to its last mapped window, inclusive */
	uint64_t n_mapped;                   /* the sum of its segments' n_windows */
	uint64_t n_covered;                  /* sum of (n_windows + k - 1) minus, per join, max(0, k - 1 - g): the read bases inside a mapped
	                                        window, which match the path by consequence (a) of the map; a lower bound of the matches */
	uint64_t first_seg, first_step;      /* its segments are segs[first_seg .. first_seg + n_segs), its steps steps[first_step .. + n_steps) */
	uint32_t n_segs, n_steps;
	uint32_t off_first;                  /* the offset of its first window in its first step */
	uint32_t off_last;                   /* the offset of its last window in its last step */
	uint32_t n_inside, n_across;
	int32_t indel;                       /* the sum of d over its joins */
	uint32_t reserved;                   /* 0 */
} kmx_walk;
typedef struct kmx_walk_stats { uint64_t n_walks, n_steps, n_edge, n_inside, n_across, n_unlinked, n_breaks, reserved; } kmx_walk_stats;   /* 64 bytes */
/* walks[walk_capacity] receives the walks, walk_offsets[n_seqs + 1] their CSR by read (walk_offsets[r] is the number of the walk
 * that starts at seg_offsets[r]), steps[step_capacity] the steps (the o of each), back to back in walk order, and link_hits
 * [n_links] (or NULL) is ADDED to: +1 at e for every EDGE and ACROSS join, so a caller accumulates over batches and zeroes the
 * array itself.  stats (HOST in both forms, required) receives the counts.  walks == NULL: the sizing call (steps is not read).
 * More walks than walk_capacity or more steps than step_capacity: KMX_E_RANGE; stats, walk_offsets and link_hits are complete,
 * the content of walks and steps is unspecified and nothing is written at or behind either capacity; n_segs always suffices for
 * both.  Outside a session: KMX_E_STATE.  KMX_E_NOMEM leaves the handle and the session usable.  n_seqs == 0: KMX_OK, all-zero
 * stats, nothing else written.  The host form checks seg_offsets (first 0, non-decreasing, last n_segs) and the CSR
 * (link_offsets[0] == 0, non-decreasing, link_offsets[2 U] == n_links, every links[e] < 2 U): KMX_E_ARG.  The _dev form reads
 * d_segs and d_seg_offsets where the map call left them and d_link_offsets and d_links where the graph call left them, and
 * clamps instead: seg_offsets into [0, n_segs], row bounds into [0, n_links], at most 4 entries of a row are read, and a segment
 * with o >= 2 U joins nothing and has no m_u looked up; bad input gives wrong walks, never an access outside the buffers.  It
 * enqueues everything on the model's stream and waits once, for the counts.  Device memory: 21 bytes per segment (a flag byte,
 * the join's d and overlap, the scanned pair of walk and step starts) plus the scan's scratch, kept on the handle between calls
 * until the session ends; the host form also stages its input and output there.                                           */
int kmx_unitig_walk_segs(kmx_model *m, const kmx_map_segment *segs, uint64_t n_segs, const uint64_t *seg_offsets /* [n_seqs + 1] */, uint64_t n_seqs,
                         const uint64_t *link_offsets /* [2 U + 1] */, const uint32_t *links, uint64_t n_links, const kmx_walk_params *params,
                         kmx_walk *walks /* or NULL */, uint64_t walk_capacity, uint64_t *walk_offsets /* [n_seqs + 1] */, uint32_t *steps, uint64_t step_capacity,
                         uint64_t *link_hits /* [n_links] or NULL */, kmx_walk_stats *stats);
int kmx_unitig_walk_segs_dev(kmx_model *m, const kmx_map_segment *d_segs, uint64_t n_segs, const uint64_t *d_seg_offsets /* [n_seqs + 1] */, uint64_t n_seqs,
                             const uint64_t *d_link_offsets /* [2 U + 1] */, const uint32_t *d_links, uint64_t n_links, const kmx_walk_params *params /* HOST */,
                             kmx_walk *d_walks /* or NULL */, uint64_t walk_capacity, uint64_t *d_walk_offsets /* [n_seqs + 1] */, uint32_t *d_steps, uint64_t step_capacity,
                             uint64_t *d_link_hits /* [n_links] or NULL */, kmx_walk_stats *stats /* HOST */);

/* ---- contigs: the unitigs merged along the edges the reads support.  A unitig ends at every branch of the k-mer graph; the
 * reads per edge that kmx_unitig_walk_segs accumulated tell the branches that reads cross from those they do not.  This call
 * drops the unsupported edges and merges unitigs along what has become the only way on.  The construction of the unitig rule one
 * level up: the items are the 2 U oriented unitigs, not the 2 n oriented k-mers.
 * Input: k, odd, in [5, 63]; a unitig set in the layout of kmx_query_seqs (useq, uoffsets[U + 1]; unitig u has
 *   m_u = len_u - k + 1 >= 1 k-mers; U < 2^31; bytes of uppercase ACGT, what every kmx_*unitig* call writes: they are not checked,
 *   a reverse step maps a byte b to b ^ 0x04 where b & 2 and to b ^ 0x15 otherwise, which complements ACGT); optionally its
 *   records urec[U] (only sum_count, min_count and max_count are read); the CSR of its graph (link_offsets[2 U + 1],
 *   links[n_links]; out[o] is the row of oriented unitig o = 2 u + d, at most 4 entries); link_hits[n_links] as
 *   kmx_unitig_walk_segs accumulated it; and kmx_contig_params, ratio in [0, 65536], reserved = 0.
 *   Support.  The mirror of edge e = (a -> b) is mir(e), the entry a ^ 1 of out[b ^ 1].  sup(e) = link_hits[e] + link_hits[mir(e)],
 *     modulo 2^64 (hits below 2^63 are exact); a self-mirror edge (a hairpin a -> a ^ 1, mir(e) = e) has sup(e) = link_hits[e],
 *     counted once.  sup is symmetric under mir by construction: the addition consequence (c) of the walks leaves to the caller.
 *   Kept edges.  best(o) = the largest sup over ALL of out[o], 0 for an empty row.  e = (a -> b) is below_min iff
 *     sup(e) < min_reads; otherwise below_ratio iff ratio > 0 and (sup(e) * ratio < best(a) or sup(e) * ratio < best(b ^ 1)), the
 *     product taken in 128 bits; otherwise KEPT.  outK[o] is the kept part of out[o], in row order, and
 *     inK[t] = { s ^ 1 : s in outK[t ^ 1] }.  best(b ^ 1) is the largest support of an edge INTO b, so both tests are the same
 *     under mir and kept is symmetric.
 *   Chain links.  o -> t is a chain link iff outK[o] = {t}, inK[t] = {o} and t != o ^ 1.  A kept hairpin is never one; a kept
 *     self-loop o -> o with nothing else kept at either side IS one, a cycle of one step.  Every oriented unitig has at most one
 *     chain link in and one out, and o -> t iff (t ^ 1) -> (o ^ 1), so the 2 U oriented unitigs fall into paths and cycles that
 *     come in mirror pairs.  No component holds both orientations of a unitig: the mirror maps such a path onto itself end for
 *     end, so its middle would be a link o -> o ^ 1 (excluded) or a unitig equal to its own mirror (o != o ^ 1); on a cycle the
 *     mirror is a reflection, which fixes a step or a link, the same two impossibilities.
 *   Contigs: one per mirror pair.  A path o_1 .. o_s: for s = 1 the representative is d = 0; otherwise, of P and its mirror, the
 *     one whose first step has the smaller unitig index (the two first steps are the two ends: distinct unitigs).  A cycle: it
 *     starts at its smallest unitig in orientation d = 0, follows the chain links once round and is spelled open with
 *     circular = 1.  The string is the oriented string of o_1 followed by each later step's oriented string without its first
 *     k - 1 bytes; a later step never rewrites the overlap, so the bytes are a function of the input even for a CSR whose
 *     overlaps do not hold.  Contigs come in ascending unitig index of the first step; every unitig lies in exactly one, in one
 *     orientation.
 * Output.  The input's sizes always suffice, so there is no sizing call and no KMX_E_RANGE.  cseq[n_ubases] and coffsets[U + 1] in
 *   the layout of kmx_query_seqs (C + 1 offsets are written); crec[U], the records below (C are written); steps[U], the o of
 *   every step, back to back in contig order; place[U]: unitig u lies in contig oc >> 1, oc & 1 is 1 iff its step is 2 u + 1, and
 *   off is the k-mer offset of that step's first window in the contig (modulo 2^32), which turns the map's segments and the
 *   walks' steps into contig coordinates.  The contig graph: clink_offsets[2 U + 1] (2 C + 1 are written), clinks[n_links] and
 *   csupport[n_links]: the edges out of oriented contig oc = 2 c + d are the kept edges of its LAST step (o_s for d = 0, o_1 ^ 1
 *   for d = 1), in row order; the target is the oriented contig whose first step is that entry, and csupport[e] the edge's sup.
 *   Such a contig exists: a kept edge o -> t that is no chain link has |outK[o]| > 1, |inK[t]| > 1 or t = o ^ 1, and in each case
 *   t has no chain link in (for the first two because a chain link into t needs inK[t] to be its one source with that source's
 *   one kept edge; for a hairpin because inK[o ^ 1] = {o} would make it the excluded link), so t starts its oriented path.  A
 *   cycle has exactly 2c -> 2c and 2c+1 -> 2c+1: the unitig graph's convention.  On the HOST: *n_contigs, *n_cbases, *n_clinks and
 *   kmx_contig_stats.  Everything is an integer sum, count, minimum or maximum and a function of the input alone: byte-identical
 *   across runs and variants.
 * Consequences:
 *   (a) a no-op is exact: on a graph that kmx_*unitig_graph* returned, with min_reads = 0 and ratio = 0, every contig is one
 *       unitig; cseq, coffsets, clink_offsets and clinks are byte for byte the input's; n_kmers, the counts, n_pred and n_succ
 *       are the unitig record's, and so is circular except for an isolated unitig whose one edge is its own self-loop o -> o (a
 *       run of one base that nothing else touches): no circular unitig, since a self-loop of the node graph is never a link, but
 *       a cycle of one step here.  n_chain counts the closing links of these and of the circular unitigs, nothing else;
 *   (b) a contig is a path of the node graph: when the overlaps hold, every window of a contig is a k-mer of exactly one unitig
 *       and no k-mer appears twice, so the contig set is a valid set for kmx_unitig_map_begin on the same listing;
 *   (c) mirror invariance: adding every edge's hits on its mirror instead changes nothing;
 *   (d) place inverts steps; the n_steps sum to U, the n_kmers to the sum of m_u, and n_cbases = that sum + C (k - 1).
 * Repeats shorter than a read: kmx_unitig_walk_through and kmx_unitig_resolve below, in front of this call.
 * Out of scope: iterating with a re-map;
 * paired reads, beyond adding the pair_hits of kmx_unitig_pair_walks to link_hits; even k; several GPUs; choosing min_reads and
 * ratio.                                                                                                                   */
typedef struct kmx_contig_params { uint64_t min_reads; uint32_t ratio; uint32_t reserved; } kmx_contig_params;          /* 16 bytes */
typedef struct kmx_contig {              /* one per contig; 64 bytes, no padding */
	uint64_t n_kmers;                    /* the sum of m_u over its steps; the string has n_kmers + k - 1 bytes */
	uint64_t sum_count;                  /* from urec; 0 when urec is NULL */
	uint32_t min_count, max_count;       /* from urec; 0 when urec is NULL */
	uint64_t first_step;                 /* its steps are steps[first_step .. first_step + n_steps) */
	uint32_t n_steps;
	uint8_t  circular;
	uint8_t  n_pred;                     /* |inK[o_1]|; 1 for a cycle */
	uint8_t  n_succ;                     /* |outK[o_s]|; 1 for a cycle */
	uint8_t  reserved;                   /* 0 */
	uint64_t min_support, sum_support;   /* over its chain links, the closing link of a cycle included; 0 when it has none */
	uint64_t reserved2;                  /* 0 */
} kmx_contig;
typedef struct kmx_contig_place { uint32_t oc; uint32_t off; } kmx_contig_place;                                         /* 8 bytes */
typedef struct kmx_contig_stats { uint64_t n_links, n_kept, n_below_min, n_below_ratio, n_chain     /* oriented edges, each */,
                                  n_contigs, n_circular, n_multi /* contigs of more than one step */; } kmx_contig_stats;    /* 64 bytes */
/* On HOST buffers.  Needs no built model and no session (like kmx_apply_edits_dev); it runs on the model's stream and is a
 * build-class call (see the threading note of kmx_query_packed).  urec may be NULL; every other buffer is required, also where a
 * count is 0 (with U == 0 only the two offset arrays, the three counts and stats).  KMX_E_ARG before anything runs: an even or
 * out-of-range k, U >= 2^31, ratio > 65536, reserved != 0, a NULL required buffer, an output that overlaps an input or another
 * output; uoffsets whose first entry is not 0, that decrease, or that give a unitig fewer than k bytes; a CSR that
 * kmx_unitig_walk_segs would refuse (link_offsets[0] != 0, decreasing, link_offsets[2 U] != n_links, a links[e] >= 2 U), a row
 * longer than 4, an edge without its mirror.  U == 0: KMX_OK, coffsets[0] = clink_offsets[0] = 0, all counts zero.
 * KMX_E_NOMEM leaves the handle usable.  The call returns when the output is complete.                                      */
int kmx_unitig_contigs(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const kmx_unitig *urec /* or NULL */,
                       const uint64_t *link_offsets /* [2 U + 1] */, const uint32_t *links, uint64_t n_links, const uint64_t *link_hits /* [n_links] */,
                       const kmx_contig_params *params, char *cseq /* [n_ubases] */, uint64_t *coffsets /* [U + 1] */, kmx_contig *crec /* [U] */,
                       uint32_t *steps /* [U] */, kmx_contig_place *place /* [U] */, uint64_t *clink_offsets /* [2 U + 1] */, uint32_t *clinks /* [n_links] */,
                       uint64_t *csupport /* [n_links] */, uint64_t *n_contigs, uint64_t *n_cbases, uint64_t *n_clinks, kmx_contig_stats *stats);
/* The same on DEVICE buffers, read where the graph, map and walk calls left them; params, the three counts and stats are on the
 * HOST.  It checks k, U, the parameters, NULL and overlap, and validates nothing else on the host; the kernels clamp instead:
 * uoffsets into [0, n_ubases] (a unitig whose clamped bounds decrease has no bytes, one shorter than k no k-mers); row bounds
 * into [0, n_links]; at most 4 entries of a row are read; a target >= 2 U is no edge and is not counted; an edge whose mirror is
 * not found has sup = link_hits[e]; and a chain link o -> t additionally requires that the mirror side agrees
 * (outK[t ^ 1] = {o ^ 1}), so the links are symmetric whatever the CSR and the argument above holds.  Every store is checked
 * against U, n_ubases or n_links.  Bad device input gives wrong contigs; it never gives an access outside a buffer, and never
 * more than the bounded number of launches: ceil(log2 2U) + 1 doubling rounds, the cut, and as many again.
 * It waits for the stream once per doubling round (a word says whether anything moved; the rounds behind the cut run only when
 * there is a cycle), as the unitig construction does, and once for the counts, and returns with nothing left in flight.  Device
 * memory, kept on the handle between calls through the owning types of hip_owned.h: 195 bytes per unitig (2 x 32 for the two
 * copies of pointer, step rank and k-mer rank of both orientations, whose spare copy the marks reuse; 2 x 8 for the two copies
 * of the running minimum; 24 for the scanned marks; 2 x 21 for best, the only kept target, its support and the kept count of both
 * orientations; 1 for the cycle flag; 8 for where a unitig's bytes go; 2 x 16 for the end counts and their scan; 2 x 4 for the
 * last step of both oriented contigs) and 9 bytes per link (its support and its verdict), plus the scan's scratch.  The host
 * form also stages its input and output there.                                                                             */
int kmx_unitig_contigs_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, uint64_t n_ubases,
                           const kmx_unitig *d_urec /* or NULL */, const uint64_t *d_link_offsets /* [2 U + 1] */, const uint32_t *d_links, uint64_t n_links,
                           const uint64_t *d_link_hits /* [n_links] */, const kmx_contig_params *params /* HOST */, char *d_cseq /* [n_ubases] */,
                           uint64_t *d_coffsets /* [U + 1] */, kmx_contig *d_crec /* [U] */, uint32_t *d_steps /* [U] */, kmx_contig_place *d_place /* [U] */,
                           uint64_t *d_clink_offsets /* [2 U + 1] */, uint32_t *d_clinks /* [n_links] */, uint64_t *d_csupport /* [n_links] */,
                           uint64_t *n_contigs /* HOST */, uint64_t *n_cbases /* HOST */, uint64_t *n_clinks /* HOST */, kmx_contig_stats *stats /* HOST */);
/* where the last of these two calls on the handle spent its time, measured only under kmx_set_profile(m, 1) (every phase then
 * waits for the stream): seconds[5] = supports and verdicts, ranking (links, rounds, cut), marks and their scan, records with
 * steps, places and the contig graph, the bytes; *rounds = its doubling rounds (counted always)                              */
int kmx_unitig_contigs_last_phases(kmx_model *m, double *seconds /* [5] */, uint64_t *rounds);

/* ---- through hits: the reads per (way in, way out) of every unitig.  link_hits judges single edges; a walk of three or more
 * steps also says which way IN to a unitig goes with which way OUT, the evidence a repeat shorter than a read is resolved from.
 * This call counts it; kmx_unitig_resolve below consumes it.
 * Notation as above: U unitigs, oriented unitig o = 2 u + d, out[o] the CSR row (at most 4 entries).  For unitig u the RIGHT row
 *   is R = out[2 u] and the LEFT row is L = out[2 u + 1]; entry a of L is "way in number a" when u is read forward: the edge
 *   (L[a] ^ 1) -> 2 u.
 * Input: the walks and steps exactly as kmx_unitig_walk_segs[_dev] wrote them, walks[n_walks] (only first_step and n_steps are
 *   read) and steps[n_steps]; the CSR those walks were made with (link_offsets[2 U + 1], links[n_links]); and U.
 * Output: through[16 U], which is ADDED to, like link_hits: the caller zeroes it and accumulates over batches.
 * For every walk with steps s_0 .. s_(n-1) and every 0 < i < n - 1, let x = s_i, P = s_(i-1), N = s_(i+1).  Then i_in is the index
 *   of P ^ 1 in out[x ^ 1] and i_out the index of N in out[x]; both take the first match among the first 4 entries.
 *   (a, b) = (i_in, i_out) when x is even and (i_out, i_in) when x is odd, and through[16 (x >> 1) + 4 a + b] += 1.  If an index is
 *   not found, or x, P or N >= 2 U, nothing is added and n_missing counts it.  n_interior counts every such i, n_added the
 *   additions: n_interior = n_added + n_missing.  n_walks and n_steps are the call's arguments.
 * Everything is an integer count and a function of (walks, steps, CSR) alone, byte-identical across runs and variants.
 * Consequences:
 *   (a) with the CSR the walks were made with n_missing is 0: every step after a walk's first came from an EDGE or ACROSS join
 *       that found N in out[x], and the graph is mirror-symmetric, so P ^ 1 is in out[x ^ 1];
 *   (b) the walk of a read's reverse complement adds to the SAME cells: it passes x ^ 1 between N ^ 1 and P ^ 1, which swaps the
 *       two indices and the parity of x at once.  Unlike link_hits there is no mirror for the caller to add;
 *   (c) when both arrays come from the same walk calls, the row sum of through[u][a][.] is at most link_hits[e] +
 *       link_hits[mir(e)] for e = entry a of L (both terms also where mir(e) = e: a hairpin join is the way in of one step and
 *       the way out of the step before, in the same row); the same holds for the columns and R;
 *   (d) a circular unitig gone round twice adds to cell (0, 0) of itself.
 * Out of scope: several GPUs.  Evidence from paired reads is added to the same array by kmx_unitig_pair_paths below.         */
typedef struct kmx_through_stats { uint64_t n_walks, n_steps, n_interior, n_added, n_missing, reserved[3]; } kmx_through_stats;   /* 64 bytes */
/* On HOST buffers.  Needs no built model and no session (like kmx_unitig_contigs); it runs on the model's stream and is a
 * build-class call.  stats is required; every buffer of a non-zero count is required, link_offsets always.  KMX_E_ARG before
 * anything runs: a NULL required argument; U >= 2^31; walks whose first_step does not start at 0, with first_step[w + 1] !=
 * first_step[w] + n_steps[w], or whose last sum is not n_steps; a CSR that kmx_unitig_walk_segs would refuse (link_offsets[0]
 * != 0, decreasing, link_offsets[2 U] != n_links, a links[e] >= 2 U).  n_steps == 0 or U == 0: KMX_OK, nothing added.
 * KMX_E_NOMEM leaves the handle usable.                                                                                   */
int kmx_unitig_walk_through(kmx_model *m, const kmx_walk *walks, uint64_t n_walks, const uint32_t *steps, uint64_t n_steps, const uint64_t *link_offsets /* [2 U + 1] */,
                            const uint32_t *links, uint64_t n_links, uint64_t n_unitigs, uint64_t *through /* [16 U] */, kmx_through_stats *stats);
/* The same on DEVICE buffers, read where the walk and graph calls left them; stats is on the HOST.  It checks NULL and U and
 * validates nothing else; the kernels clamp instead.  The records' n_steps is not used: walk boundaries are the first_step
 * values, clamped into [0, n_steps]; row bounds are clamped into [0, n_links]; at most 4 entries of a row are read.  Bad input
 * gives wrong counts and never an access outside a buffer.  It enqueues everything on the model's stream and waits once, for the
 * stats.  Device memory, kept on the handle between calls: one byte per step plus the three counters.                       */
int kmx_unitig_walk_through_dev(kmx_model *m, const kmx_walk *d_walks, uint64_t n_walks, const uint32_t *d_steps, uint64_t n_steps, const uint64_t *d_link_offsets /* [2 U + 1] */,
                                const uint32_t *d_links, uint64_t n_links, uint64_t n_unitigs, uint64_t *d_through /* [16 U] */, kmx_through_stats *stats /* HOST */);

/* ---- resolution: a unitig whose through hits pair its ways in with its ways out one to one is split into one copy per way in.
 * The output is an ordinary unitig graph, so kmx_unitig_contigs merges through the repeat unchanged.
 * Input: as kmx_unitig_contigs (k, the unitig set, optionally urec, the CSR, optionally link_hits), through[16 U] as
 *   kmx_unitig_walk_through accumulated it, and kmx_resolve_params.
 * Unitig u, with R = out[2 u] of q entries and L = out[2 u + 1] of p entries, is a CANDIDATE iff p = q >= 2 and no entry of L or
 *   R has unitig index u.  This excludes self-loops, hairpins and circular unitigs.  For a candidate, cell (a, b) with a, b < p is
 *   SUPPORTED iff T = through[16 u + 4 a + b] >= min_reads and T >= 1.  The verdict is one of the following, in this order:
 *   CROSSED: some unsupported cell has T > max_cross.  UNSUPPORTED: no cell is supported.  RESOLVED: every row a has exactly one
 *   supported cell pi(a), and every column has exactly one.  AMBIGUOUS: otherwise.  Cells with a >= p or b >= p are ignored.
 * The new graph.  An unresolved unitig has 1 copy.  A resolved one has p copies, and copy c belongs to way in c.  first[u] is the
 *   exclusive sum of the copy counts, so new unitig first[u] + c is copy c of u; U' is the total.  Strings of copies are byte for
 *   byte the origin's; the new offsets follow.  Every input edge e (entry j of out[o], o = 2 u + d, target t = 2 v + dt) becomes
 *   exactly one new edge, so n_links does not change.  Its source: u unresolved: 2 first[u] + d; u resolved, d = 0 (j is a right
 *   index): copy pi^-1(j); u resolved, d = 1 (j is a left index): copy j.  Its target: v unresolved: 2 first[v] + dt; v resolved:
 *   with i = the index of o ^ 1 in out[t ^ 1], copy i for dt = 0 and copy pi_v^-1(i) for dt = 1.  Rows of an unresolved unitig
 *   keep their order.  Copy c of a resolved unitig, u' = first[u] + c, has out'[2 u'] = {entry pi(c) of R} and
 *   out'[2 u' + 1] = {entry c of L}.  Edges are numbered by (new oriented unitig, row order).
 * Output: rseq[seq_capacity] and roffsets[rec_capacity + 1]; rrec[rec_capacity], NULL exactly when urec is: the origin's record
 *   verbatim, with n_pred = n_succ = 1 for copies of a resolved unitig; origin[rec_capacity]; rplace[U]; rlink_offsets
 *   [2 rec_capacity + 1]; rlinks[n_links]; link_origin[n_links], the input edge; rlink_hits[n_links] = link_hits[link_origin], NULL
 *   exactly when link_hits is.  On the HOST: *n_unitigs_out, *n_bases_out and kmx_resolve_stats.  rseq == NULL is the sizing call:
 *   the two counts and the stats, nothing else is written or needed of the outputs.  A capacity too small is KMX_E_RANGE, with
 *   both counts set and nothing written.  4 U and 4 n_ubases always suffice; rec_capacity < 2^32, and a U' >= 2^31 is KMX_E_RANGE.
 * Consequences:
 *   (a) a no-op is exact: with through all zero, or with no resolved candidate, every output is byte for byte the input, and
 *       origin and link_origin are the identity;
 *   (b) the output is a valid input for kmx_unitig_contigs, whose host form accepts it: it is mirrored, has rows <= 4, has no edge
 *       twice, and every overlap holds;
 *   (c) a k-mer of a resolved unitig now appears p times, so the output is NOT a valid set for kmx_unitig_map_begin (it refuses
 *       with KMX_E_ARG); through hits for a second round therefore cannot be had;
 *   (d) everything is an integer count and a function of the input alone, byte-identical across runs and variants.
 * Out of scope: iterating; p != q; repeats with a self edge; choosing min_reads.  Evidence from paired reads reaches this
 * call through the cells kmx_unitig_pair_paths below adds to.                                                               */
typedef struct kmx_resolve_params { uint64_t min_reads, max_cross; } kmx_resolve_params;                                 /* 16 bytes */
typedef struct kmx_resolve_place { uint32_t first, n_copies; } kmx_resolve_place;                                        /* 8 bytes */
typedef struct kmx_resolve_stats { uint64_t n_candidates, n_resolved, n_crossed, n_unsupported, n_ambiguous, n_copies_added, n_unitigs_out, reserved; } kmx_resolve_stats;   /* 64 bytes */
/* On HOST buffers.  Needs no built model and no session; a build-class call on the model's stream.  KMX_E_ARG before anything
 * runs, as kmx_unitig_contigs: an even or out-of-range k, U >= 2^31, a NULL required buffer (urec and rrec go together where
 * U > 0, link_hits and rlink_hits where n_links > 0), an output that overlaps another buffer, bad uoffsets, a CSR that is not
 * valid and mirrored with rows <= 4.
 * U == 0: KMX_OK, roffsets[0] = rlink_offsets[0] = 0, all counts zero.  KMX_E_NOMEM leaves the handle usable.               */
int kmx_unitig_resolve(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const kmx_unitig *urec /* or NULL */,
                       const uint64_t *link_offsets /* [2 U + 1] */, const uint32_t *links, uint64_t n_links, const uint64_t *link_hits /* or NULL */, const uint64_t *through /* [16 U] */,
                       const kmx_resolve_params *params, char *rseq /* or NULL */, uint64_t seq_capacity, uint64_t *roffsets, uint64_t rec_capacity, kmx_unitig *rrec, uint32_t *origin,
                       kmx_resolve_place *rplace /* [U] */, uint64_t *rlink_offsets, uint32_t *rlinks, uint64_t *link_origin, uint64_t *rlink_hits, uint64_t *n_unitigs_out,
                       uint64_t *n_bases_out, kmx_resolve_stats *stats);
/* The same on DEVICE buffers; params, the two counts and stats are on the HOST.  It checks k, U, NULL and overlap; the kernels
 * clamp as those of kmx_unitig_contigs_dev do (uoffsets into [0, n_ubases], row bounds into [0, n_links], at most 4 entries of a
 * row), and an edge whose target is >= 2 U or whose mirror is not found makes BOTH its ends unresolved, so the renaming is always
 * defined.  Every store is checked against its capacity: bad input gives a wrong graph, never an access outside a buffer.  It
 * waits for the stream once, for the counts and the stats, in front of the records, links and bytes, which it leaves enqueued on
 * the model's stream.  Device memory, kept on the handle between calls: 53 bytes per unitig plus the scan's scratch.          */
int kmx_unitig_resolve_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets, uint64_t n_unitigs, uint64_t n_ubases, const kmx_unitig *d_urec /* or NULL */,
                           const uint64_t *d_link_offsets, const uint32_t *d_links, uint64_t n_links, const uint64_t *d_link_hits /* or NULL */, const uint64_t *d_through,
                           const kmx_resolve_params *params /* HOST */, char *d_rseq /* or NULL */, uint64_t seq_capacity, uint64_t *d_roffsets, uint64_t rec_capacity, kmx_unitig *d_rrec,
                           uint32_t *d_origin, kmx_resolve_place *d_rplace, uint64_t *d_rlink_offsets, uint32_t *d_rlinks, uint64_t *d_link_origin, uint64_t *d_rlink_hits,
                           uint64_t *n_unitigs_out /* HOST */, uint64_t *n_bases_out /* HOST */, kmx_resolve_stats *stats /* HOST */);
/* seconds[4] of the last of these two calls under kmx_set_profile(m, 1): verdicts, scan and records, links, bytes */
int kmx_unitig_resolve_last_phases(kmx_model *m, double *seconds /* [4] */);

/* ---- read pairs: where the two mates of a pair lie in the graph.  The repeats kmx_unitig_resolve leaves are longer than a read;
 * a read cannot cross them, the fragment both mates were read from can.  A post-pass on what kmx_unitig_walk_segs[_dev] wrote for
 * a batch in which reads 2 p and 2 p + 1 are the two mates of pair p (interleaved), inside the map session, which holds k, U and
 * m_u; it reads no bases and no segments.  The library is forward-reverse (FR): mate 2 comes from the opposite strand and faces
 * inward.  It gives the insert-size histogram of the library, the pairs per edge of the graph in the layout of link_hits (so
 * that kmx_unitig_contigs consumes it unchanged), and the pairs between unitigs that are not adjacent, with a distance: the
 * scaffold evidence.  The contigs of kmx_unitig_contigs are a valid unitig set for kmx_unitig_map_begin, so pairs mapped onto the
 * contigs give links between contigs without a coordinate translation.
 * Input: walks[n_walks], walk_offsets[n_seqs + 1] and steps[n_steps] as the walk call wrote them; n_seqs is even and
 *   n_pairs = n_seqs / 2; the CSR of the session's graph (link_offsets[2 U + 1], links[n_links]; out[o] is the row of oriented
 *   unitig o, at most 4 entries of a row are read); and kmx_pair_params, bin_width >= 1, n_bins in [1, 65536].
 * Placing a read.  The candidates of read r are the walks w in [walk_offsets[r], walk_offsets[r + 1]) with n_mapped >= min_mapped,
 *   n_steps >= 1, a last step o = steps[first_step + n_steps - 1] < 2 U and off_last < m_(o >> 1).  The ANCHOR is the candidate
 *   with the largest n_mapped (compared as min(n_mapped, 2^32 - 1)); ties go to the lowest index (only the first 2^32 - 1 walks
 *   of a read are looked at).  A read with no candidate is unplaced.  The INNER END of a placed read is (o, x) = (last step, off_last): the mapped window nearest to its mate.
 * A pair.  A is read 2 p, B is read 2 p + 1.  With both placed, a = (oa, xa) is A's inner end, and B's inner end (oB, xB) is
 *   mirrored onto A's strand: ob = oB ^ 1, xb = m_(oB >> 1) - 1 - xB.  All arithmetic is signed 64-bit.  The class of the pair:
 *   KMX_PAIR_NONE      neither mate is placed;
 *   KMX_PAIR_SINGLE    exactly one is;
 *   KMX_PAIR_SAME      oa == ob.  d = xb - xa and frag = d + A.n_span + B.n_span + k - 2: the fragment's bases between the outer
 *                      mapped windows, exact for reads without indels.  frag < 0: n_negative counts the pair; otherwise
 *                      hist[min(frag / bin_width, n_bins - 1)] += 1;
 *   KMX_PAIR_INVERTED  oa == ob ^ 1;
 *   otherwise dist = (m_(oa >> 1) - 1 - xa) + xb, the windows left in oa behind A plus the windows of ob in front of B, and
 *   KMX_PAIR_FAR       dist > max_dist;
 *   KMX_PAIR_LINK      otherwise.  With e the index of the first entry equal to ob among the (at most 4) entries of out[oa], if
 *                      there is one: pair_hits[e] += 1 and n_adjacent counts it -- the traversed direction only, exactly like
 *                      link_hits; the mirror edge is the consumer's to add.  The pair contributes (key, dist) to the pair links:
 *                      key = (oa, ob) when oa << 32 | ob is smaller than (ob ^ 1) << 32 | (oa ^ 1), and (ob ^ 1, oa ^ 1)
 *                      otherwise; the two are equal only for an inverted pair.
 * Output.  pairs[n_pairs] (or NULL), one record each.  hist[n_bins] and pair_hits[n_links] (either may be NULL) are ADDED to, as
 *   hits and link_hits are.  plinks[capacity] with *n_plinks (HOST in both forms) is an IN/OUT list of kmx_pair_link, strictly
 *   ascending by a << 32 | b: on entry what earlier batches left (a first call passes *n_plinks = 0), on return the merge with
 *   this batch, equal keys folded by sum, sum, minimum and maximum; capacity >= *n_plinks + n_pairs always suffices.  If more
 *   entries are needed the call returns KMX_E_RANGE with *n_plinks the number needed, the list exactly as it was and records,
 *   stats, hist and pair_hits complete, so a caller that repeats the call passes hist = pair_hits = NULL: the convention of
 *   kmx_unitig_map_seqs.  plinks == NULL: no list is built and *n_plinks is not used.  stats (HOST in both forms, required).
 * Every decision looks at two anchors, two walks, two steps, two m_u and one row, and all outputs are integer sums, counts,
 * minima and maxima: a function of (walks, steps, CSR, m_u, parameters, list) alone, byte-identical across runs, variants and
 * batch splits.  Consequences:
 *   (a) swapping the two mates of every pair leaves hist, the list, stats and every SAME d and frag unchanged, and moves each
 *       pair_hits increment to the mirror edge: A' = B and B' = A give oa' = ob ^ 1 and ob' = oa ^ 1, which mirrors the same
 *       position, swaps the two terms of dist and picks the same canonical key;
 *   (b) n_none + n_single + n_same + n_inverted + n_link + n_far == n_pairs; the n_pairs added to the list sum to n_link, the
 *       increments to hist to n_same - n_negative, those to pair_hits to n_adjacent;
 *   (c) cutting a batch at any pair boundary and merging into the same list gives the same bytes as one call;
 *   (d) for error-free pairs drawn from a genome that is one unitig every pair is SAME and frag is the true fragment length.
 * Out of scope: RF and FF libraries; mates in two separate files; pairs on a resolved graph, where a k-mer lies on several
 * copies; choosing max_dist; several GPUs.  What acts on the links: kmx_unitig_scaffold below.                            */
#define KMX_PAIR_NONE     0
#define KMX_PAIR_SINGLE   1
#define KMX_PAIR_SAME     2
#define KMX_PAIR_INVERTED 3
#define KMX_PAIR_LINK     4
#define KMX_PAIR_FAR      5
typedef struct kmx_pair_params { uint32_t min_mapped, max_dist, bin_width, n_bins; } kmx_pair_params;                    /* 16 bytes */
typedef struct kmx_pair {                /* one per pair; 64 bytes, no padding */
	uint64_t walk_a, walk_b;             /* the anchors' indices into walks; all ones for an unplaced mate */
	uint32_t cls;                        /* KMX_PAIR_* */
	uint32_t edge;                       /* e of a LINK between adjacent unitigs; 0xFFFFFFFF when there is none */
	uint32_t oa, xa, ob, xb;             /* the inner ends, B's mirrored; 0 for an unplaced mate */
	int64_t d;                           /* d for SAME, dist for LINK and FAR, 0 otherwise */
	int64_t frag;                        /* SAME only, 0 otherwise */
	uint64_t reserved;                   /* 0 */
} kmx_pair;
typedef struct kmx_pair_link {           /* 32 bytes, no padding */
	uint32_t a, b;                       /* the canonical key: oriented unitig a, then b at the distance below */
	uint64_t n_pairs, sum_dist;
	uint32_t min_dist, max_dist;
} kmx_pair_link;
typedef struct kmx_pair_stats { uint64_t n_pairs, n_none, n_single, n_same, n_negative, n_inverted, n_link, n_adjacent, n_far, reserved; } kmx_pair_stats;   /* 80 bytes */
/* On HOST buffers.  KMX_E_ARG before anything runs: an odd n_seqs, bin_width == 0, n_bins outside [1, 65536], a NULL required
 * buffer (params, stats and walk_offsets; walks, steps and links where their count is not 0; link_offsets; n_plinks with
 * plinks), *n_plinks > capacity, an output that overlaps an input; walk_offsets (first 0, non-decreasing, last n_walks) and the
 * CSR checked as kmx_unitig_walk_segs checks seg_offsets and the CSR; an input list that is not strictly ascending.  Outside a
 * session: KMX_E_STATE.  KMX_E_NOMEM leaves the handle and the session usable.  n_seqs == 0: KMX_OK, all-zero stats, the list
 * untouched.  It stages its input and output on the device as the host form of the walk call does.                          */
int kmx_unitig_pair_walks(kmx_model *m, const kmx_walk *walks, uint64_t n_walks, const uint64_t *walk_offsets /* [n_seqs + 1] */, uint64_t n_seqs, const uint32_t *steps, uint64_t n_steps,
                          const uint64_t *link_offsets /* [2 U + 1] */, const uint32_t *links, uint64_t n_links, const kmx_pair_params *params, kmx_pair *pairs /* [n_seqs / 2] or NULL */,
                          uint64_t *hist /* [n_bins] or NULL */, uint64_t *pair_hits /* [n_links] or NULL */, kmx_pair_link *plinks /* or NULL */, uint64_t capacity, uint64_t *n_plinks,
                          kmx_pair_stats *stats);
/* The same on DEVICE buffers, read where the walk and graph calls left them; params, *n_plinks and stats are on the HOST.  It
 * checks the parameters, NULL, *n_plinks <= capacity and overlap, and clamps instead of validating: walk_offsets into
 * [0, n_walks]; a walk whose first_step + n_steps - 1 is not in [0, n_steps) is no candidate; row bounds into [0, n_links]; the
 * input list is taken as it is (a list that is not ascending is merged all the same).  Every store is checked against its
 * capacity: bad device input gives wrong pairs and never an access outside a buffer.  It enqueues everything on the model's
 * stream and waits once, for the merged count and the stats; the list is written by a last launch only where the count fits.
 * Device memory, kept on the session until kmx_unitig_map_end: 8 bytes per read for the anchors, 4 per pair for the distances,
 * and 72 bytes per work item (a pair or an entry of the input list: key and index, both twice for the sort; the scanned key
 * changes; the merged record) plus the scratch of the sort and the scan.                                                       */
int kmx_unitig_pair_walks_dev(kmx_model *m, const kmx_walk *d_walks, uint64_t n_walks, const uint64_t *d_walk_offsets /* [n_seqs + 1] */, uint64_t n_seqs, const uint32_t *d_steps,
                              uint64_t n_steps, const uint64_t *d_link_offsets /* [2 U + 1] */, const uint32_t *d_links, uint64_t n_links, const kmx_pair_params *params /* HOST */,
                              kmx_pair *d_pairs /* or NULL */, uint64_t *d_hist /* or NULL */, uint64_t *d_pair_hits /* or NULL */, kmx_pair_link *d_plinks /* or NULL */, uint64_t capacity,
                              uint64_t *n_plinks /* HOST */, kmx_pair_stats *stats /* HOST */);

/* ---- scaffolds: unitigs or contigs ordered and oriented along the pair links, spelled with runs of 'N' sized from the insert
 * size.  A repeat longer than a read, or a hole in the coverage, ends every contig; the pairs that span it are in the list
 * kmx_unitig_pair_walks leaves.  This call keeps the links the pairs support and joins what has become the only way on.  The
 * construction of the contig rule on another edge set: a list of unbounded degree instead of rows of at most 4, and bytes that
 * carry gaps.
 * Input: k, odd, in [5, 63]; a unitig set in the layout of kmx_query_seqs (useq, uoffsets[U + 1], U < 2^31, every unitig at least
 *   k bytes of uppercase ACGT, not checked; a reverse step complements with the byte map of kmx_unitig_contigs, whose contigs are
 *   such a set); optionally urec[U] (only sum_count, min_count and max_count are read); plinks[n_plinks] as
 *   kmx_unitig_pair_walks leaves it, n_plinks < 2^31; and kmx_scaffold_params: ratio in [0, 65536], min_n <= max_n, reserved = 0.
 *   Links.  Entry i is a PAIR LINK iff a < 2 U, b < 2 U, a >> 1 != b >> 1 and n_pairs >= 1; every other entry is ignored and
 *     counted in n_ignored.  A pair link is one edge a -> b and its own mirror b ^ 1 -> a ^ 1, both with sup = n_pairs.  out(o) is
 *     the multiset of edges out of oriented unitig o: in a list that is not canonical, two entries that give the same edge are
 *     two edges.
 *   Kept edges.  best(o) = the largest sup over out(o), 0 when it is empty.  An entry is below_min iff n_pairs < min_pairs;
 *     otherwise below_ratio iff ratio > 0 and (n_pairs * ratio < best(a) or n_pairs * ratio < best(b ^ 1)), the product taken in
 *     128 bits; otherwise KEPT.  nk(o) = the kept edges in out(o), a true count (below 2^31, as n_plinks is).
 *   Chain links.  Entry i is a chain link iff it is kept, nk(a) == 1 and nk(b ^ 1) == 1; then a -> b and b ^ 1 -> a ^ 1.  The
 *     argument of the contig rule holds unchanged, because a >> 1 != b >> 1 excludes o -> o ^ 1: the 2 U oriented unitigs fall
 *     into mirror-paired paths and cycles, and no component holds both orientations of a unitig.
 *   Gap of a chain link, in signed 64-bit arithmetic (two's complement, wrapping): D = sum_dist / n_pairs (unsigned floor
 *     division); g = inner - 1 - D, where inner is the library's typical d of a KMX_PAIR_SAME pair: a pair across a hole of g
 *     missing windows has d = dist + g + 1; est = g - (k - 1), the estimated bases between the two unitigs, negative when they
 *     would overlap; n_gap = min(max(est, min_n), max_n), the 'N' bytes written.
 *   Scaffolds: one per mirror pair, chosen exactly as contigs are (a single step takes d = 0; of a path and its mirror the one
 *     whose first step has the smaller unitig index; a cycle starts at its smallest unitig in orientation 0 and is spelled open,
 *     marked circular), in ascending unitig index of the first step.  The string is the WHOLE oriented string of o_1, then for each
 *     later step n_gap bytes 'N' and the WHOLE oriented string of that step: pair links claim no overlap, so nothing is trimmed.
 * Output.  sseq[seq_capacity] and soffsets[U + 1] in the layout of kmx_query_seqs (S + 1 offsets are written); srec[U], the
 *   records below (S are written); steps[U], back to back in scaffold order: n_gap and est belong to the link IN FRONT of the
 *   step, are 0 for the first step of a path, and for the first step of a cycle are the closing link's (not spelled, not counted
 *   in n_gap_bases); place[U]: unitig u lies in scaffold os >> 1, os & 1 is 1 iff its step is 2 u + 1, step is the index of that
 *   step inside its scaffold and off the base offset of the step's first byte there.  On the HOST: *n_scaffolds, *n_sbases and
 *   kmx_scaffold_stats.  *n_sbases > seq_capacity: KMX_E_RANGE, everything but sseq complete, nothing written at or behind
 *   sseq[seq_capacity]; n_ubases + (U - 1) * max_n always suffices.  sseq == NULL with seq_capacity == 0 is the sizing call (KMX_OK
 *   when there is nothing to spell, KMX_E_RANGE otherwise), as in the unitig calls.  Everything is an integer sum, count, minimum
 *   or maximum and a function of the input alone: byte-identical across runs and forms.
 * Consequences:
 *   (a) with n_plinks = 0, or min_pairs above every entry, every scaffold is one unitig and sseq and soffsets are the input byte
 *       for byte;
 *   (b) replacing any entry (a, b) by (b ^ 1, a ^ 1) changes nothing but which entry is counted in n_chain;
 *   (c) place inverts steps; the n_steps sum to U; n_sbases = n_ubases + the sum of n_gap_bases;
 *   (d) two islands of one genome that the pairs span come out as one scaffold with the hole as a run of 'N' of its true length,
 *       when inner is the library's d.
 * Out of scope: comparing bases when est < 0; RF and FF libraries; several GPUs; choosing min_pairs and inner.  Gaps the graph can
 * spell: kmx_unitig_scaffold_fill below.  Links that skip a unitig: kmx_unitig_pair_reduce below drops them from the list before
 * this call.  A unitig-level list in contig coordinates through place: kmx_unitig_pair_lift below.                           */
typedef struct kmx_scaffold_params { uint64_t min_pairs; uint32_t ratio /* [0, 65536] */; uint32_t inner; uint32_t min_n, max_n /* min_n <= max_n */;
                                     uint64_t reserved /* 0 */; } kmx_scaffold_params;                                  /* 32 bytes */
#define KMX_SCAFFOLD_CIRCULAR 0x80000000u
typedef struct kmx_scaffold {            /* one per scaffold; 64 bytes, no padding */
	uint64_t n_bases;                    /* the bytes of its string, the N included */
	uint64_t n_kmers;                    /* the sum of m_u over its steps */
	uint64_t sum_count;                  /* from urec; 0 when urec is NULL */
	uint32_t min_count, max_count;       /* from urec; 0 when urec is NULL */
	uint32_t first_step;                 /* its steps are steps[first_step .. first_step + n_steps) */
	uint32_t n_steps;                    /* below 2^31; KMX_SCAFFOLD_CIRCULAR is set above it for a cycle: circular = n_steps >> 31 */
	uint64_t n_gap_bases;                /* the spelled N */
	uint64_t min_pairs, sum_pairs;       /* n_pairs over its chain links, the closing link of a cycle included; 0 when it has none */
} kmx_scaffold;
typedef struct kmx_scaffold_step { uint32_t o; uint32_t n_gap; int64_t est; } kmx_scaffold_step;                         /* 16 bytes */
typedef struct kmx_scaffold_place { uint32_t os; uint32_t step; uint64_t off; } kmx_scaffold_place;                      /* 16 bytes */
typedef struct kmx_scaffold_stats { uint64_t n_entries, n_links, n_ignored, n_below_min, n_below_ratio, n_kept, n_chain /* entries of the list, each */,
                                    n_scaffolds, n_circular, n_multi /* scaffolds of more than one step */; } kmx_scaffold_stats;   /* 80 bytes */
/* On HOST buffers.  Needs no built model and no session (like kmx_unitig_contigs); it runs on the model's stream and is a
 * build-class call.  urec may be NULL, plinks with n_plinks == 0, sseq with seq_capacity == 0; every other buffer is required
 * (with U == 0 only soffsets, the two counts and stats).  KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31,
 * n_plinks >= 2^31, ratio > 65536, min_n > max_n, reserved != 0, a NULL required buffer, an output that overlaps an input or
 * another output; uoffsets whose first entry is not 0, that decrease, or that give a unitig fewer than k bytes; a list that is
 * not strictly ascending by a << 32 | b.  U == 0: KMX_OK, soffsets[0] = 0, all counts zero but n_entries and n_ignored.
 * KMX_E_NOMEM leaves the handle usable.  The call returns when the output is complete.                                      */
int kmx_unitig_scaffold(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const kmx_unitig *urec /* or NULL */,
                        const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_scaffold_params *params, char *sseq /* [seq_capacity] or NULL */, uint64_t seq_capacity,
                        uint64_t *soffsets /* [U + 1] */, kmx_scaffold *srec /* [U] */, kmx_scaffold_step *steps /* [U] */, kmx_scaffold_place *place /* [U] */,
                        uint64_t *n_scaffolds, uint64_t *n_sbases, kmx_scaffold_stats *stats);
/* The same on DEVICE buffers, read where the graph, contig and pair calls left them; params, the two counts and stats are on the
 * HOST.  It checks k, U, n_plinks, the parameters, NULL and overlap, and validates nothing else on the host; the kernels clamp
 * instead, exactly as the contig kernels do: uoffsets into [0, n_ubases]; an entry that is no pair link is ignored; the list is
 * taken as it is (not ascending, not canonical, duplicate keys: every entry is its own edge); and the chain link is tested
 * from both sides, so whatever the list holds the links form mirror-paired paths and cycles and the doubling ends within
 * ceil(log2 2U) + 1 rounds, the cut, and as many again.  Every store is checked against U, seq_capacity or n_plinks.  Bad device
 * input gives wrong scaffolds and never an access outside a buffer.
 * It waits for the stream once per doubling round and once for the counts; the bytes are written only after that wait has
 * shown that n_sbases fits (the N by a fill of sseq[0, n_sbases), the unitigs over it by the tile emit of the contigs), and a
 * last wait behind them leaves nothing in flight.  Device memory, kept on the handle between calls through the owning types
 * of hip_owned.h: 145 bytes per unitig (2 x 32 for the two copies of pointer, step rank and byte rank of both orientations, whose
 * spare copy the marks reuse; 2 x 8 for the two copies of the running minimum; 24 for the scanned marks; 2 x 16 for best, the
 * kept count and the smallest kept entry of both orientations; 1 for the cycle flag; 8 for where a unitig's bytes go) and none
 * per entry, plus the scan's scratch.  The host form also stages its input and output there.                                 */
int kmx_unitig_scaffold_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, uint64_t n_ubases,
                            const kmx_unitig *d_urec /* or NULL */, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_scaffold_params *params /* HOST */,
                            char *d_sseq /* [seq_capacity] or NULL */, uint64_t seq_capacity, uint64_t *d_soffsets /* [U + 1] */, kmx_scaffold *d_srec /* [U] */,
                            kmx_scaffold_step *d_steps /* [U] */, kmx_scaffold_place *d_place /* [U] */, uint64_t *n_scaffolds /* HOST */, uint64_t *n_sbases /* HOST */,
                            kmx_scaffold_stats *stats /* HOST */);
/* where the last of these two calls on the handle spent its time, measured only under kmx_set_profile(m, 1) (every phase then
 * waits for the stream): seconds[5] = verdicts, ranking (links, rounds, cut), marks and their scan, records with steps and
 * places, the bytes; *rounds = its doubling rounds (counted always)                                                          */
int kmx_unitig_scaffold_last_phases(kmx_model *m, double *seconds /* [5] */, uint64_t *rounds);

/* ---- pair paths: for every entry of a pair list, the unique path of the unitig graph between its two ends whose length fits
 * the library's insert size.  A repeat longer than a read but shorter than the fragment between the mates is crossed by no read,
 * so kmx_unitig_walk_through leaves its cells at 0; the pairs that span it are entries of the list kmx_unitig_pair_walks leaves.
 * This call finds the one graph path such an entry stands for and credits that path's interior unitigs (in the layout of
 * through) and edges (in the layout of link_hits), so that kmx_unitig_resolve and kmx_unitig_contigs consume it unchanged.  It
 * needs no model, no session and no bases.
 * Input: k, odd, in [5, 63]; uoffsets[U + 1] of the unitig set, U < 2^31, with m_u = max(len_u - (k - 1), 0) the windows of
 *   unitig u; the CSR (link_offsets[2 U + 1], links[n_links]; row(o) is the row of oriented unitig o): at most 4 entries of a row
 *   are read, and an entry >= 2 U is skipped, neither matched nor extended; plinks[n_plinks] as kmx_unitig_pair_walks leaves it,
 *   n_plinks < 2^31; and kmx_pair_path_params: max_steps in [1, KMX_PATH_MAX_STEPS], max_visits in [1, 65536], reserved = 0.
 * Entry i = (a, b, n_pairs, sum_dist, ...), all arithmetic in signed 64 bits (two's complement, wrapping):
 *   KMX_PATH_IGNORED    unless a < 2 U, b < 2 U, a >> 1 != b >> 1 and n_pairs >= 1: the scaffold call's pair link;
 *   KMX_PATH_BELOW_MIN  otherwise, if n_pairs < min_pairs.
 *   Otherwise D = sum_dist / n_pairs (unsigned floor division), g = inner - 1 - D (the g of kmx_unitig_scaffold: the windows
 *   missing between a and b), lo = g - tol, hi = g + tol.  hi < 0: KMX_PATH_NO_PATH with n_visited = 0.
 *   A PREFIX is a sequence v_1 .. v_t with 0 <= t <= max_steps, v_1 an entry of row(a), v_(j+1) an entry of row(v_j), and
 *     W = the sum of m_(v_j >> 1) <= hi.  The empty prefix is one; every row position gives a prefix of its own (an edge listed
 *     twice gives two); intermediates may repeat and may equal a or b.
 *   A prefix is a HIT iff b is among the read entries of row(v_t) (row(a) for t = 0) and W >= lo; a prefix is at most one hit.
 *   n_prefix = the number of prefixes, n_visited = min(n_prefix, max_visits + 1).  The verdict, in this order:
 *   KMX_PATH_COMPLEX    n_prefix > max_visits; n_hits is then 0 and nothing else is reported;
 *   KMX_PATH_NO_PATH    n_hits = 0;
 *   KMX_PATH_AMBIGUOUS  n_hits >= 2;
 *   KMX_PATH_ADJACENT   one hit with t = 0: kmx_unitig_pair_walks has counted it in pair_hits, nothing is added here;
 *   KMX_PATH_PATH       one hit with t >= 1.
 *   The definition counts sets, so no search order shows; a search that stops once its counter has passed max_visits gives the
 *   same verdict.
 * Effects of a PATH with steps v_1 .. v_t, v_0 = a and v_(t+1) = b.  For 1 <= j <= t, with x = v_j, P = v_(j-1), N = v_(j+1):
 *   the cell is exactly that of kmx_unitig_walk_through (i_in the first match of P ^ 1 in row(x ^ 1), i_out that of N in row(x),
 *   swapped for odd x) and through[16 (x >> 1) + 4 a + b] += n_pairs; an index not found is counted in n_missing and adds
 *   nothing, every other one in n_added.  For 0 <= j <= t: path_hits[e] += n_pairs for e the first entry equal to v_(j+1) in
 *   row(v_j): the traversed direction only, like link_hits.
 * Output.  precs[n_plinks], the records below: n_steps = t, windows = W and first_step of the hit are set for PATH and ADJACENT
 *   and are 0 otherwise; first_step is the number of steps of the PATH entries in front of the entry.  psteps[capacity]: the
 *   intermediates of the PATH entries, back to back in entry order, with *n_psteps (HOST in both forms) their number.
 *   through[16 U] and path_hits[n_links] are ADDED to; either may be NULL (n_added and n_missing are counted all the same).
 *   stats is required and on the HOST in both forms.  More steps than capacity: KMX_E_RANGE with *n_psteps the number needed
 *   and records, stats, through and path_hits complete, so a caller that repeats the call passes those two as NULL: the
 *   convention of kmx_unitig_pair_walks.  n_plinks * max_steps always suffices.  psteps == NULL: no list is built and n_psteps
 *   may be NULL (where it is given it is set).
 * Consequences:
 *   (a) n_ignored + n_below_min + n_no_path + n_adjacent + n_path + n_ambiguous + n_complex == n_entries; the n_steps of the PATH
 *       entries sum to *n_psteps = n_added + n_missing;
 *   (b) with a mirrored CSR and no COMPLEX in either direction, replacing an entry by its mirror (b ^ 1, a ^ 1) leaves verdict,
 *       n_hits and windows as they are, gives the steps reversed and flipped (v_t ^ 1 .. v_1 ^ 1), adds to the SAME cells of
 *       through (as the walk of a read's reverse complement does) and moves every path_hits increment to the mirror edge;
 *   (c) through summed with the array of kmx_unitig_walk_through feeds kmx_unitig_resolve unchanged, and path_hits summed with
 *       link_hits feeds kmx_unitig_contigs;
 *   (d) every output is an integer count or sum and a function of the input alone: byte-identical across runs and forms.
 * Out of scope: meeting in the middle; choosing among several paths, by coverage or by fit; a search per pair instead of per
 * entry; RF and FF libraries; several GPUs; choosing tol and inner.  A scaffold link is such an entry: kmx_unitig_scaffold_fill
 * below spells its path into the scaffold's gap.                                                                             */
#define KMX_PATH_IGNORED   0
#define KMX_PATH_BELOW_MIN 1
#define KMX_PATH_NO_PATH   2
#define KMX_PATH_ADJACENT  3
#define KMX_PATH_PATH      4
#define KMX_PATH_AMBIGUOUS 5
#define KMX_PATH_COMPLEX   6
#define KMX_PATH_MAX_STEPS 16
typedef struct kmx_pair_path_params { uint64_t min_pairs; uint32_t inner, tol, max_steps /* [1, KMX_PATH_MAX_STEPS] */, max_visits /* [1, 65536] */;
                                      uint64_t reserved /* 0 */; } kmx_pair_path_params;                                /* 32 bytes */
typedef struct kmx_pair_path {           /* one per entry of the list; 32 bytes, no padding */
	uint32_t verdict;                    /* KMX_PATH_* */
	uint32_t n_steps;                    /* t of the hit */
	uint64_t first_step;                 /* its steps are psteps[first_step .. first_step + n_steps) */
	uint64_t windows;                    /* W of the hit */
	uint32_t n_hits, n_visited;
} kmx_pair_path;
typedef struct kmx_pair_path_stats { uint64_t n_entries, n_ignored, n_below_min, n_no_path, n_adjacent, n_path, n_ambiguous, n_complex, n_added, n_missing; } kmx_pair_path_stats;   /* 80 bytes */
/* On HOST buffers.  Needs no built model and no session (like kmx_unitig_scaffold); it runs on the model's stream and is a
 * build-class call.  psteps, through and path_hits may be NULL, links with n_links == 0, plinks and precs with n_plinks == 0;
 * every other buffer is required.  KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31, n_plinks >= 2^31,
 * max_steps or max_visits out of range, reserved != 0, a NULL required buffer, an output that overlaps an input or another
 * output; uoffsets whose first entry is not 0, that decrease, or that give a unitig fewer than k bytes; a CSR that
 * kmx_unitig_walk_segs would refuse; a list that is not strictly ascending by a << 32 | b.  n_plinks == 0: KMX_OK, all-zero
 * stats.  U == 0: KMX_OK, every entry is IGNORED.  KMX_E_NOMEM leaves the handle usable.                                      */
int kmx_unitig_pair_paths(kmx_model *m, int k, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const uint64_t *link_offsets /* [2 U + 1] */, const uint32_t *links,
                          uint64_t n_links, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_path_params *params, kmx_pair_path *precs /* [n_plinks] */,
                          uint32_t *psteps /* [capacity] or NULL */, uint64_t capacity, uint64_t *n_psteps, uint64_t *through /* [16 U] or NULL */, uint64_t *path_hits /* [n_links] or NULL */,
                          kmx_pair_path_stats *stats);
/* The same on DEVICE buffers, read where the graph and pair calls left them; params, *n_psteps and stats are on the HOST.  It
 * checks k, U, n_plinks, the parameters, NULL and overlap, and validates nothing else; the kernels clamp instead: row bounds into
 * [0, n_links], at most 4 entries of a row, an entry >= 2 U skipped, a unitig whose offsets decrease or that is shorter than k
 * has m_u = 0, and the list is taken as it is.  Every store is checked against its capacity: bad device input gives wrong paths
 * and never an access outside a buffer.  No entry costs more than max_visits + 1 visits.  It enqueues everything on the model's
 * stream and waits once, for *n_psteps and the stats; the steps are stored only where they fit.  Device memory, kept on the
 * handle between calls through the owning types of hip_owned.h: 4 max_steps + 8 bytes per entry plus the scan's scratch.  The
 * host form also stages its input and output there.                                                                         */
int kmx_unitig_pair_paths_dev(kmx_model *m, int k, const uint64_t *d_uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const uint64_t *d_link_offsets /* [2 U + 1] */,
                              const uint32_t *d_links, uint64_t n_links, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_pair_path_params *params /* HOST */,
                              kmx_pair_path *d_precs /* [n_plinks] */, uint32_t *d_psteps /* [capacity] or NULL */, uint64_t capacity, uint64_t *n_psteps /* HOST */,
                              uint64_t *d_through /* [16 U] or NULL */, uint64_t *d_path_hits /* [n_links] or NULL */, kmx_pair_path_stats *stats /* HOST */);
/* seconds[3] of the last of these two calls under kmx_set_profile(m, 1): the search, the scan, the additions with the wait */
int kmx_unitig_pair_paths_last_phases(kmx_model *m, double *seconds /* [3] */);

/* ---- filled scaffolds: the scaffolds of kmx_unitig_scaffold spelled again, with the bases of the graph in every gap that
 * kmx_unitig_pair_paths found the one path for.  A scaffold writes a run of 'N' between two steps even where the unitig graph
 * holds the real bases of that gap, and writes two whole strings with at least min_n 'N' between them even where the two steps
 * share a graph edge and so overlap by k - 1 bases.  This call takes what the two calls returned and needs no model, no session
 * and no CSR.
 * Input: k, odd, in [5, 63]; the unitig set the scaffold call was given (useq, uoffsets[U + 1], U < 2^31, every unitig at least k
 *   bytes); srec[S] and steps[U] as the scaffold call left them (of srec only first_step and n_steps with its circular bit are
 *   read: every scaffold holds a step, first_step is the number of steps of the scaffolds in front of it, and the steps sum to
 *   U; of steps, o and n_gap); plinks[n_plinks], strictly ascending by a << 32 | b, n_plinks < 2^31; precs[n_plinks] and
 *   psteps[n_psteps] as kmx_unitig_pair_paths left them on that list and the graph's CSR; and kmx_fill_params: kinds in [0, 3]
 *   (bit 0: fill PATH links, bit 1: fill ADJACENT links), reserved = 0.
 *   The entry of a link.  Take step j >= 1 of a scaffold, p = steps[first_step + j - 1].o and q = steps[first_step + j].o.  F is
 *     the entry with (a, b) = (p, q), M the entry with (a, b) = (q ^ 1, p ^ 1), each found by a lower-bound search on the key.
 *     The link's entry is F if it exists, else M, else none.
 *   The path of a link.  Through F it is psteps[first_step .. first_step + t) of the entry's record as it stands; through M it is
 *     reversed and flipped, v_t ^ 1 .. v_1 ^ 1: consequence (b) of the pair-path contract.
 *   The kind of a step.  KMX_FILL_HEAD: step 0 of its scaffold (the closing link of a cycle is never spelled, as in the scaffold
 *     call).  KMX_FILL_PATH: the entry's verdict is KMX_PATH_PATH, kinds & 1, 1 <= t <= KMX_PATH_MAX_STEPS, first_step + t <=
 *     n_psteps and every v < 2 U.  KMX_FILL_ADJACENT: the verdict is KMX_PATH_ADJACENT and kinds & 2; then t = 0.  KMX_FILL_N:
 *     everything else.
 *   The bytes.  A HEAD step writes the whole oriented string of its unitig.  An N step writes steps[].n_gap bytes 'N', then the
 *     whole oriented string of q: exactly what the scaffold call writes.  A PATH or ADJACENT step writes, for each v_j in turn,
 *     the LAST m_v = len_v - (k - 1) bytes of the oriented string of v_j (a PIECE), then the last len_q - (k - 1) bytes of the
 *     oriented string of q: consecutive unitigs along a graph edge overlap by k - 1 bytes.  The rule is defined on lengths
 *     alone; overlaps are not checked.  A reverse step or piece complements with the byte map of kmx_unitig_contigs.
 * Output.  fseq[seq_capacity] and foffsets[S + 1] in the layout of kmx_query_seqs; frec[S] and fsteps[U], the records below, the
 *   steps in the order of steps[]: off is where the step's WHOLE oriented string starts inside its scaffold (for a filled step
 *   k - 1 bytes in front of its first written byte), n_front the 'N' or the piece bytes in front of the step; pieces[
 *   piece_capacity]: the oriented unitigs of every filled path, back to back in scaffold order (frec.first_piece, fsteps.
 *   n_pieces); it may be NULL.  On the HOST: *n_fbases, *n_pieces and kmx_fill_stats.  *n_fbases > seq_capacity: KMX_E_RANGE,
 *   everything but fseq complete, nothing written at or behind fseq[seq_capacity]; *n_fbases is the scaffold call's n_sbases less
 *   n_gap + (k - 1) per filled link plus W, the windows of its path, per PATH link, so n_ubases + (U - 1) * (the largest n_gap) +
 *   the sum of W over the filled links suffices.  fseq == NULL with seq_capacity == 0 is the sizing call, as in the
 *   scaffold call.  More pieces than piece_capacity: KMX_E_RANGE with *n_pieces the number needed and everything else, fseq
 *   included, complete: the convention of psteps; pieces == NULL: no list is built and n_pieces may be NULL.  Everything is an
 *   integer sum or count and a function of the input alone: byte-identical across runs and forms.
 * Consequences:
 *   (a) with kinds = 0, or no PATH / ADJACENT entry among the chain links, fseq and foffsets are the scaffold call's sseq and
 *       soffsets byte for byte;
 *   (b) where every edge of the CSR is a true k - 1 overlap, fseq[foffsets[s] + off, + len) is the oriented string of the step,
 *       for every step;
 *   (c) replacing an entry and its record and steps by their mirror changes nothing in fseq;
 *   (d) per scaffold, n_bases = the sum of len over its steps - (k - 1) * its filled links + n_gap_bases + n_fill_bases.
 * Out of scope: choosing among several paths (an AMBIGUOUS entry stays a run of 'N'); comparing bases when est < 0 or along a
 * filled link; filling the closing link of a cycle; several GPUs.                                                             */
#define KMX_FILL_HEAD     0
#define KMX_FILL_N        1
#define KMX_FILL_ADJACENT 2
#define KMX_FILL_PATH     3
#define KMX_FILL_NO_ENTRY 0xFFFFFFFFu
typedef struct kmx_fill_params { uint32_t kinds /* [0, 3] */; uint32_t reserved /* 0 */; } kmx_fill_params;                    /* 8 bytes */
typedef struct kmx_scaffold_fill {       /* one per scaffold; 64 bytes, no padding */
	uint64_t n_bases;                    /* the bytes of its string */
	uint64_t n_gap_bases;                /* the 'N' still written */
	uint64_t n_fill_bases;               /* the bytes of its path pieces */
	uint64_t n_path_links, n_adjacent_links, n_n_links;   /* its steps behind the first, by kind */
	uint64_t n_pieces;                   /* its pieces are pieces[first_piece .. first_piece + n_pieces) */
	uint64_t first_piece;
} kmx_scaffold_fill;
typedef struct kmx_fill_step {           /* one per step; 32 bytes, no padding */
	uint32_t o;                          /* the oriented unitig, steps[].o */
	uint32_t kind;                       /* KMX_FILL_* */
	uint32_t entry;                      /* the entry of the link in front, KMX_FILL_NO_ENTRY for none and at a HEAD */
	uint32_t n_pieces;                   /* t of a PATH step, else 0 */
	uint64_t off;                        /* where the step's whole oriented string starts inside its scaffold */
	uint64_t n_front;                    /* the 'N' (N step) or the piece bytes (PATH step) in front of it */
} kmx_fill_step;
typedef struct kmx_fill_stats { uint64_t n_head, n_path, n_adjacent, n_n /* steps of each kind */, n_no_entry /* links without an entry */,
                                n_mirror /* links whose entry is M */, n_removed /* the 'N' of the filled links */, n_filled /* the piece bytes */, reserved[2]; } kmx_fill_stats;   /* 80 bytes */
/* On HOST buffers; it stages through the handle, runs on the model's stream and is a build-class call.  pieces may be NULL,
 * plinks and precs with n_plinks == 0, psteps with n_psteps == 0, fseq with seq_capacity == 0; every other buffer is required
 * (with U == 0 only foffsets, n_fbases and stats).  KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31,
 * n_plinks >= 2^31, S > U, kinds > 3, reserved != 0, a NULL required buffer, an output that overlaps an input or another output;
 * uoffsets whose first entry is not 0, that decrease, or that give a unitig fewer than k bytes; a list that is not strictly
 * ascending by a << 32 | b; a scaffold with first_step + n_steps > U, without a step, or whose first_step is not the number of
 * steps in front of it; steps that do not sum to U.  U == 0: KMX_OK, foffsets[0] = 0, all counts zero.  KMX_E_NOMEM leaves the
 * handle usable.  The call returns when the output is complete.                                                            */
int kmx_unitig_scaffold_fill(kmx_model *m, int k, const char *useq, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const kmx_scaffold *srec /* [n_scaffolds] */,
                             uint64_t n_scaffolds, const kmx_scaffold_step *steps /* [U] */, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_path *precs /* [n_plinks] */,
                             const uint32_t *psteps, uint64_t n_psteps, const kmx_fill_params *params, char *fseq /* [seq_capacity] or NULL */, uint64_t seq_capacity,
                             uint64_t *foffsets /* [S + 1] */, kmx_scaffold_fill *frec /* [S] */, kmx_fill_step *fsteps /* [U] */, uint32_t *pieces /* [piece_capacity] or NULL */,
                             uint64_t piece_capacity, uint64_t *n_fbases, uint64_t *n_pieces, kmx_fill_stats *stats);
/* The same on DEVICE buffers, read where the scaffold and pair-path calls left them; params, the two counts and stats are on the
 * HOST.  It checks k, U, n_plinks, S <= U, the parameters, NULL and overlap, and validates nothing else; the kernels clamp
 * instead: uoffsets into [0, n_ubases]; step 0 starts a scaffold whatever srec says, and so does every step a first_step < U
 * names; a step with o >= 2 U writes no byte; a link whose lookups fail any bound is an N step, and so is a link beside a
 * unitig shorter than k or with such a unitig on its path; a list that is not ascending is searched all the same.  Every store
 * is checked against S, U, seq_capacity or piece_capacity.  Bad device input gives wrong strings and never an access outside a
 * buffer.  It enqueues the kinds and one scan on the model's stream and waits ONCE, for the counts; steps, records and pieces
 * follow, and the bytes only when that wait has shown that n_fbases fits: 'N' over fseq[0, n_fbases), the steps' own bytes by
 * the tile emit of the contigs with k - 1 bytes skipped at a filled step, then the pieces by a gather emit tiled over the
 * piece bytes, because a repeat unitig is written once per path that crosses it.  A last wait leaves nothing in flight.  Device
 * memory, kept on the handle between calls through the owning types of hip_owned.h: 88 bytes per unitig (2 x 40 for what a step
 * writes and its scan, 8 for where a unitig's bytes go) and 20 per piece, plus the scan's scratch.  The host form also stages
 * its input and output there.                                                                                               */
int kmx_unitig_scaffold_fill_dev(kmx_model *m, int k, const char *d_useq, const uint64_t *d_uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, uint64_t n_ubases,
                                 const kmx_scaffold *d_srec /* [n_scaffolds] */, uint64_t n_scaffolds, const kmx_scaffold_step *d_steps /* [U] */, const kmx_pair_link *d_plinks,
                                 uint64_t n_plinks, const kmx_pair_path *d_precs /* [n_plinks] */, const uint32_t *d_psteps, uint64_t n_psteps, const kmx_fill_params *params /* HOST */,
                                 char *d_fseq /* [seq_capacity] or NULL */, uint64_t seq_capacity, uint64_t *d_foffsets /* [S + 1] */, kmx_scaffold_fill *d_frec /* [S] */,
                                 kmx_fill_step *d_fsteps /* [U] */, uint32_t *d_pieces /* [piece_capacity] or NULL */, uint64_t piece_capacity, uint64_t *n_fbases /* HOST */,
                                 uint64_t *n_pieces /* HOST */, kmx_fill_stats *stats /* HOST */);
/* seconds[4] of the last of these two calls under kmx_set_profile(m, 1): the kinds, the scan with the wait, steps with records
 * and pieces, the bytes */
int kmx_unitig_scaffold_fill_last_phases(kmx_model *m, double *seconds /* [4] */);

/* ---- reduced pair lists: a pair list without the entries that skip a unitig.  The scaffold call joins two unitigs only where a
 * pair link is the one kept edge out of a and the one kept edge into c.  A fragment that is longer than a short unitig b spans
 * it, so the list of kmx_unitig_pair_walks holds a -> b, b -> c and the skipping entry a -> c; then nk(a) = 2 and nk(c ^ 1) = 2,
 * none of the three is a chain link, and the scaffold breaks at exactly the place the pairs describe best.  This call returns the
 * same list without the entries that two other entries explain (its transitive reduction, one unitig deep).
 * kmx_unitig_scaffold, kmx_unitig_pair_paths and kmx_unitig_scaffold_fill consume the result unchanged.  It needs no built model,
 * no session, no bases and no CSR; uoffsets is read only for m_u = len_u - k + 1 (0 for what is shorter than k).
 * Input: k, odd, in [5, 63]; uoffsets[U + 1], U < 2^31; plinks[n_plinks] as kmx_unitig_pair_walks leaves it, n_plinks < 2^31; and
 *   kmx_pair_reduce_params: max_row in [1, 65536], reserved = 0.  All arithmetic is signed 64-bit, two's complement, wrapping.
 *   ELIGIBLE.  Entry i = (a, c, n_pairs, sum_dist, ...) is eligible iff it is a pair link by the scaffold's definition (a < 2 U,
 *     c < 2 U, a >> 1 != c >> 1, n_pairs >= 1) and n_pairs >= min_pairs.  An entry that is no pair link is KMX_REDUCE_IGNORED, a
 *     pair link below min_pairs KMX_REDUCE_BELOW_MIN; neither is examined and neither serves as a witness.
 *   g(i) = inner - 1 - sum_dist / n_pairs (unsigned floor division): the scaffold's g, the windows missing between the two.
 *   TABLE.  Every eligible entry gives two rows, (a, c, i) and (c ^ 1, a ^ 1, i).  The rows are sorted ascending by (src, dst, i).
 *     out(o) is the contiguous run of rows with src = o; first(x, y) is the first row with src = x and dst = y, or none.  In a
 *     canonical list every oriented edge has exactly one row; the definition holds as it stands for the lists that are not
 *     canonical or carry duplicate keys, which the _dev form accepts.
 *   SIDE.  r_a = |out(a)|, r_c = |out(c ^ 1)|; side = 0 if r_a <= r_c, else 1.  min(r_a, r_c) > max_row: KMX_REDUCE_COMPLEX; the
 *     entry stays, with n_via = 0, via = 0xFFFFFFFF and delta = 0 (side and g are reported).
 *   WITNESSES.  On side 0, for every row (a, b, j) of out(a) with F = first(b, c) present:
 *     delta = g(i) - (g(j) + m_(b >> 1) + g(F.i)).  On side 1, for every row (c ^ 1, y, j) of out(c ^ 1), with b = y ^ 1 and
 *     F = first(a, b) present: delta = g(i) - (g(F.i) + m_(b >> 1) + g(j)).  The row is a witness iff -tol <= delta <= tol
 *     (signed).  The entry's own rows never qualify: first(c, c) does not exist.  n_via = the witness rows on the enumerated
 *     side; via = the smallest b over them; delta = the delta of that witness: of the first such row in table order on side 0,
 *     of the last on side 1.
 *   VERDICT.  KMX_REDUCE_TRANSITIVE iff n_via >= 1, otherwise KMX_REDUCE_KEPT.  Every verdict is taken on the INPUT list at once:
 *     a transitive entry still serves as a witness, so no order shows.
 * Output.  rrecs[n_plinks], the records below; for an entry that is not examined g and delta are 0 and via is all ones.
 *   lout[capacity]: every entry whose verdict is not TRANSITIVE, byte-identical and in input order, so a strictly ascending list
 *   stays one; origin[capacity]: origin[j] is the input index of output entry j.  Either may be NULL; with both NULL no list is
 *   built and the call gives the verdicts only (the sizing call: KMX_OK, *n_out what a list would hold).  Otherwise
 *   *n_out > capacity: KMX_E_RANGE with rrecs, stats and *n_out complete and nothing written to lout or origin; capacity =
 *   n_plinks always suffices.  On the HOST in both forms: *n_out and kmx_pair_reduce_stats; n_rows = the rows of the table,
 *   n_examined = the rows enumerated (min(r_a, r_c) summed over the KEPT and TRANSITIVE entries).
 * Consequences:
 *   (a) with min_pairs above every entry, or n_plinks < 3, lout is the input byte for byte;
 *   (b) n_ignored + n_below_min + n_kept + n_transitive + n_complex == n_entries, and n_out = n_entries - n_transitive;
 *   (c) in a canonical list in which no unitig is a witness in both orientations, replacing an entry by its mirror (c ^ 1, a ^ 1)
 *       changes none of verdict, n_via, g, delta for any entry, and changes via only by ^ 1 for that entry;
 *   (d) lout is a valid input for the scaffold, pair-path and fill calls;
 *   (e) three islands of one genome, the middle one shorter than the fragment, come out of kmx_unitig_scaffold on lout as one
 *       scaffold with both holes as runs of 'N' of their true length; on the full list they stay three.
 *   (f) every output is an integer count, sum or minimum and a function of the input alone: byte-identical across runs and forms.
 * Out of scope: crediting a removed entry's pairs to its two witnesses; skips of more than one unitig without the intermediate
 * skips (a -> d with only a -> b -> c -> d stays KEPT); iterating; choosing tol; RF and FF libraries; several GPUs.           */
#define KMX_REDUCE_IGNORED    0
#define KMX_REDUCE_BELOW_MIN  1
#define KMX_REDUCE_KEPT       2
#define KMX_REDUCE_TRANSITIVE 3
#define KMX_REDUCE_COMPLEX    4
typedef struct kmx_pair_reduce_params { uint64_t min_pairs; uint32_t inner, tol, max_row /* [1, 65536] */, reserved /* 0 */; } kmx_pair_reduce_params;   /* 24 bytes */
typedef struct kmx_pair_reduce {         /* one per entry of the list; 32 bytes, no padding */
	uint32_t verdict;                    /* KMX_REDUCE_* */
	uint32_t via;                        /* the smallest witness b, 0xFFFFFFFF for none */
	uint32_t n_via;                      /* the witness rows on the enumerated side */
	uint32_t side;                       /* 0: out(a) was enumerated, 1: out(c ^ 1) */
	int64_t g;                           /* g(i) */
	int64_t delta;                       /* the delta of via's witness */
} kmx_pair_reduce;
typedef struct kmx_pair_reduce_stats { uint64_t n_entries, n_ignored, n_below_min, n_kept, n_transitive, n_complex, n_out, n_rows, n_examined /* rows enumerated */,
                                       reserved; } kmx_pair_reduce_stats;                                               /* 80 bytes */
/* On HOST buffers.  Needs no built model and no session (like kmx_unitig_scaffold); it runs on the model's stream and is a
 * build-class call.  lout and origin may be NULL, plinks and rrecs with n_plinks == 0; every other buffer is required.
 * KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31, n_plinks >= 2^31, max_row outside [1, 65536],
 * reserved != 0, a NULL required buffer, an output that overlaps an input or another output; uoffsets whose first entry is not 0,
 * that decrease, or that give a unitig fewer than k bytes; a list that is not strictly ascending by a << 32 | b.  U == 0: KMX_OK,
 * every entry is IGNORED and lout is the input.  n_plinks == 0: KMX_OK, all counts zero.  KMX_E_NOMEM leaves the handle usable.
 * The call returns when the output is complete.                                                                             */
int kmx_unitig_pair_reduce(kmx_model *m, int k, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const kmx_pair_link *plinks, uint64_t n_plinks,
                           const kmx_pair_reduce_params *params, kmx_pair_reduce *rrecs /* [n_plinks] */, kmx_pair_link *lout /* [capacity] or NULL */,
                           uint32_t *origin /* [capacity] or NULL */, uint64_t capacity, uint64_t *n_out, kmx_pair_reduce_stats *stats);
/* The same on DEVICE buffers, read where the pair call left them; params, *n_out and stats are on the HOST.  It checks k, U,
 * n_plinks, the parameters, NULL and overlap, and validates nothing else; the kernels clamp instead: uoffsets into
 * [0, n_ubases], and the list is taken as it is (not ascending, not canonical, duplicate keys, an entry beside its mirror: the
 * table above is defined for all of them).  Every store is checked against its capacity: bad device input gives wrong verdicts
 * and never an access outside a buffer.  No entry costs more than max_row rows.  It enqueues the rows, one stable radix sort of
 * the 2 n_plinks (key, row) pairs, the verdicts (8 lanes per entry) and the scan of the keep flags on the model's stream and
 * waits once, for *n_out and the counters; the entries that stay are copied only after that wait has shown that they fit, and a
 * last wait behind the copy leaves nothing in flight.  Device memory, kept on the handle between calls through the owning
 * types of hip_owned.h: 60 bytes per entry (2 x (8 + 4) x 2 for the sort's double buffers of the two rows, 4 for the keep flag,
 * 8 for its scan) plus rocPRIM's scratch.  The host form also stages its input and output there.                             */
int kmx_unitig_pair_reduce_dev(kmx_model *m, int k, const uint64_t *d_uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, uint64_t n_ubases, const kmx_pair_link *d_plinks,
                               uint64_t n_plinks, const kmx_pair_reduce_params *params /* HOST */, kmx_pair_reduce *d_rrecs /* [n_plinks] */,
                               kmx_pair_link *d_lout /* [capacity] or NULL */, uint32_t *d_origin /* [capacity] or NULL */, uint64_t capacity, uint64_t *n_out /* HOST */,
                               kmx_pair_reduce_stats *stats /* HOST */);
/* seconds[4] of the last of these two calls under kmx_set_profile(m, 1): the rows, the sort, the verdicts, the scan with the
 * wait and the compaction */
int kmx_unitig_pair_reduce_last_phases(kmx_model *m, double *seconds /* [4] */);

/* ---- lifted pair lists: a pair list with unitig keys and unitig distances, rewritten in the coordinates of the contigs those
 * unitigs were chained into.  kmx_unitig_contigs returns place[u], the contig, strand and k-mer offset of every unitig; the
 * distance of a list entry moves by a constant that depends only on its two unitigs.  So the list that a second mapping of the
 * same pairs onto the contigs would build is a function of the first list, place and the contigs' lengths, and the pairs need
 * not be read and mapped again.  kmx_unitig_scaffold, kmx_unitig_pair_reduce, kmx_unitig_pair_paths and
 * kmx_unitig_scaffold_fill on the contig set consume the result unchanged.  It needs no built model, no session, no bases and no
 * CSR.
 * Input: k, odd, in [5, 63]; uoffsets[U + 1], U < 2^31, read only for m_u = len_u - k + 1 (0 for what is shorter than k); place[U]
 *   and crec[C] as kmx_unitig_contigs left them (of crec only n_kmers is read), C <= U; plinks[n_plinks] as
 *   kmx_unitig_pair_walks leaves it, n_plinks < 2^31; and kmx_pair_lift_params, reserved = 0.  All arithmetic is signed 64-bit.
 *   WHERE AN ORIENTED UNITIG LIES.  o = 2 u + d < 2 U, P = place[u], c = P.oc >> 1, s = P.oc & 1, M = crec[c].n_kmers, m = m_u.
 *     o is PLACED iff c < C, M < 2^32 and P.off + m <= M.  It lies along the oriented contig O(o) = 2 c + (d ^ s), and
 *     start(o) = P.off when d ^ s = 0, else M - P.off - m: the windows of O(o) in front of it.  head(o) = start(o) and
 *     tail(o) = M - start(o) - m, the windows behind it.
 *   CLASS of entry i = (a, b, n_pairs, sum_dist, min_dist, max_dist); the first that applies:
 *   KMX_LIFT_IGNORED   a >= 2 U, b >= 2 U, a >> 1 == b >> 1, n_pairs == 0, or an end that is not placed;
 *   with A = O(a) and B = O(b):
 *   KMX_LIFT_SAME      A == B: both mates lie on one oriented contig.  shift = start(b) - start(a) - m_a + 1, so that the d of
 *                      every pair of the entry at the contig level is its dist + shift.  The entry is FORWARD when
 *                      min_dist + shift >= 0; otherwise its pairs contradict the order of the contig and n_same_back counts it;
 *   KMX_LIFT_INVERTED  A == B ^ 1.  shift = 0;
 *   otherwise shift = tail(a) + head(b), lo = min_dist + shift, hi = max_dist + shift, and
 *   KMX_LIFT_FAR       lo > max_dist (of the parameters) or hi >= 2^32: no pair of the entry is within reach, or the maximum
 *                      cannot be stored;
 *   KMX_LIFT_LINK      otherwise.  It contributes (key, n_pairs, sum_dist + n_pairs * shift wrapping in 64 bits, lo, hi), where key
 *                      is canonical as in the pair call: (A, B) when A << 32 | B is smaller than (B ^ 1) << 32 | (A ^ 1), else
 *                      (B ^ 1, A ^ 1).  The two are never equal: that would be an INVERTED entry.
 * Output.  lout[capacity] with *n_out: the LINK contributions, strictly ascending by key, equal keys folded by sum, sum, minimum
 *   and maximum: exactly a list kmx_unitig_pair_walks could have left for the contig set.  lrec[n_plinks], one record below per
 *   input entry: cls; out, the index of the output entry it was folded into, 0xFFFFFFFF when it is no LINK; A and B before
 *   canonicalisation, 0 for an IGNORED entry; shift (0 when IGNORED); flipped, 1 when a LINK's key is the mirror; reserved = 0.
 *   *n_out > capacity with a list: KMX_E_RANGE with *n_out the number needed, lout untouched, and lrec and stats complete;
 *   capacity = n_plinks always suffices.  lout == NULL with capacity 0 is the sizing call: KMX_OK, *n_out what a list would
 *   hold, lrec and stats complete.  On the HOST in both forms: *n_out and kmx_pair_lift_stats: the entries of each class (n_same
 *   includes the n_same_back backward ones), n_out, the n_pairs of the entries of each class (sums modulo 2^64), pairs_same_back,
 *   and sum_same_d = the sum of (sum_dist + n_pairs * shift) over the FORWARD SAME entries: the lifted d of their pairs.
 * Consequences:
 *   (a) with a place from a contig call that merged nothing (every contig one unitig: c = u, s = 0, off = 0) and
 *       max_dist = 2^32 - 1, lout is the input byte for byte, for a canonical list of pair links;
 *   (b) replacing an entry by its mirror (b ^ 1, a ^ 1) changes A, B and flipped of its record and nothing in lout (head and tail
 *       swap under the mirror, and start(b ^ 1) - start(a ^ 1) - m_b = start(b) - start(a) - m_a); permuting the input entries
 *       (_dev form) changes only the order of lrec;
 *   (c) pairs are conserved: the pairs of the five classes sum to the n_pairs of the input, and the n_pairs of lout to pairs_link;
 *   (d) re-mapping equivalence: for pairs whose every read is one walk on the unitigs and one walk on the contigs, with no pair
 *       FAR at either level, lout equals byte for byte the list kmx_unitig_pair_walks builds when the same pairs are mapped onto
 *       the contigs (same max_dist), and (the sum of d over the SAME pairs on the unitigs) + sum_same_d is the sum of d over the
 *       SAME pairs on the contigs;
 *   (e) every output is an integer count, sum, minimum or maximum and a function of the input alone: byte-identical across runs,
 *       forms and fold variants.
 * Out of scope: lifting to scaffold coordinates (kmx_scaffold_place, base offsets with 'N'); lifting `through` or walks;
 * splitting an entry whose pairs straddle max_dist (the entry is a LINK with its whole count as soon as its nearest pair is
 * within reach); insert-size histograms from SAME entries; several GPUs; choosing max_dist.                                  */
#define KMX_LIFT_IGNORED  0
#define KMX_LIFT_SAME     1
#define KMX_LIFT_INVERTED 2
#define KMX_LIFT_LINK     3
#define KMX_LIFT_FAR      4
typedef struct kmx_pair_lift_params { uint32_t max_dist; uint32_t reserved /* 0 */; } kmx_pair_lift_params;                 /* 8 bytes */
typedef struct kmx_pair_lift {           /* one per entry of the input list; 32 bytes, no padding */
	uint32_t cls;                        /* KMX_LIFT_* */
	uint32_t out;                        /* the entry of lout it was folded into, 0xFFFFFFFF for none */
	uint32_t A, B;                       /* O(a), O(b); 0 when IGNORED */
	int64_t shift;                       /* what the entry's distances move by; 0 when IGNORED or INVERTED */
	uint32_t flipped;                    /* 1: the key in lout is (B ^ 1, A ^ 1) */
	uint32_t reserved;                   /* 0 */
} kmx_pair_lift;
typedef struct kmx_pair_lift_stats { uint64_t n_entries, n_ignored, n_same, n_inverted, n_link, n_far, n_same_back, n_out,
                                     pairs_ignored, pairs_same, pairs_inverted, pairs_link, pairs_far, pairs_same_back;
                                     int64_t sum_same_d; uint64_t reserved; } kmx_pair_lift_stats;                       /* 128 bytes */
/* On HOST buffers.  Needs no built model and no session (like kmx_unitig_pair_reduce); it runs on the model's stream and is a
 * build-class call.  lout may be NULL (with capacity 0); plinks and lrec with n_plinks == 0, place with U == 0 and crec with
 * C == 0; every other buffer is required.  KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31,
 * n_plinks >= 2^31, C > U, reserved != 0, a NULL required buffer, a capacity without a list, an output that overlaps an input or
 * another output; uoffsets whose first entry is not 0, that decrease, or that give a unitig fewer than k bytes; a place[u] that is
 * not placed; a list that is not strictly ascending by a << 32 | b.  n_plinks == 0: KMX_OK, an empty list and all counts zero.
 * U == 0: KMX_OK, an empty list; every entry is IGNORED and counted as such, so that (c) holds.  KMX_E_NOMEM leaves the handle
 * usable.  The call returns when the output is complete.                                                                    */
int kmx_unitig_pair_lift(kmx_model *m, int k, const uint64_t *uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, const kmx_contig_place *place /* [n_unitigs] */,
                         const kmx_contig *crec /* [n_contigs] */, uint64_t n_contigs, const kmx_pair_link *plinks, uint64_t n_plinks, const kmx_pair_lift_params *params,
                         kmx_pair_lift *lrec /* [n_plinks] */, kmx_pair_link *lout /* [capacity] or NULL */, uint64_t capacity, uint64_t *n_out, kmx_pair_lift_stats *stats);
/* The same on DEVICE buffers, read where the contig and pair calls left them; params, *n_out and stats are on the HOST.  It
 * checks k, U, C, n_plinks, the parameters, NULL and overlap, and validates nothing else; the kernels clamp instead: uoffsets
 * into [0, n_ubases]; an end that is not placed (an oc beyond C included) makes the entry IGNORED; and the list is taken as it is
 * (not ascending, duplicate keys, an entry beside its mirror: all of them fold into the same lout).  Every store is checked
 * against its capacity: bad device input gives wrong classes and never an access outside a buffer.  It enqueues the classes,
 * one stable radix sort of the n_plinks (key, index) pairs, the scan of the key changes, the fold and the store on the model's
 * stream and waits once, for *n_out and the counters; the store writes lout only where the merged count fits, which it checks
 * on the device.  Device memory, kept on the handle between calls through the owning types of hip_owned.h: 96 bytes per entry
 * (2 x (8 + 4) for the sort's double buffers, 32 for the shifted item, 32 for the merged record, 8 for the scan) plus rocPRIM's
 * scratch.  The host form also stages its input and output there.                                                           */
int kmx_unitig_pair_lift_dev(kmx_model *m, int k, const uint64_t *d_uoffsets /* [n_unitigs + 1] */, uint64_t n_unitigs, uint64_t n_ubases, const kmx_contig_place *d_place /* [n_unitigs] */,
                             const kmx_contig *d_crec /* [n_contigs] */, uint64_t n_contigs, const kmx_pair_link *d_plinks, uint64_t n_plinks, const kmx_pair_lift_params *params /* HOST */,
                             kmx_pair_lift *d_lrec /* [n_plinks] */, kmx_pair_link *d_lout /* [capacity] or NULL */, uint64_t capacity, uint64_t *n_out /* HOST */,
                             kmx_pair_lift_stats *stats /* HOST */);
/* which fold kernel the next lift calls on the handle run: the segmented reduction inside a wavefront or the plain fold with
 * four atomics per item.  Both give the same bytes; the call exists so that the two can be measured on the same buffers
 * (tools/bench_unitig_pair_lift.py).  A handle starts with the library's default.                          */
#define KMX_LIFT_FOLD_WAVE  0
#define KMX_LIFT_FOLD_PLAIN 1
int kmx_unitig_pair_lift_fold_variant(kmx_model *m, int variant);
/* seconds[4] of the last of the two lift calls under kmx_set_profile(m, 1): the classes, the sort, the scan with the fold, the
 * store with the wait */
int kmx_unitig_pair_lift_last_phases(kmx_model *m, double *seconds /* [4] */);

/* KModel::save(dir) -> header, km.bin, rest.bin (dir must exist)           kmodel.hpp:173-206 */
int kmx_save(kmx_model *m, const char *dir);
/* get_model(save_dir) = header parse + KModel::load                        kmodel.hpp:680-696, :209-235
 * rest.bin with k = 3: KMX_E_ARG; with a prefix longer than k (or not k minus whole groups of 4 bases): KMX_E_IO */
int kmx_load(const char *dir, kmx_model **out);

int kmx_get_stats(kmx_model *m, kmx_stats *st);
/* the same, writing at most `size` bytes: kmx_stats only ever grows at its end, so a caller that passes sizeof of ITS kmx_stats
 * is safe against a newer library (kmx_get_stats and kmx_shard_local write the library's full struct: compare kmx_abi_version()
 * first).  ABI 5 (this header): kmx_stats + query_neighbour_calls / query_accounted; kmx_range_* move regions with in-band
 * headers; piped_* are filled only by builds under kmx_set_profile(m, 2) (since ABI 4).                                    */
int kmx_get_stats_n(kmx_model *m, void *st, uint64_t size);

/* Raw on-disk-layout views for byte-level parity checks (kmodel.hpp:183-202).
 * which: 0 bf[i], 1 bf_back[i], 2 km_back, 3 value array i (bit_array_1), 4 tag array i (bit_array_2),
 *        5 insert-time scratch left in array i (none any more: always zero; kept for the tests' invariant).   */
int kmx_download(kmx_model *m, int which, int index, uint8_t *dst, uint64_t capacity, uint64_t *written);

/* Primitive known-answer surface, evaluated ON THE DEVICE (tools.hpp:16-50, :160-167).
 * hashes[n*n_seeds]: murmur_hash64 of the k-mer string (whole=1) or its (k-2)-mer (whole=0).       */
int kmx_debug_hash(int k, const uint64_t *kmers, uint64_t n, const uint32_t *seeds, int n_seeds, int whole, uint64_t *hashes);
int kmx_debug_min_kmer(int k, const uint64_t *kmers, uint64_t n, uint64_t *out);
/* out[i] = h[i] % d with the device's exact reciprocal modulo (`% length`, kmodel.hpp:378,503,600,633), d up to 2^63 */
int kmx_debug_mod(const uint64_t *h, uint64_t n, uint64_t d, uint64_t *out);
/* Host half of kmx_query_strings / kmx_query_ascii, on its own (no device needed): strings -> packed k-mers
 * (2 bits per base, first base most significant, ceil(len/32) words each, tools.hpp:63-76).  strs != NULL: n separate
 * strings; else n records of `stride` bytes in `flat`.  *clean = 0 when a string holds anything but ACGT (such a
 * batch travels as bytes and is answered by the byte-string kernel).                                */
int kmx_debug_pack_strings(const char *const *strs, const char *flat, int len, int stride, uint64_t n, uint64_t *packed, int *clean);
/* OccuBin tables (occu_bin.hpp:27-83): bin_of_occ[cs+1], mean_of_bin[2^nh]                         */
int kmx_occubin(int cs, int nh, uint32_t *bin_of_occ, uint32_t *mean_of_bin);

/* Random-access ceiling of the memory system for this access pattern: `touches` random touches over
 * `bytes` of device memory, 8 per lane like one k-mer on one array; seconds per launch out.  mode: 0 8-byte loads,
 * 1 64-bit atomic OR (agent scope, what the insert uses), 2 byte stores, 3 byte loads, 4 8-byte stores,
 * 5 32-bit atomic OR (what the insert uses on its 4-byte cells), 6 64-bit atomic OR at workgroup scope, 7 64-bit atomic OR
 * returning the old word, 8 4-byte loads (what the insert's check uses); 9 / 10 / 11 the same non-temporal / agent-scope
 * (sc1) / with 16 loads in flight per lane; 12 32-bit atomic OR with 3/8 of the lanes active (`touches` counts all lanes);
 * 20 modes 8 and 5 side by side on two streams, each on its own buffer of `bytes` (seconds until both are done).          */
int kmx_microbench(int mode, uint64_t bytes, uint64_t touches, int iters, double *seconds);

/* Per-kernel-class timing with HIP events recorded on the model's stream around each launch (off by default).
 * classes: 0 classify(+Bloom insert) 1 check (+ claim emission) 2 commit 3 ordered slow path 4 reorder 5 rest table (sort + index) 6 query
 * 7 detect (opposite claims) 8 commit of the previous round beside the check of the next (k_round_commit_check)
 * 9 file (k_round_file).  seconds[KMX_KERNEL_CLASSES], launches[KMX_KERNEL_CLASSES] accumulate until reset: a caller
 * must size both arrays with the macro of the header it was compiled against and check kmx_kernel_classes() == it.  */
#define KMX_KERNEL_CLASSES 10
int kmx_kernel_classes(void);           /* what this library writes: KMX_KERNEL_CLASSES of ITS header */
/* on = 1: time the kernel classes of the next builds / queries; on = 2: no timing, but the fused launches of the next builds
 * run their ACCOUNTING variant (kmx_stats piped_*: what they examined, committed and issued) -- it is slower than the
 * product's kernel, so it is never the one that is timed; 0: neither                                                    */
/* (any other value: KMX_E_ARG)                                                                                          */
int kmx_set_profile(kmx_model *m, int on);
int kmx_get_kernel_times(kmx_model *m, double *seconds, uint64_t *launches, int reset);

/* timing of the last build with HIP events on the model's stream: total_s = whole build call;
 * insert_kernels_s = time inside the insert kernels (only collected while kmx_set_profile is on, else 0) */
int kmx_last_build_seconds(kmx_model *m, double *insert_kernels_s, double *total_s);

#ifdef __cplusplus
}
#endif
#endif
