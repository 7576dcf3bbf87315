// kmx_types.h -- plain structs passed by value from the host orchestration to the gfx950 kernels.
#pragma once
#include "device_common.h"

// Everything a kernel needs to address the model in HBM (A.1-A.3 of SURVEY.md).
struct ModelDev {
	int k, nh, nb, ci, cs, bf_num;
	int nh_first, nh_second;                   // the check gathers positions [0, nh_first) first, then [nh_first, nh_second), then the rest -- each group only if no earlier one conflicts
	StrGeom gfull, gback;                      // geometry of the k-mer and (k-2)-mer strings
	u32 *bf[3];      ModU64 bf_mod[3];         // Bloom filters, on-disk byte layout (kmodel.hpp:250,253)
	u32 *bf_back[3]; ModU64 bf_back_mod[3];    // their (k-2)-mer back filters       (kmodel.hpp:251,255)
	u32 *km_back;    ModU64 km_back_mod;       // back filter of the coupled arrays  (kmodel.hpp:267-269)
	cell_t *cells[KMX_MAX_NB];                 // coupled arrays, cell layout (device_common.h)
	ModU64 km_mod;                             // bit_array_length                   (kmodel.hpp:33,445)
	int bloom_direct;                          // 1: Bloom-class k-mers OR their bits in right away; 0: through the BitScatter of the Bloom slab
	u64 bf_woff[3], bf_back_woff[3];           // word offsets of the filters inside the slab (they are allocated back to back)
	int kmb_direct;                            // 1: a success ORs its (k-2)-mer into km_back right away (atomics); 0: the bits are
	                                           // scattered round by round through a BitScatter (k_kmback_emit / k_bs_apply)
	const u32 *bin_of_occ;                     // occ -> bin  (occu_bin.hpp:67-77)
	const u32 *mean_of_bin;                    // bin -> mean (occu_bin.hpp:79-83)
	// exact rest table (rest.hpp), device form: suffixes as integers instead of byte rows
	int rest_pre_len, rest_W;
	u64 rest_entries;
	const int *rest_h2i;                       // hash2index[4^pre_len]
	const int *rest_pre;                       // pre_buffer[groups+1]
	const u64 *rest_suf;                       // [entries][W] suffix value (low 2*(k-pre_len) bits)
	const int *rest_cnt;                       // count_bin[entries]
	// device-only accelerators of the lookup (same answers as the reference's binary search, far fewer touches)
	int rest_fbits;                            // F: rows are bucketed by the top F bits of the 2k-bit k-mer
	const u32 *rest_fine;                      // [2^F + 1] first row of every bucket
	const u64 *rest_q;                         // [4^pre_len][W] suffix of the first row of the NEXT group (the one row the
	                                           // reference's inclusive upper bound can still match), all-ones if none
};

// Partitioned bit-set into one order-free filter (set_bit is an OR, kmodel.hpp:576-581): producers append the bit
// addresses they want set to BS_BINS position-range bins (LDS-staged runs, bs_block_emit); k_bs_apply then sweeps the
// filter bin by bin, tile by tile: the bits of a tile are collected in LDS and the tile is OR-ed back with whole-word
// coalesced accesses -- streaming traffic instead of one random read-modify-write per bit.
#define BS_BINS 256
#define BS_TILE_WORDS (1u << 15)               // 2^15 words = 128 KB of LDS = 2^20 positions per tile
struct BitScatter {
	u32 *words;              // the filter (32-bit words; bit p of the filter = bit bit_in_word32(p) of word p >> 5)
	u64 nwords;
	u32 wshift;              // log2(positions per bin): bin = address >> wshift (a power of two of words, at most 2^32 positions)
	u32 cap;                 // tuples per bin; a producer that finds its bin full sets the bit with an atomic instead
	u32 *tup;                // [BS_BINS][cap] bit offsets inside the bin: (word - bin start) << 5 | bit in word
	int *cnt;                // [BS_BINS], reset by k_bs_apply
	u32 tlog2;               // log2(positions per tile), <= 20 (smaller only under the KMX_BS_TILE_LOG2 test hook)
	// second level, for bins of more than 8 tiles (filters above 256 MB): k_bs_split deals a bin's tuples to its tiles,
	// k_bs_apply2 sweeps one tile per workgroup -- every tuple and every word of the filter is then read once per sweep
	u32 cap2;                // tuples per (bin, tile); 0 = single level
	u32 *tup2;               // [BS_BINS << (wshift - tlog2)][cap2] bit offsets inside the tile
	int *cnt2;               // [BS_BINS << (wshift - tlog2)], reset by k_bs_apply2
};
// km_back tuples a finished block still owes (the whole-block form of k_kmback_emit): hosted by the finisher launches of
// the NEXT block's first two rounds -- one workgroup per list, the rest of the chip idle (k_slow_finish)
struct KmbackJob {
	const u64 *kmers;            // the finished block's k-mers (its staging region, identity order)
	const unsigned char *surv;   // its survivor flags (the other half of the double buffer)
	int n_in_block;
	int i0, n_lists;             // this launch emits lists [i0, i0 + n_lists) of that block; n_lists == 0: nothing hosted
};
#define BS_MAX_TILES_LOG2 8                    // tiles per bin at most, two-level (the split counts them in 256 LDS counters)

// Raw KMC records on the device (k_kmc_decode): fixed-size [suffix bytes big-endian | counter bytes little-endian];
// record r carries the prefix idx & prefix_mask of the LUT entry with lut[idx] <= r < lut[idx + 1] (kmc_file.cpp:439-478).
struct KmcDecode {
	const unsigned char *recs;   // records of this batch
	const u64 *lut;              // n_lut entries + sentinel
	u64 n_lut, prefix_mask;
	u32 rec_bytes, suf_bytes, cnt_bytes;
};

// device-side statistics (one u64 each)
enum { ST_ATTEMPTS = 0, ST_SUCCESSES, ST_SLOW_SUCC, ST_CONTENDED, ST_FIN_ITERS, ST_BAD_COUNT, ST_MAX_U0, ST_MAX_UFIN,
       ST_PIPE_ATTEMPTS, ST_PIPE_SUCC,        // attempts examined / winners committed inside fused commit|check launches (accounting only)
       ST_PIPE_GATHERS, ST_PIPE_ATOMICS,      // random 4-byte loads / 32-bit atomic ORs issued inside those launches (the staged fetch stops early; one atomic per NEW tag bit)
       ST_MAX_LATE_BIN,                       // fullest claim bin of a late round (t >= 2) since the last block: picks the form of their k_round_detect
       ST_DELTA_FAILS,                        // candidates of a stale check that a still-uncommitted winner of the previous visit ruled out (k_round_detect)
       ST_QUERY_NEIGH, ST_QUERY_N,            // accounting queries (kmx_set_profile(m, 2)): how many entered the neighbour disambiguation / were asked
       ST_N };

#define KMX_CLS_TILE 2048                      // k-mers per classification tile (front end)
#define KMX_RSIZE_LOG2 20
#define KMX_RSIZE (1u << KMX_RSIZE_LOG2)      // reservation slots per list (ordered slow path)
#define KMX_FIN_RPT(NHM) ((NHM) <= 8 ? 2 : 1)      // records per finisher thread kept in registers (1024 threads)
#define KMX_FIN_RANGES 8                        // the finisher takes up to this many register loads, in index ranges
#define KMX_APPLY_WGS 8                         // extra workgroups per list in k_reorder that apply the finisher's decisions
enum { KMX_ROUND_FIN_GLOBAL = 1, KMX_ROUND_RESOLVE_GATHER = 2,     // test hooks of kmxk::round (older code paths)
       KMX_ROUND_PENDING = 4,                                        // the previous round's winners are not committed yet: their commit rides with this round's check
       KMX_ROUND_KEEP = 8,
       KMX_ROUND_SMALL_DETECT = 16 };                               // rounds t >= 2: k_round_detect with small tables (their bins hold a few hundred tuples)                                         // this round's winners will be committed beside the next round's check (its detect re-reads the claims)
#define KMX_NSLOW 2                            // contended-record levels, ping-pong: pass s reads level s&1, defers to (s+1)&1
#define KMX_MAX_NSUB 16                        // most grid-wide ordered passes per round
#define KMX_CTR_STRIDE 32                      // ints between per-list counters: one 128-byte line each (same-line atomics serialise)
#define UN_IDX(s, i, nb) ((((s) * (nb)) + (i)) * KMX_CTR_STRIDE)
#define KMX_TILE 1024                          // slots per reorder tile
#define KMX_NTILES (KMX_BUCKET / KMX_TILE)

// Working set of one nb*2^18 block (kmodel.hpp:508-573): lists are index permutations into the block.
struct BlockDev {
	const u64 *kmers;        // [nb*BUCKET][W] this block's k-mers in listing order (buffer i = slice i)
	const u32 *counts;       // [nb*BUCKET]
	// Lists are index permutations, ping-pong by round parity pp.  An entry with bit 31 set is a hole of the last
	// reorder that has not been filled yet: its value is mover[pp][entry & 0x7FFFFFFF] (resolved by check_emit).
	u32 *list[2];            // list[pp][i*BUCKET + x] = index into buffer i of slot x
	u32 *mover[2];           // mover[pp][i*BUCKET + r] = r-th survivor from the right of the previous round
	int *n[2];               // n[pp][i] current list lengths (buff_real_n, kmodel.hpp:277)
	int *tile_cnt[2];        // tile_cnt[pp][i*NTILES + tile] survivors (failed slots) per 1024-slot tile, counted as they fail
	// Per-slot state of a round, double-buffered by the round parity pp like the lists: the winners of round r are committed
	// beside the check of round r+1 (k_round_commit_check), which writes the other half.
	unsigned char *status[2]; // [nb*BUCKET] per slot: 0 undecided -- after the round: a winner nobody contended, committed one round
	                          // later from cidx/cnib/want --, 1 failed (survivor), 2 inserted by the ordered path, 3 contended (transient)
	unsigned char *dfail;    // [nb*BUCKET] set by k_round_detect: a winner of the previous visit to the array, not yet committed when
	                          // this slot was checked, holds one of its positions with the other value; k_round_file makes it a failure
	unsigned char *surv;     // [nb*BUCKET] per k-mer of the block: 1 = it went to the rest table (k_rest_append); the others were inserted
	// contended k-mers; level (s & 1) = still undecided after s grid-wide resolve passes.  A record carries what the
	// ordered slow path needs -- word 0 = slot | bin << 32, then the W packed k-mer words -- so that its latency-bound
	// kernels reach the cells after ONE dependent load.
	u64 *Urec[KMX_NSLOW];    // [nb*BUCKET][1 + W]
	int *Un;                 // [KMX_NSLOW*nb*KMX_CTR_STRIDE], use UN_IDX
	u64 *R;                  // [nb*KMX_RSIZE] epoch-tagged reservations
	u64 *stats;              // [ST_N]
	// claims of a round as a partitioned stream (k_round_check_emit -> k_round_detect -> k_round_commit)
	u32 *uw[2];              // [nb*BUCKET] per candidate: positions it saw untagged (bit j = hash j) | values it wants there << 16 (= its occurrence bin)
	u32 *crec[2];            // [nb*BUCKET][crec_words(nh)] per candidate: cell index of every position + their low 4 bits (kernels.hip CRec)
	u64 *cl_tup[2];          // [nb][bins][KMX_CL_CAP] claim tuples, hash-partitioned by position
	int *cl_cnt[2];          // [nb][KMX_CL_MAXBINS] tuples per bin; a round's counts are reset by the NEXT round's k_round_detect, which reads
	                         // the tuples once more as the delta of the still-uncommitted winners
	int *cl_ovf;             // [nb] a bin of the list overflowed: every candidate of the round takes the ordered path (reset by k_reorder)
	unsigned char *rverdict; // position-range partition, owner's view only: the verdict bytes of the triples it received this round -- a claim
	                         // on a position wanted with both values is reported there (k_round_detect<..., RANGE>); null elsewhere
};

// claim partition: bins per list and slots of the LDS table of one bin (kernels.hip, "claims as a partitioned stream")
#define KMX_CL_BINS_LOG2(NHM) 8
#define KMX_CL_BINS(NHM) (1 << KMX_CL_BINS_LOG2(NHM))
#define KMX_CL_MAXBINS 256
// a position is identified inside a bin by the rest of a bijective 36-bit mix of it (kernels.hip cl_mix): exact for arrays
// of up to 2^36 positions (2e10 coupled k-mers at nh = 7) -- beyond that winners are committed before the next check
#define KMX_CL_MIX_BITS 36
// tuples per bin: 2^18 * nh / bins at most on average (7168 at nh = 7, 16384 at nh = 16), + 25 % and more
#ifndef KMX_CL_CAP                             // (tools/stress_small_tables.py builds a library with a tiny capacity: the overflow path every round)
#define KMX_CL_CAP_OF(NHM) ((NHM) <= 8 ? 12288 : 20480)
#else
#define KMX_CL_CAP_OF(NHM) KMX_CL_CAP
#endif
// 2^TBITS > capacity slots: the table of a bin can always take every tuple.  64 KB of LDS at nh <= 8: two 1024-thread
// workgroups per CU, so one's loads run under the other's table phase
#define KMX_CL_TBITS(NHM) ((NHM) <= 8 ? 14 : 15)
#define KMX_CL_TBITS_SMALL 12                  // the late rounds' form: 16 KB, 256 threads; takes bins of up to 3072 tuples

#define LIST_HOLE 0x80000000u

// One list of a multi-GPU ring round (kernels.hip, k_ring_import / k_ring_export), indexed by list number.
#define KMX_MSG_HDR 8                          // u64 words of message header; word 0 = number of entries
struct RingList {
	int active;              // this rank attempts the list this round
	int n_host;              // >= 0: entries, known on the host (fresh from the stream); < 0: read from the message header
	const u64 *src_kmers;    // n_host >= 0
	const u32 *src_counts;
	const u64 *src_msg;      // n_host < 0: message received from the rank that owns the previous array
	u64 *dst_msg;            // survivors of the round as a message; null in the last round (they go to the rest table)
};
struct RingLists { RingList e[KMX_MAX_NB]; };

// ---- the position-range partition of the coupled arrays over several GPUs (range_kernels.h)
#define KMX_MAX_RANKS 16
#define KMX_RANGE_HDR 4                        // u32 words of a region's header: commits, triples, bulk commits (the first part of the commits, complete early), pad
#define KMX_RANGE_QBITS 27                     // a claim tuple on the owner names the received triple it came from in this many bits (kernels.hip CL_RANGE_TUPLE)
struct RangePlan {
	int rank, world;
	u64 cell_lo[KMX_MAX_RANKS + 1];   // rank q owns the cells [cell_lo[q], cell_lo[q+1]) -- 16 positions each -- of every array
};
// Between a list rank and an owner lies one REGION of `cap` 64-bit words: the winners' commits of a round in front, the next
// round's triples behind them, a header {commits, triples} beside it.  The list rank's side:
struct RangeDev {
	u64 *out[KMX_MAX_RANKS];             // out[q]: the region for owner q -- this rank's own memory (the caller moves the words) or owner q's inbox through a peer mapping
	u32 *hdr_out[KMX_MAX_RANKS];         // hdr_out[q][0..2]: where the header {commits, triples, bulk commits} of that region is left for owner q
	const unsigned char *vin[KMX_MAX_RANKS];   // vin[q][off]: verdict byte of word `off` of the region for owner q
	int *ccnt, *tcnt;        // [KMX_MAX_RANKS * KMX_CTR_STRIDE] commits / triples per destination written since the last seal
	u64 cap;                 // words a region takes.  The worst case of a round (nothing is ever dropped) -- or, when the regions travel as
	                         // fixed-size messages, what the transport ships: a word beyond it is DROPPED and *ovf raised (the build is void:
	                         // the caller repeats it with counted messages; uniform hashing makes that a once-in-never event)
	int *ovf;
	u32 *tidx;               // [nb*BUCKET][nh] where the triple of hash j of a slot went: destination << 28 | index in its region
	u32 *contended;          // [nb*BUCKET] slots of the contended candidates of a list (any order)
	int *n_contended;        // [KMX_MAX_NB * KMX_CTR_STRIDE]
	// k_range_resolve: exact position table per held list (2^rt_bits entries), per-record scratch
	u64 *rt_key;
	u32 *rt_resv, *rt_mark;
	u32 *rt_eidx;            // [nb*BUCKET][nh]
	u32 *rt_um;              // [nb*BUCKET] per contended record (same index as `contended`): its positions wanted with both values
	u32 rt_bits;
};
// which commit words of a region: all, the BULK (the uncontended winners', complete when k_range_apply ends -- the sender still
// orders its contended candidates then) or the LATE ones behind them (k_range_resolve's)
enum { RANGE_ALL = 0, RANGE_BULK = 1, RANGE_LATE = 2 };
// ... and the owner's: what it received from every sender, and where the verdict bytes go
struct RangeIn {
	const u64 *reg[KMX_MAX_RANKS];       // region of sender s
	unsigned char *vout[KMX_MAX_RANKS];  // vout[s][off]: where sender s reads the verdict of word `off` of its region (its own memory, possibly through a peer mapping)
	const u32 *hdr;                      // hdr[hdr_stride s + 0 .. 2]: commits / triples / bulk commits of region s, in device memory (in band) -- or null and
	u32 nc[KMX_MAX_RANKS], nt[KMX_MAX_RANKS];   // the counts by value (the caller moved the words and knows them)
	u32 hdr_stride;                      // u32 words between the headers of consecutive regions
	u32 cap;                             // words of a region that arrived (0: all of them): the counts of a header are cut to it
	int world;
};

// the pre-gather probe of kmxk::round (test hook)
struct RoundProbe {
	bool on;
	hipStream_t side;
	hipEvent_t fork, done;
	u32 *sink;
};

// The two argument blocks of the launchers that work along sequences (launchers.h); they unpack them into the kernels' parameters.
// Which bases a launch holds: seq[0] is the base at position g0 of an input of n_total bases, [g0, g1) is on hand, and the
// n_seqs + 1 offsets are in those positions (of the whole input, whatever part of it seq holds).
struct SeqView {
	const unsigned char *seq;
	u64 g0, g1, n_total;
	const u64 *offs;
	u64 n_seqs;
};
// The dirty list of one piece: the windows with a byte outside ACGT, which the piece's first launch appends to list[*cnt++]
// and its second launch answers.  list needs cap entries, one per window of the piece; *cnt is 0 on entry; the second launch
// zeroes *cnt_next, the counter of the NEXT piece, so consecutive pieces alternate between two counters.
struct SeqDirty {
	u32 *list;
	u32 cap;
	u32 *cnt, *cnt_next;
};

// kmx_summarise_seqs: one record per sequence, the layout of kmx_seq_summary (include/kmx.h; kmx_api.hip asserts it) ...
struct SeqSummary {
	u64 n_windows, sum;
	int mn, mx;
	u64 n_ge[3];
	u64 first_below, last_below;
};
// ... and what the kernels that fold windows into the records take by value.  Between k_seq_summary_init and
// k_seq_summary_finish a record holds mn = INT_MAX, first_below = ~0 until a window is folded in (below thr[0]).
struct SeqSumDev {
	SeqSummary *rec;
	int thr[3];
	int n_thr;
};

// kmx_correct_seqs: one record per sequence, the layout of kmx_seq_correction (include/kmx.h; kmx_api.hip asserts it) ...
struct SeqCorrection {
	u64 n_windows, n_weak, n_runs, n_sites, n_corrected, n_ambiguous, n_unfixable, reserved;
};
// ... and where the kernels of one piece leave what they decide (correct_kernels.h).  A corrected byte goes to out[b]
// (positions of the offsets; the device variant) or, as (b - p0) << 2 | code, to fix[2 + fix[0]++] (the host variant:
// fix[0] is zero before the piece; the host sizes fix_cap for the worst case of a piece, checks the count it reads back and
// fails the call if it ever exceeds fix_cap, so an entry the kernel had no room for is never lost silently).  rec may be null.
struct CorrDev {
	SeqCorrection *rec;
	unsigned char *out;
	u32 *fix;
	u32 fix_cap;
	int thr, min_support;
};
#define KMX_CORR_HALO(k) (2 * (k) + 2)         // windows of weak bits a piece needs beyond each of its ends

// kmx_edit_seqs: one record per sequence, the layout of kmx_seq_edits (include/kmx.h; kmx_api.hip asserts it) ...
struct SeqEdits {
	u64 n_windows, n_weak, n_runs, n_sites, n_sub, n_del, n_ins, n_ambiguous, n_unfixable, out_len;
};
// ... and where k_edit_sites leaves what it decides (edit_kernels.h): an edit goes to edits[(*count)++] as a kmx_edit when
// there is room; *count is zero before the first piece and counts every edit found.  rec may be null.
struct EditDev {
	SeqEdits *rec;
	u64 *edits;
	u64 cap;
	unsigned long long *count;
	int thr, min_support, ops;
};

// kmx_polish_seqs: one record per sequence, the layout of kmx_seq_polish (include/kmx.h; kmx_api.hip asserts it) ...
struct SeqPolish {
	u64 n_passes, converged, n_sub, n_del, n_ins, out_len, n_windows, n_weak, n_runs, n_sites, n_ambiguous, n_unfixable;
};
// ... what one pass hands the next (polish_device.hip): the reads that go on, their bytes after the edits, the bytes of the
// reads that retire into this pass's parking area.  The host reads the totals where it reads the pass's edit count.
struct PolishTri {
	u64 n, next, park;
};
// ... and where a retired read lies: home[i] = area << 56 | offset, area 0 the caller's input (a read that pass 1 left alone
// stays there), area p the parking area of pass p, POLISH_HOME_PLACED: already written to its place in the output
enum { POLISH_MAX_PASSES = 16, POLISH_HOME_SHIFT = 56, POLISH_HOME_PLACED = 255 };
struct PolishHomes {
	const unsigned char *area[POLISH_MAX_PASSES + 1];
};

// kmx_extend_seqs: one record per seed, the layout of kmx_seq_extension (include/kmx.h; kmx_api.hip asserts it) ...
struct SeqExtension {
	u32 n_ext, stop;
	int seed_occ, min_occ, max_occ;
	u32 n_lookahead;
	u64 sum_occ;
};
enum { EXT_DEAD_END = 1, EXT_BRANCH = 2, EXT_JOIN = 3, EXT_CYCLE = 4, EXT_MAX_EXT = 5, EXT_BAD_SEED = 6 };   // KMX_EXT_* of kmx.h
// ... a walk between two launches (extend_kernels.h): the k-mer it stands on, the seed's k-mer, the record so far
// (one word each for k <= 32) ...
struct ExtWalk {
	u64 cur[2], first[2];
	SeqExtension r;
};
// ... and what the kernels of one chunk of seeds take by value: walk, rec (may be null) and ext (rows of max_ext bytes, zero
// on entry) are the chunk's, indexed by the seed's place in it
struct ExtDev {
	ExtWalk *walk;
	SeqExtension *rec;
	unsigned char *ext;
	int thr;
	u32 max_ext;
	int depth;
};

// kmx_unitigs: one record per unitig, the layout of kmx_unitig (include/kmx.h; kmx_api.hip asserts it) ...
struct Unitig {
	u64 n_kmers, sum_count;
	u32 min_count, max_count;
	u64 first_node;
	unsigned char circular, n_pred, n_succ, first_fwd, reserved[4];
};
// ... what the scan of the emit adds up per listing entry (unitigs that start there, their bytes) ...
struct UniTot {
	u64 n, len;
};
// ... and the work arrays of one call (unitig_kernels.h), views of the handle's buffers.  An ORIENTED node is 2 i + s: listing
// entry i, s = 0 as listed (canonical), s = 1 its reverse complement; UNI_NONE = no such node.  n < 2^31, so it fits 32 bits.
#define UNI_NONE 0xFFFFFFFFu
enum { UNI_DEG_NODE = 0x40, UNI_DEG_CIRC = 0x80 };              // deg[i] = |succ| | |pred| << 3 of the listed orientation, | these
struct UniDev {
	const u64 *km;               // the listing: [n][W] k-mers, [n] counts
	const u32 *cnt;
	u64 n;
	int k, W, bits, shift;       // start[] is indexed by the top `bits` bits of the 2k-bit k-mer = k-mer >> shift
	u32 thr;
	u32 *start;                  // [2^bits + 1]: the first entry whose prefix is at least p
	u32 *succ1, *pred1;          // [n]: the only successor / predecessor of the listed orientation, or UNI_NONE
	unsigned char *deg;          // [n]
	u32 *err;                    // [1]: the listing is not strictly ascending, not canonical, or wider than 2k bits
};
// ... and the graph a cleaning round decides on (kmx_*unitig_graph_clean*): what the two emits wrote for the working counts.  A
// verdict is 0 or the KMX_CLEAN_* bit of what removes the unitig.
enum { UNI_CLEAN_TIPS = 1, UNI_CLEAN_ISLANDS = 2, UNI_CLEAN_BUBBLES = 4 };
struct UniClean {
	const Unitig *rec;           // [n_uni]
	const u64 *loffs;            // [2 n_uni + 1]
	const u32 *links;            // [n_links]
	u64 n_uni, n_links;
	u32 ops, max_tip, max_bubble;
};
// kmx_unitig_map_*: a segment and a per-read record, the layouts of kmx_map_segment and kmx_seq_map (include/kmx.h; map_host.h
// asserts them) ...
struct MapSeg {
	u64 pos;
	u32 n_windows, o, off, reserved;
};
struct SeqMap {
	u64 n_windows, n_mapped, n_segments, n_gaps, first_mapped, last_mapped, longest, reserved;
};
// ... the index of a session (map_kernels.h): the listing with its bucket index (d: km, n, k, W, bits, shift, start, err), the
// place of every entry, u << 32 | f << 31 | j or MAP_NONE, and the windows of every unitig ...
#define MAP_NONE (~0ULL)
struct MapDev {
	UniDev d;
	u64 *place;                  // [n]
	u32 *mu;                     // [U]
	u64 U;
};
// ... and the work arrays of one chunk of at most `cap` windows.  A window's code is o << 32 | off, or MAP_NONE when it is not
// mapped; code[0] is the window in front of the chunk (what the previous chunk left), code[1 + i] window p0 + i.
struct MapChunk {
	u64 *code;                   // [cap + 1]
	u32 *ex;                     // [cap + 1]: the exclusive scan of the start flags; ex[n_win] their number
	u64 *spos;                   // [cap]: where the chunk's l-th segment starts
	u64 *state;                  // [2]: segments in front of the chunk; the start of the last segment begun so far
};
// ... and where the segments and what is kept per read go: segs[cap] (may be null), so[n_seqs + 1] (counts, scanned at the
// end), rec[n_seqs] (may be null)
struct MapOut {
	MapSeg *segs;
	u64 cap;
	u64 *so;
	SeqMap *rec;
};
// kmx_unitig_walk_segs*: a walk, the layout of kmx_walk (include/kmx.h; map_host.h asserts it) ...
struct Walk {
	u64 pos, n_span, n_mapped, n_covered, first_seg, first_step;
	u32 n_segs, n_steps, off_first, off_last, n_inside, n_across;
	int indel;
	u32 reserved;
};
// ... the scanned pair per segment: the walks and the steps that start in front of it ...
struct WalkTot {
	u64 w, s;
};
// ... what a segment's flag byte says of it and of the join with its predecessor ...
enum { WALK_START = 1, WALK_STEP = 2, WALK_EDGE = 4, WALK_INSIDE = 8, WALK_ACROSS = 16 };
// ... the counters of a call, in the order of kmx_walk_stats behind n_walks and n_steps ...
enum { WALK_C_EDGE = 0, WALK_C_INSIDE, WALK_C_ACROSS, WALK_C_UNLINKED, WALK_C_BREAKS, WALK_C_N };
// ... and the input, the work arrays (flag[n_segs], join[n_segs] = overlap << 16 | (d & 0xFFFF), sc[n_segs + 1], cnt[WALK_C_N])
// and the output of one call (walk_kernels.h).  Every array of the caller is read and written under the bounds given here.
struct WalkDev {
	const MapSeg *segs;
	u64 n_segs;
	const u64 *so;               // [n_seqs + 1]
	u64 n_seqs;
	const u64 *loffs;            // [2 U + 1]
	const u32 *links;            // [n_links]
	u64 n_links;
	const u32 *mu;               // [U]
	u64 U;
	int k;
	u32 max_gap, max_indel;
	unsigned char *flag;
	u32 *join;
	WalkTot *sc;
	unsigned long long *cnt;
	Walk *walks;                 // [walk_cap], null with walk_cap = 0 in the sizing call
	u64 walk_cap;
	u64 *wo;                     // [n_seqs + 1]
	u32 *steps;                  // [step_cap]
	u64 step_cap;
	unsigned long long *link_hits;   // [n_links] or null
};
// kmx_unitig_contigs*: a contig and a unitig's place, the layouts of kmx_contig and kmx_contig_place (include/kmx.h; contig_host.h
// asserts them) ...
struct Contig {
	u64 n_kmers, sum_count;
	u32 min_count, max_count;
	u64 first_step;
	u32 n_steps;
	unsigned char circular, n_pred, n_succ, reserved;
	u64 min_support, sum_support, reserved2;
};
struct CtgPlace {
	u32 oc, off;
};
// ... the rank state of an oriented unitig (a head points at itself with steps == 0): the steps and the k-mers from ptr to here ...
struct CtgRank {
	u32 ptr, steps;
	u64 kmers;
};
// ... what the scan of the marks adds up per unitig: the contigs that start there, their bytes, their steps ...
struct CtgTot {
	u64 n, len, steps;
};
// ... the counters of a call, the first five in the order of kmx_contig_stats ...
enum { CTG_C_LINKS = 0, CTG_C_KEPT, CTG_C_BELOW_MIN, CTG_C_BELOW_RATIO, CTG_C_CHAIN, CTG_C_CIRCULAR, CTG_C_MULTI, CTG_C_N };
// ... and the input, the work arrays and the output of one call (contig_kernels.h).  Every array of the caller is read and
// written under the bounds given here: U, n_ubases, n_links.
struct CtgDev {
	int k;
	u64 U, n_ubases, n_links;
	const unsigned char *useq;   // [n_ubases]
	const u64 *uoffs;            // [U + 1]
	const Unitig *urec;          // [U] or null
	const u64 *loffs;            // [2 U + 1]
	const u32 *links;            // [n_links]
	const u64 *hits;             // [n_links]
	u64 min_reads;
	u32 ratio;
	u64 *esup;                   // [n_links]: sup(e)
	unsigned char *ekeep;        // [n_links]: 1 iff e is kept
	u64 *best;                   // [2 U]
	unsigned char *nk;           // [2 U]: |outK[o]|
	u32 *only;                   // [2 U]: the one kept target, or CTG_NONE
	u64 *supo;                   // [2 U]: its support
	unsigned char *circ;         // [U]: the unitig lies on a cycle of chain links
	CtgTot *sc;                  // [U + 1]: the scanned marks
	u64 *ubase;                  // [U]: where the oriented string of u starts in cseq | CTG_REV | CTG_FIRST
	u64 *clc, *clsc;             // [2 U + 1] each: the kept edges at the end of every oriented contig, and their scan
	u32 *last;                   // [2 U]: the last step of every oriented contig
	unsigned long long *cnt;     // [CTG_C_N]
	unsigned char *cseq;         // [n_ubases]
	u64 *coffs;                  // [U + 1]
	Contig *crec;                // [U]
	u32 *steps;                  // [U]
	CtgPlace *place;             // [U]
	u64 *cloffs;                 // [2 U + 1]
	u32 *clinks;                 // [n_links]
	u64 *csup;                   // [n_links]
};
// kmx_unitig_walk_through*: the counters of a call, in the order of kmx_through_stats behind n_walks and n_steps ...
enum { THR_C_INTERIOR = 0, THR_C_ADDED, THR_C_MISSING, THR_C_N };
// ... and the input, the work arrays (mark[n_steps + 1]: 1 where a walk starts; cnt[THR_C_N]) and the output of one call
// (resolve_kernels.h).  Every array of the caller is read and written under the bounds given here.
struct ThroughDev {
	const Walk *walks;           // [n_walks]: only first_step is read
	u64 n_walks;
	const u32 *steps;            // [n_steps]
	u64 n_steps;
	const u64 *loffs;            // [2 U + 1]
	const u32 *links;            // [n_links]
	u64 n_links, U;
	unsigned char *mark;
	unsigned long long *cnt;
	unsigned long long *through; // [16 U], added to
};
// kmx_unitig_resolve*: a unitig's place in the resolved set, the layout of kmx_resolve_place (include/kmx.h; resolve_host.h asserts it) ...
struct ResPlace {
	u32 first, n_copies;
};
// ... the counters of a call, in the order of kmx_resolve_stats ...
enum { RES_C_CANDIDATES = 0, RES_C_RESOLVED, RES_C_CROSSED, RES_C_UNSUPPORTED, RES_C_AMBIGUOUS, RES_C_N };
// ... and the input, the work arrays and the output of one call (resolve_kernels.h).  ver[u] = the copies of unitig u (1 to 4) with
// pi packed above them: bits 8 + 2 a .. 9 + 2 a hold pi(a).  sc[u] = (new unitigs, bytes, edges) in front of unitig u, the scan of
// (copies, copies x bytes, edges out of both orientations of all copies).  Every array of the caller is read and written under the
// bounds given here: U, n_ubases, n_links, seq_cap, rec_cap.
struct ResDev {
	int k;
	u64 U, n_ubases, n_links;
	const unsigned char *useq;   // [n_ubases]
	const u64 *uoffs;            // [U + 1]
	const Unitig *urec;          // [U] or null
	const u64 *loffs;            // [2 U + 1]
	const u32 *links;            // [n_links]
	const u64 *hits;             // [n_links] or null
	const u64 *through;          // [16 U]
	u64 min_reads, max_cross;
	unsigned char *bad;          // [U]: an edge at this unitig has no mirror
	u32 *ver;                    // [U]
	CtgTot *sc;                  // [U + 1]
	unsigned long long *cnt;     // [RES_C_N]
	unsigned char *rseq;         // [seq_cap]
	u64 seq_cap, rec_cap;
	u64 *roffs;                  // [rec_cap + 1]
	Unitig *rrec;                // [rec_cap] or null
	u32 *origin;                 // [rec_cap]
	ResPlace *rplace;            // [U]
	u64 *rloffs;                 // [2 rec_cap + 1]
	u32 *rlinks;                 // [n_links]
	u64 *lorigin;                // [n_links]
	u64 *rhits;                  // [n_links] or null
};
// kmx_unitig_pair_walks*: a pair's record and an entry of the pair links, the layouts of kmx_pair and kmx_pair_link (include/kmx.h;
// pair_host.h asserts them) ...
struct Pair {
	u64 walk_a, walk_b;
	u32 cls, edge, oa, xa, ob, xb;
	long long d, frag;
	u64 reserved;
};
struct PairLink {
	u32 a, b;
	u64 n_pairs, sum_dist;
	u32 min_dist, max_dist;
};
// ... the classes (KMX_PAIR_* of include/kmx.h) and the counters of a call, in the order of kmx_pair_stats behind n_pairs ...
enum { PAIR_NONE = 0, PAIR_SINGLE, PAIR_SAME, PAIR_INVERTED, PAIR_LINK, PAIR_FAR };
enum { PAIR_C_NONE = 0, PAIR_C_SINGLE, PAIR_C_SAME, PAIR_C_NEGATIVE, PAIR_C_INVERTED, PAIR_C_LINK, PAIR_C_ADJACENT, PAIR_C_FAR, PAIR_C_N };
// ... and the input, the work arrays and the output of one call (pair_kernels.h).  The work items of the fold are the n_in entries
// of the input list, then one per pair: key[i] = a << 32 | b (PAIR_NO_KEY for a pair that is no link), idx[i] = i; skey, sidx: the
// same sorted by key; sc[n_items + 1]: the key changes in front of a sorted item, sc[n_items] the merged count; mrg[n_items]: the
// merged records, their min_dist inverted so that all zero is the neutral element.  Every array of the caller is read and
// written under the bounds given here.
struct PairDev {
	const Walk *walks;           // [n_walks]
	u64 n_walks;
	const u64 *wo;               // [n_seqs + 1]
	u64 n_seqs, n_pairs;
	const u32 *steps;            // [n_steps]
	u64 n_steps;
	const u64 *loffs;            // [2 U + 1]
	const u32 *links;            // [n_links]
	u64 n_links;
	const u32 *mu;               // [U]
	u64 U;
	int k;
	u32 min_mapped, max_dist, bin_width, n_bins;
	unsigned long long *anchor;  // [n_seqs]: min(n_mapped, 2^32 - 1) << 32 | ~(index within the read), 0 for none
	unsigned long long *cnt;     // [PAIR_C_N]
	Pair *pairs;                 // [n_pairs] or null
	unsigned long long *hist;    // [n_bins] or null, added to
	unsigned long long *pair_hits;   // [n_links] or null, added to
	PairLink *plinks;            // [cap] or null: the list, in and out
	u64 cap, n_in, n_items;      // n_items = n_in + n_pairs, 0 without a list
	u64 *key, *idx, *skey, *sidx;
	u32 *dist;                   // [n_pairs]
	u64 *sc;
	PairLink *mrg;
};
// kmx_unitig_scaffold*: a scaffold, a step and a unitig's place, the layouts of kmx_scaffold, kmx_scaffold_step and
// kmx_scaffold_place (include/kmx.h; scaffold_host.h asserts them) ...
struct Scaffold {
	u64 n_bases, n_kmers, sum_count;
	u32 min_count, max_count;
	u32 first_step, n_steps;     // n_steps | SCF_CIRCULAR
	u64 n_gap_bases, min_pairs, sum_pairs;
};
struct ScfStep {
	u32 o, n_gap;
	long long est;
};
struct ScfPlace {
	u32 os, step;
	u64 off;
};
static constexpr u32 SCF_CIRCULAR = 0x80000000u;
// ... the counters of a call, the first six per entry of the list ...
enum { SCF_C_LINKS = 0, SCF_C_IGNORED, SCF_C_BELOW_MIN, SCF_C_BELOW_RATIO, SCF_C_KEPT, SCF_C_CHAIN, SCF_C_CIRCULAR, SCF_C_MULTI, SCF_C_N };
// ... and the input, the work arrays and the output of one call (scaffold_kernels.h).  The rank state is the contigs' CtgRank, its
// second rank in bytes, and the marks are their CtgTot.  Every array of the caller is read and written under the bounds given
// here: U, n_ubases, n_plinks, seq_cap.
struct ScfDev {
	int k;
	u64 U, n_ubases, n_plinks;
	const unsigned char *useq;   // [n_ubases]
	const u64 *uoffs;            // [U + 1]
	const Unitig *urec;          // [U] or null
	const PairLink *plinks;      // [n_plinks]
	u64 min_pairs;
	u32 ratio, inner, min_n, max_n;
	u64 *best;                   // [2 U]
	u32 *nk;                     // [2 U]: the kept edges out of o
	u32 *only;                   // [2 U]: the smallest entry that gives a kept edge out of o, all ones for none
	unsigned char *circ;         // [U]: the unitig lies on a cycle of chain links
	CtgTot *sc;                  // [U + 1]: the scanned marks
	u64 *ubase;                  // [U]: where the oriented string of u starts in sseq | CTG_REV
	unsigned long long *cnt;     // [SCF_C_N]
	unsigned char *sseq;         // [seq_cap] or null
	u64 seq_cap;
	u64 *soffs;                  // [U + 1]
	Scaffold *srec;              // [U]
	ScfStep *steps;              // [U]
	ScfPlace *place;             // [U]
};
// kmx_unitig_pair_paths*: the record of a list entry, the layout of kmx_pair_path (include/kmx.h; pair_path_host.h asserts it) ...
struct PairPath {
	u32 verdict, n_steps;
	u64 first_step, windows;
	u32 n_hits, n_visited;
};
// ... the verdicts (KMX_PATH_* of include/kmx.h), which are also the first seven counters of a call, in the order of
// kmx_pair_path_stats behind n_entries ...
enum { PP_IGNORED = 0, PP_BELOW_MIN, PP_NO_PATH, PP_ADJACENT, PP_PATH, PP_AMBIGUOUS, PP_COMPLEX, PP_C_ADDED, PP_C_MISSING, PP_C_N };
static constexpr u32 PP_MAX_STEPS = 16;                          // KMX_PATH_MAX_STEPS
// ... and the input, the work arrays and the output of one call (pair_path_kernels.h).  work[n_plinks * max_steps]: the steps of an
// entry's first hit; sc[n_plinks + 1]: the steps of the PATH entries in front of an entry, sc[n_plinks] their total.  Every array
// of the caller is read and written under the bounds given here: U, n_links, n_plinks, cap.
struct PathDev {
	int k;
	u64 U, n_links, n_plinks, cap;
	const u64 *uoffs;            // [U + 1]
	const u64 *loffs;            // [2 U + 1]
	const u32 *links;            // [n_links]
	const PairLink *plinks;      // [n_plinks]
	u64 min_pairs;
	u32 inner, tol, max_steps, max_visits;
	PairPath *precs;             // [n_plinks]
	u32 *psteps;                 // [cap] or null
	unsigned long long *through; // [16 U] or null, added to
	unsigned long long *path_hits;   // [n_links] or null, added to
	u32 *work;
	u64 *sc;
	unsigned long long *cnt;     // [PP_C_N]
};
// kmx_unitig_scaffold_fill*: a filled scaffold's record and a step, the layouts of kmx_scaffold_fill and kmx_fill_step
// (include/kmx.h; fill_host.h asserts them) ...
struct ScfFill {
	u64 n_bases, n_gap_bases, n_fill_bases, n_path_links, n_adjacent_links, n_n_links, n_pieces, first_piece;
};
struct FillStep {
	u32 o, kind, entry, n_pieces;
	u64 off, n_front;
};
// ... the kinds of a step (KMX_FILL_* of include/kmx.h), which are also the first four counters of a call, in the order of
// kmx_fill_stats ...
enum { FILL_HEAD = 0, FILL_N, FILL_ADJACENT, FILL_PATH, FILL_C_NO_ENTRY, FILL_C_MIRROR, FILL_C_REMOVED, FILL_C_FILLED, FILL_C_N };
// ... what the scan carries per step: the scaffolds that start, the bytes, the pieces and the piece bytes in front of it, and the
// last step in front of it that starts a scaffold ...
struct FillTot {
	u64 n, len, np, pb, first;
};
// ... and the input, the work arrays and the output of one call (fill_kernels.h).  pc_*: the n_pc pieces of the filled paths in
// scaffold order: the oriented unitig, where its bytes go in fseq, and the piece bytes in front of it (pc_pre[n_pc] their total,
// pbytes).  Every array of the caller is read and written under the bounds given here: U, n_ubases, S, n_plinks, n_psteps,
// seq_cap, piece_cap.
struct FillDev {
	int k;
	u32 kinds;
	u64 U, n_ubases, S, n_plinks, n_psteps;
	const unsigned char *useq;   // [n_ubases]
	const u64 *uoffs;            // [U + 1]
	const Scaffold *srec;        // [S]
	const ScfStep *steps;        // [U]
	const PairLink *plinks;      // [n_plinks]
	const PairPath *precs;       // [n_plinks]
	const u32 *psteps;           // [n_psteps]
	FillTot *tot, *sc;           // [U + 1] each: per step, and scanned
	u64 *ubase;                  // [U]: where the oriented string of u starts in fseq | CTG_REV | CTG_FIRST
	unsigned long long *cnt;     // [FILL_C_N]
	u32 *pc_o;                   // [n_pc]
	u64 *pc_dst;                 // [n_pc]
	u64 *pc_pre;                 // [n_pc + 1]
	u64 n_pc, pbytes;
	unsigned char *fseq;         // [seq_cap] or null
	u64 seq_cap;
	u64 *foffs;                  // [S + 1]
	ScfFill *frec;               // [S]
	FillStep *fsteps;            // [U]
	u32 *pieces;                 // [piece_cap] or null
	u64 piece_cap;
};
// kmx_unitig_pair_reduce*: the record of a list entry, the layout of kmx_pair_reduce (include/kmx.h; reduce_host.h asserts it) ...
struct PairReduce {
	u32 verdict, via, n_via, side;
	long long g, delta;
};
// ... the verdicts (KMX_REDUCE_* of include/kmx.h), which are also the first five counters of a call, in the order of
// kmx_pair_reduce_stats behind n_entries ...
enum { RED_IGNORED = 0, RED_BELOW_MIN, RED_KEPT, RED_TRANSITIVE, RED_COMPLEX, RED_C_EXAMINED, RED_C_N };
static constexpr u64 RED_NO_KEY = ~0ULL;                         // the row key of an entry that gives no rows: behind every real row
// ... and the input, the work arrays and the output of one call (reduce_kernels.h).  The table: key[2 n_plinks] = src << 32 | dst
// of the rows 2 i and 2 i + 1 of entry i (RED_NO_KEY for an entry that is not eligible), val = the row's number; skey, sval: the
// same sorted by key, stably, so rows of one key are in entry order.  flag[n_plinks]: 1 for an entry that stays; sc[n_plinks + 1]:
// its exclusive scan, sc[n_plinks] is n_out.  Every array of the caller is read and written under the bounds given
// here: U, n_ubases, n_plinks, cap.
struct RedDev {
	int k;
	u64 U, n_ubases, n_plinks, cap;
	const u64 *uoffs;            // [U + 1]
	const PairLink *plinks;      // [n_plinks]
	u64 min_pairs;
	u32 inner, tol, max_row;
	PairReduce *rrecs;           // [n_plinks]
	PairLink *lout;              // [cap] or null
	u32 *origin;                 // [cap] or null
	u64 *key, *skey;             // [2 n_plinks] each
	u32 *val, *sval;             // [2 n_plinks] each
	u32 *flag;                   // [n_plinks]
	u64 *sc;                     // [n_plinks + 1]
	unsigned long long *cnt;     // [RED_C_N]
};
// kmx_unitig_pair_lift*: the record of a list entry, the layout of kmx_pair_lift (include/kmx.h; lift_host.h asserts it) ...
struct PairLift {
	u32 cls, out, A, B;
	long long shift;
	u32 flipped, reserved;
};
// ... the classes (KMX_LIFT_* of include/kmx.h), which are also the first five counters of a call; behind them the backward SAME
// entries, the pairs of the five classes and of the backward SAME entries, and the lifted d of the forward SAME entries ...
enum { LIFT_IGNORED = 0, LIFT_SAME, LIFT_INVERTED, LIFT_LINK, LIFT_FAR, LIFT_C_SAME_BACK, LIFT_C_PAIRS /* + class */, LIFT_C_PAIRS_SAME_BACK = LIFT_C_PAIRS + 5, LIFT_C_SUM_SAME_D, LIFT_C_N };
static constexpr u64 LIFT_NO_KEY = ~0ULL;                        // the key of an entry that is no LINK: behind every real key
enum { LIFT_FOLD_WAVE = 0, LIFT_FOLD_PLAIN = 1 };
// ... and the input, the work arrays and the output of one call (lift_kernels.h).  The work item of entry i: key[i] = its canonical
// contig key A << 32 | B (LIFT_NO_KEY when it is no LINK), idx[i] = i, item[i] = (A, B, n, sum, lo, hi) after the shift; skey, sidx:
// key and idx sorted by key, stably; sc[n_plinks + 1]: the key changes in front of a sorted item, sc[n_plinks] is n_out;
// mrg[n_plinks]: the merged records, their min_dist inverted so that all zero is the neutral element.  Every array of the caller is
// read and written under the bounds given here: U, n_ubases, C, n_plinks, cap.
struct LiftDev {
	int k, fold;                 // fold: LIFT_FOLD_*
	u64 U, n_ubases, C, n_plinks, cap;
	const u64 *uoffs;            // [U + 1]
	const CtgPlace *place;       // [U]
	const Contig *crec;          // [C]
	const PairLink *plinks;      // [n_plinks]
	u32 max_dist;
	PairLift *lrec;              // [n_plinks]
	PairLink *lout;              // [cap] or null
	u64 *key, *skey;             // [n_plinks] each
	u32 *idx, *sidx;             // [n_plinks] each
	PairLink *item;              // [n_plinks]
	PairLink *mrg;               // [n_plinks]
	u64 *sc;                     // [n_plinks + 1]
	unsigned long long *cnt;     // [LIFT_C_N]
};
// rank state per oriented node: pair = pointer << 32 | rank (a head points at itself with rank 0), mn = the smallest listing
// index among the `rank` nodes from this one back (what a cycle is cut at)

enum { SLOT_UNDECIDED = 0, SLOT_FAILED = 1, SLOT_INSERTED = 2, SLOT_CONTENDED = 3 };

// Optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg).
enum { KC_CLASSIFY = 0, KC_CHECK_CLAIM, KC_VERIFY_COMMIT, KC_SLOW, KC_REORDER, KC_REST, KC_QUERY, KC_DETECT, KC_COMMIT_CHECK, KC_FILE, KC_N };   // CHECK_CLAIM = check + emit, VERIFY_COMMIT = commit
struct KernelProf {
	bool on = false;             // HIP events around every launch of a kernel class
	bool count = false;          // the fused launches also count what they examine, commit and issue (the ST_PIPE_* statistics): their
	                             // accounting variant is slower than the product's, so it is never the one that is timed
	void *events = nullptr;      // std::vector<hipEvent_t>* owned by the host side
	void *spans = nullptr;       // std::vector<int>* : class of span i uses events 2i, 2i+1
	void (*begin)(KernelProf *, int cls, hipStream_t) = nullptr;
	void (*end)(KernelProf *, hipStream_t) = nullptr;
};
#define KPROF_BEGIN(p, cls, st) do { if ((p) && (p)->on) (p)->begin((p), (cls), (st)); } while (0)
#define KPROF_END(p, st) do { if ((p) && (p)->on) (p)->end((p), (st)); } while (0)
