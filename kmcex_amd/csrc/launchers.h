// launchers.h -- every kmxk:: launcher of kernels.hip (with range_kernels.h, count_kernels.h), rest_device.hip and
// count_device.hip, declared once: the defining files include it too, so a changed return type or default argument no longer
// compiles (a changed parameter list is an unresolved symbol when libkmx.so is linked).
#pragma once
#include "kmx_types.h"

template <typename T> struct DevBuf;                               // hip_owned.h

namespace kmxk {
void histogram(const u32 *, u64, int, int, int, u64 *, u64 *, hipStream_t);
int classify_tiles(u64 n);
void classify_count(const ModelDev &, const u64 *, const u32 *, u64, u64, int *, int *, int *, u64 *, const BitScatter &, int, hipStream_t, KernelProf *);
void classify_scatter(const ModelDev &, const u64 *, const u32 *, u64, const int *, u64 *, u32 *, u64, hipStream_t);
void block_init(const BlockDev &, int, int, int, hipStream_t);
void round(const ModelDev &, const BlockDev &, int, int, int, u64 *, int, hipStream_t, KernelProf *, const KmbackJob *, const BitScatter *, const RoundProbe *probe = nullptr);
void commit_flush(const ModelDev &, const BlockDev &, int, int, hipStream_t, KernelProf *);
void rest_append(const ModelDev &, const BlockDev &, int, int, int, u64 *, int *, unsigned long long *, u64 *, int *, u64 *, hipStream_t, int istride = 1);
void kmback_emit(const ModelDev &, const BlockDev &, const u64 *, const unsigned char *, int, int, int, int, int, const BitScatter &, hipStream_t, int istride = 1);
void bs_apply(const BitScatter &, hipStream_t);
void ring_import(const ModelDev &, const BlockDev &, int, const RingLists &, u64 *, u32 *, hipStream_t);
void ring_export(const ModelDev &, const BlockDev &, int, const RingLists &, u64 *, hipStream_t);
void or_words(u32 *, const u32 *, u64, hipStream_t);
void range_emit(const ModelDev &, const BlockDev &, const RangeDev &, const RangePlan &, int, int, bool, hipStream_t);
void range_seal(const RangeDev &, const RangePlan &, hipStream_t);
void range_verdict(const ModelDev &, const BlockDev &, int *, int, const RangeIn &, unsigned char *, int, bool, hipStream_t);
void range_apply(const ModelDev &, const BlockDev &, const RangeDev &, const RangePlan &, int, int, bool, hipStream_t);
void range_resolve(const ModelDev &, const BlockDev &, const RangeDev &, const RangePlan &, int, int, bool, hipStream_t);
void range_commit_apply(const ModelDev &, const RangeIn &, int, hipStream_t);
void query(const ModelDev &, const u64 *, u64, int *, hipStream_t, KernelProf *, u64 *acct = nullptr);
void query_ascii(const ModelDev &, int, const unsigned char *, int, u64, int *, hipStream_t);
void query_seq(const ModelDev &, const SeqView &, u64 p0, u64 n_win, int *, const SeqDirty &, hipStream_t, KernelProf *);
void seq_summary_init(SeqSummary *, u64, hipStream_t, KernelProf *);
void seq_summary_finish(SeqSummary *, const u64 *, u64, u64, int, hipStream_t, KernelProf *);
void summarise_seq(const ModelDev &, const SeqView &, u64 p0, u64 n_win, const SeqSumDev &, const SeqDirty &, hipStream_t, KernelProf *);
void seq_correction_init(SeqCorrection *, const u64 *, u64, u64, int, hipStream_t, KernelProf *);
void correct_piece(const ModelDev &, const SeqView &, u64 p0, u64 n_win, u64 w0, u64 w1, u64 *bits, const CorrDev &, unsigned char *flags, const SeqDirty &, hipStream_t, KernelProf *);
void seq_edits_init(SeqEdits *, const u64 *, u64, u64, int, hipStream_t, KernelProf *);
void edit_weak_piece(const ModelDev &, const SeqView &, u64 w0, u64 n_win, int thr, u64 *bits, const SeqDirty &, hipStream_t, KernelProf *);
void edit_sites_piece(const ModelDev &, const SeqView &, u64 p0, u64 n_win, const u64 *bits, const EditDev &, unsigned char *flags, hipStream_t, KernelProf *);
void extend_walks(const ModelDev &, const SeqView &, const ExtDev &, u32 *lists, u32 *cnt, int steps, hipStream_t, KernelProf *);
void cells_from_disk(const unsigned char *, const unsigned char *, u64, cell_t *, u64, hipStream_t);
void cells_to_disk(const cell_t *, u64, u64, int, unsigned char *, hipStream_t);
void debug_hash(int, const u64 *, u64, const u32 *, int, int, u64 *, hipStream_t);
void debug_min_kmer(int, const u64 *, u64, u64 *, hipStream_t);
void debug_mod(const u64 *, u64, u64, u64 *, hipStream_t);
void micro(int, u64 *, u64, u64, u64, u64 *, hipStream_t);
// rest_device.hip: `tmp` is the scratch of both, grown (after the stream has drained) when a table asks for more
hipError_t rest_sort(const u64 *, const int *, u64, int, int, u64 *, int *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t rest_index(const u64 *, u64, int, int, int, int *, int *, u64 *, int *, DevBuf<unsigned char> &tmp, hipStream_t);
void rest_expand(const int *, const int *, const u64 *, int, int, int, int, u64 *, hipStream_t);
void rest_accel(const u64 *, u64, int, int, int, const int *, const int *, const u64 *, int, u32 *, u64 *, hipStream_t);
void rest_suffix_bytes(const u64 *, u64, int, int, unsigned char *, hipStream_t);
void count_windows(int, const unsigned char *, u64, const u64 *, u64, u64, u64, u64 *, u64 *, u64, unsigned long long *, hipStream_t);
void kmc_decode(const KmcDecode &, int, u64, u64, u64 *, u32 *, hipStream_t);
// count_device.hip: `tmp` is rocPRIM's scratch, grown (after the stream has drained) when a pass asks for more
hipError_t count_piece(int, int, u64 *, u64 *, u64, u64, u32 *, unsigned long long *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t count_merge(int, const u64 *, const u32 *, u64, const u64 *, const u32 *, u64, u64 *, u32 *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t count_reduce(int, const u64 *, const u32 *, u64, u64 *, u32 *, unsigned long long *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t count_filter(int, const u64 *, const u32 *, u64, u32, u32, u32, u64 *, u32 *, unsigned char *, unsigned long long *, DevBuf<unsigned char> &tmp, hipStream_t);
// edit_device.hip: the edit list sorted (keys -> keys, alt is room for n more), and applied to the bases it was found on
hipError_t edit_sort(u64 *keys, u64 *alt, u64 n, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t edit_apply(const unsigned char *, const u64 *, u64, u64, const u64 *, u64, u64 *, unsigned char *, u64, u64 *, unsigned long long *, DevBuf<unsigned char> &tmp, hipStream_t);
// polish_device.hip: what runs between two passes of kmx_polish_seqs (fold + scan, then place + apply), the final offsets and gather
void polish_empty(SeqPolish *, u64 *, u64, hipStream_t);
hipError_t polish_fold(const SeqEdits *, const u64 *, const u64 *, u64, u64, SeqPolish *, int, bool, PolishTri *, PolishTri *, unsigned char *, u64 *, u64 *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t polish_apply(const unsigned char *, const u64 *, const u64 *, u64, u64, const unsigned char *, const PolishTri *, const u64 *, u64, u64 *, int, const u64 *, u64 *, unsigned char *, u64, u64 *, u64 *,
                        unsigned char *, u64, u64 *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t polish_offsets(const u64 *, u64, u64 *, DevBuf<unsigned char> &tmp, hipStream_t);
void polish_gather(const PolishHomes &, const u64 *, const u64 *, u64, unsigned char *, u64, hipStream_t);
// unitig_device.hip: the phases of kmx_unitigs (index + validation, adjacency, links, a doubling round, the cut of the cycles,
// marks + scan, emit)
void unitig_index(const UniDev &, hipStream_t);
void unitig_adjacency(const UniDev &, hipStream_t);
void unitig_links(const UniDev &, u64 *, u32 *, hipStream_t);
void unitig_round(const u64 *, const u32 *, u64 *, u32 *, u64, u32 *, hipStream_t);
void unitig_cut(const UniDev &, const u64 *, const u32 *, u64 *, hipStream_t);
hipError_t unitig_mark(const UniDev &, const u64 *, UniTot *, UniTot *, DevBuf<unsigned char> &tmp, hipStream_t);
void unitig_emit(const UniDev &, const u64 *, const UniTot *, u64, unsigned char *, u64, u64 *, Unitig *, u64, hipStream_t);
// ... and of kmx_unitig_graph: the link counts at the heads + their scan, the edges between oriented unitigs
hipError_t unitig_link_mark(const UniDev &, const u64 *, const UniTot *, u64 *, u64 *, DevBuf<unsigned char> &tmp, hipStream_t);
void unitig_link_emit(const UniDev &, const u64 *, const UniTot *, const u64 *, u64, u64 *, u64, u32 *, u64, hipStream_t);
// ... and of kmx_unitig_graph_clean: a round's verdicts (one byte per unitig; the kind counters), the removal (the working counts, removed[], the k-mer counter)
void unitig_clean(const UniClean &, unsigned char *, unsigned long long *, hipStream_t);
void unitig_drop(const UniDev &, const u64 *, const UniTot *, const unsigned char *, u64, u32 *, unsigned char *, unsigned char, unsigned long long *, hipStream_t);
// unitig_device.hip, behind those: kmx_unitig_map_*: the place table of a session; per batch the records' start, one chunk of windows, the end
void map_index(const MapDev &, const unsigned char *, const u64 *, u64, hipStream_t);
void map_rec_init(SeqMap *, u64, hipStream_t);
hipError_t map_chunk(const MapDev &, const SeqView &, u64, u64, const MapChunk &, const MapOut &, unsigned long long *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t map_finish(const MapOut &, const u64 *, u64, u64, int, DevBuf<unsigned char> &tmp, hipStream_t);
// ... and kmx_unitig_walk_segs*: the walks of a batch's segments (walk_kernels.h); the totals land in D.sc[D.n_segs] and D.cnt
hipError_t walk_segs(const WalkDev &, DevBuf<unsigned char> &tmp, hipStream_t);
// ... and kmx_unitig_contigs* (contig_kernels.h): supports, verdicts and the rank state; a doubling round; the cut; marks + scan
// (the totals land in D.sc[D.U]); steps, places, records, the scan of the end counts (its total in D.clsc[2 D.U]), the contig
// graph and the bytes
void contig_links(const CtgDev &, CtgRank *, u32 *, hipStream_t);
void contig_round(const CtgRank *, const u32 *, CtgRank *, u32 *, u64, u32 *, hipStream_t);
void contig_cut(const CtgDev &, const CtgRank *, const u32 *, CtgRank *, hipStream_t);
hipError_t contig_mark(const CtgDev &, const CtgRank *, CtgTot *, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t contig_place(const CtgDev &, const CtgRank *, DevBuf<unsigned char> &tmp, hipStream_t);
void contig_bytes(const CtgDev &, hipStream_t);
// ... and kmx_unitig_walk_through* (resolve_kernels.h): the through hits of a batch's walks; the counters land in D.cnt
hipError_t walk_through(const ThroughDev &, hipStream_t);
// ... and kmx_unitig_pair_walks* (pair_kernels.h): the pairs of a batch's walks; the counters land in D.cnt, the merged count of
// the list in D.sc[D.n_items]
hipError_t pair_walks(const PairDev &, DevBuf<unsigned char> &tmp, hipStream_t);
// ... and kmx_unitig_resolve*: verdicts (the counters land in D.cnt), the scan (its totals in D.sc[D.U]), records, links, bytes
hipError_t resolve_verdicts(const ResDev &, CtgTot *, hipStream_t);
hipError_t resolve_scan(const ResDev &, const CtgTot *, DevBuf<unsigned char> &tmp, hipStream_t);
void resolve_records(const ResDev &, hipStream_t);
void resolve_links(const ResDev &, hipStream_t);
void resolve_bytes(const ResDev &, hipStream_t);
// ... and kmx_unitig_scaffold* (scaffold_kernels.h): bests, verdicts and the rank state (the rounds are contig_round's); the cut;
// marks + scan (the totals land in D.sc[D.U]); steps, places and records; the N fill and the bytes
hipError_t scaffold_links(const ScfDev &, CtgRank *, u32 *, hipStream_t);
void scaffold_cut(const ScfDev &, const CtgRank *, const u32 *, CtgRank *, hipStream_t);
hipError_t scaffold_mark(const ScfDev &, const CtgRank *, CtgTot *, DevBuf<unsigned char> &tmp, hipStream_t);
void scaffold_place(const ScfDev &, const CtgRank *, hipStream_t);
hipError_t scaffold_bytes(const ScfDev &, u64 n_sbases, hipStream_t);
// ... and kmx_unitig_pair_paths* (pair_path_kernels.h): the search per list entry, the scan of the paths' steps, the additions
hipError_t pair_path_search(const PathDev &, hipStream_t);
hipError_t pair_path_scan(const PathDev &, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t pair_path_apply(const PathDev &, hipStream_t);
// ... and kmx_unitig_scaffold_fill* (fill_kernels.h): the kinds with the counters, the scan (its totals in D.sc[D.U]), steps,
// records and pieces, the N fill and the two emits
hipError_t fill_kinds(const FillDev &, hipStream_t);
hipError_t fill_scan(const FillDev &, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t fill_place(const FillDev &, hipStream_t);
hipError_t fill_bytes(const FillDev &, u64 n_fbases, hipStream_t);
// ... and kmx_unitig_pair_reduce* (reduce_kernels.h): the rows and their sort, the verdicts with the keep flags, the scan (its
// total in D.sc[D.n_plinks]), the entries that stay
hipError_t reduce_rows(const RedDev &, hipStream_t);
hipError_t reduce_sort(const RedDev &, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t reduce_verdicts(const RedDev &, hipStream_t);
hipError_t reduce_scan(const RedDev &, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t reduce_compact(const RedDev &, hipStream_t);
// ... and kmx_unitig_pair_lift* (lift_kernels.h): the classes with the work items, their sort, the scan of the key changes (its
// total in D.sc[D.n_plinks]) with the fold, the records' run indices with the list
hipError_t lift_classify(const LiftDev &, hipStream_t);
hipError_t lift_sort(const LiftDev &, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t lift_fold(const LiftDev &, DevBuf<unsigned char> &tmp, hipStream_t);
hipError_t lift_store(const LiftDev &, hipStream_t);
}   // namespace kmxk
