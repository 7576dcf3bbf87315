// unitig_device.hip -- the launchers of unitig_kernels.h (kmx_unitigs*, kmx_count_unitigs*, kmx_*unitig_graph*, kmx_*unitig_graph_clean*).  The host side that sizes the
// buffers, waits for the round flags and the totals, and checks the capacities is unitig_host.h.  Behind them the launchers of map_kernels.h (kmx_unitig_map_*), which
// search the same listing through the same bucket index, and the launcher of walk_kernels.h (kmx_unitig_walk_segs*); their host side is map_host.h.
// Then the launchers of contig_kernels.h (kmx_unitig_contigs*); their host side is contig_host.h.  Last the launcher of
// resolve_kernels.h (kmx_unitig_walk_through*); its host side is resolve_host.h.  Behind them the launcher of pair_kernels.h
// (kmx_unitig_pair_walks*); its host side is pair_host.h.  Last the launchers of scaffold_kernels.h (kmx_unitig_scaffold*); their
// host side is scaffold_host.h.  Behind them the launchers of pair_path_kernels.h (kmx_unitig_pair_paths*); their host side is
// pair_path_host.h.  Then the launchers of fill_kernels.h (kmx_unitig_scaffold_fill*); their host side is fill_host.h.  Then the
// launchers of reduce_kernels.h (kmx_unitig_pair_reduce*); their host side is reduce_host.h.  Last the launchers of lift_kernels.h
// (kmx_unitig_pair_lift*); their host side is lift_host.h.
#include "hip_owned.h"
#include "launchers.h"
#include "unitig_kernels.h"
#include "map_kernels.h"
#include "walk_kernels.h"
#include "contig_kernels.h"
#include "resolve_kernels.h"
#include "pair_kernels.h"
#include "scaffold_kernels.h"
#include "pair_path_kernels.h"
#include "fill_kernels.h"
#include "reduce_kernels.h"
#include "lift_kernels.h"
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace {

inline unsigned nblk(u64 n) { return (unsigned)((n + 255) / 256); }

struct TotPlus {
	__host__ __device__ UniTot operator()(const UniTot &a, const UniTot &b) const { return UniTot{a.n + b.n, a.len + b.len}; }
};
struct CtgPlus {
	__host__ __device__ CtgTot operator()(const CtgTot &a, const CtgTot &b) const { return CtgTot{a.n + b.n, a.len + b.len, a.steps + b.steps}; }
};

struct FillPlus {
	__host__ __device__ FillTot operator()(const FillTot &a, const FillTot &b) const { return FillTot{a.n + b.n, a.len + b.len, a.np + b.np, a.pb + b.pb, a.first > b.first ? a.first : b.first}; }
};

}   // namespace

namespace kmxk {

// validation + the bucket index; *d.err is zero before
void unitig_index(const UniDev &d, hipStream_t st)
{
	if (d.W == 1) hipLaunchKernelGGL(k_uni_index<1>, dim3(nblk(d.n + 1)), dim3(256), 0, st, d);
	else hipLaunchKernelGGL(k_uni_index<2>, dim3(nblk(d.n + 1)), dim3(256), 0, st, d);
}

// degrees and only-neighbours of every entry
void unitig_adjacency(const UniDev &d, hipStream_t st)
{
	if (!d.n) return;
	if (d.W == 1) hipLaunchKernelGGL(k_uni_adj<1>, dim3(nblk(8 * d.n)), dim3(256), 0, st, d);
	else hipLaunchKernelGGL(k_uni_adj<2>, dim3(nblk(8 * d.n)), dim3(256), 0, st, d);
}

// links in -> the rank state of the 2 n oriented nodes
void unitig_links(const UniDev &d, u64 *pair, u32 *mn, hipStream_t st)
{
	if (d.n) hipLaunchKernelGGL(k_uni_init, dim3(nblk(2 * d.n)), dim3(256), 0, st, d, pair, mn);
}

// one round of doubling from (pin, mnin) into (pout, mnout); *moved is set when a node moved (mnin / mnout may be null)
void unitig_round(const u64 *pin, const u32 *mnin, u64 *pout, u32 *mnout, u64 n, u32 *moved, hipStream_t st)
{
	if (n) hipLaunchKernelGGL(k_uni_round, dim3(nblk(2 * n)), dim3(256), 0, st, pin, mnin, pout, mnout, 2 * n, moved);
}

void unitig_cut(const UniDev &d, const u64 *pin, const u32 *mnin, u64 *pout, hipStream_t st)
{
	if (d.n) hipLaunchKernelGGL(k_uni_cut, dim3(nblk(2 * d.n)), dim3(256), 0, st, d, pin, mnin, pout);
}

// marks, then their exclusive scan: sc[i] = (unitigs, bytes) in front of entry i, sc[n] the totals
hipError_t unitig_mark(const UniDev &d, const u64 *pair, UniTot *tot, UniTot *sc, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	hipLaunchKernelGGL(k_uni_mark, dim3(nblk(d.n + 1)), dim3(256), 0, st, d, pair, tot);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const UniTot *)tot, sc, UniTot{0, 0}, (size_t)(d.n + 1), TotPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const UniTot *)tot, sc, UniTot{0, 0}, (size_t)(d.n + 1), TotPlus(), st));
	return hipGetLastError();
}

// strings, offsets and records of n_uni unitigs; nothing is written at or behind seq[seq_cap], offs[rec_cap + 1], rec[rec_cap]
void unitig_emit(const UniDev &d, const u64 *pair, const UniTot *sc, u64 n_uni, unsigned char *seq, u64 seq_cap, u64 *offs, Unitig *rec, u64 rec_cap, hipStream_t st)
{
	const u64 nr = n_uni < rec_cap ? n_uni : rec_cap;
	if (rec && nr) hipLaunchKernelGGL(k_uni_rec_init, dim3(nblk(nr)), dim3(256), 0, st, rec, nr);
	if (d.W == 1) hipLaunchKernelGGL(k_uni_emit<1>, dim3(nblk(d.n + 1)), dim3(256), 0, st, d, pair, sc, seq, seq_cap, offs, rec, rec_cap);
	else hipLaunchKernelGGL(k_uni_emit<2>, dim3(nblk(d.n + 1)), dim3(256), 0, st, d, pair, sc, seq, seq_cap, offs, rec, rec_cap);
}

// per-head link counts into lc, then their exclusive scan: lsc[i] = the edges of the unitigs in front of entry i, lsc[n] the
// total; the head and tail entry of every unitig into d.succ1 and d.pred1 (sc: the scanned marks)
hipError_t unitig_link_mark(const UniDev &d, const u64 *pair, const UniTot *sc, u64 *lc, u64 *lsc, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	hipLaunchKernelGGL(k_uni_lmark, dim3(nblk(d.n + 1)), dim3(256), 0, st, d, pair, sc, lc);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const u64 *)lc, lsc, (u64)0, (size_t)(d.n + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const u64 *)lc, lsc, (u64)0, (size_t)(d.n + 1), rocprim::plus<u64>(), st));
	return hipGetLastError();
}

// the CSR of the edges between the 2 n_uni oriented unitigs, 8 lanes per unitig; nothing is written at or behind loffs[2 rec_cap + 1], links[link_cap]
void unitig_link_emit(const UniDev &d, const u64 *pair, const UniTot *sc, const u64 *lsc, u64 n_uni, u64 *loffs, u64 rec_cap, u32 *links, u64 link_cap, hipStream_t st)
{
	if (d.W == 1) hipLaunchKernelGGL(k_uni_links<1>, dim3(nblk(8 * (n_uni + 1))), dim3(256), 0, st, d, pair, sc, lsc, n_uni, loffs, rec_cap, links, link_cap);
	else hipLaunchKernelGGL(k_uni_links<2>, dim3(nblk(8 * (n_uni + 1))), dim3(256), 0, st, d, pair, sc, lsc, n_uni, loffs, rec_cap, links, link_cap);
}

// one verdict byte per unitig of the graph the two emits wrote (c), the three kind counters into cnt[0..2]
void unitig_clean(const UniClean &c, unsigned char *verdict, unsigned long long *cnt, hipStream_t st)
{
	if (c.n_uni) hipLaunchKernelGGL(k_uni_clean, dim3(nblk(8 * c.n_uni)), dim3(256), 0, st, c, verdict, cnt);
}

// the working counts of the unitigs with a verdict to 0, their entries' round into removed (may be null), their number into cnt[3]
void unitig_drop(const UniDev &d, const u64 *pair, const UniTot *sc, const unsigned char *verdict, u64 n_uni, u32 *wcnt, unsigned char *removed, unsigned char round, unsigned long long *cnt, hipStream_t st)
{
	if (d.n) hipLaunchKernelGGL(k_uni_drop, dim3(nblk(d.n)), dim3(256), 0, st, d, pair, sc, verdict, n_uni, wcnt, removed, round, cnt);
}

// ---- kmx_unitig_map_* (map_kernels.h)

// m_u and the place of every window of the unitig set; M.place is all ones and *M.d.err zero before
void map_index(const MapDev &M, const unsigned char *useq, const u64 *uoffs, u64 n_ubases, hipStream_t st)
{
	if (!M.U || !n_ubases) return;
	hipLaunchKernelGGL(k_map_mu, dim3(nblk(M.U)), dim3(256), 0, st, M, uoffs, n_ubases);
	if (M.d.W == 1) hipLaunchKernelGGL(k_map_index<1>, dim3(nblk(n_ubases)), dim3(256), 0, st, M, useq, uoffs, n_ubases);
	else hipLaunchKernelGGL(k_map_index<2>, dim3(nblk(n_ubases)), dim3(256), 0, st, M, useq, uoffs, n_ubases);
}

void map_rec_init(SeqMap *rec, u64 n_seqs, hipStream_t st)
{
	if (rec && n_seqs) hipLaunchKernelGGL(k_map_rec_init, dim3(nblk(n_seqs)), dim3(256), 0, st, rec, n_seqs);
}

// the windows [p0, p0 + n_win) of the reads: codes, the scan of the start flags, starts, ends, and the state for the next chunk
hipError_t map_chunk(const MapDev &M, const SeqView &v, u64 p0, u64 n_win, const MapChunk &C, const MapOut &O, unsigned long long *hits, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	if (!n_win) return hipSuccess;
	const unsigned grid = (unsigned)((n_win + MAP_WIN - 1) / MAP_WIN);
	if (M.d.W == 1) hipLaunchKernelGGL(k_map_windows<1>, dim3(grid), dim3(MAP_BT), 0, st, M, v, p0, n_win, C.code, hits);
	else hipLaunchKernelGGL(k_map_windows<2>, dim3(grid), dim3(MAP_BT), 0, st, M, v, p0, n_win, C.code, hits);
	auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), MapStartFlag{C.code, n_win});
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, flags, C.ex, 0u, (size_t)(n_win + 1), rocprim::plus<u32>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, flags, C.ex, 0u, (size_t)(n_win + 1), rocprim::plus<u32>(), st));
	hipLaunchKernelGGL(k_map_starts, dim3(nblk(n_win)), dim3(256), 0, st, C, O, v.offs, v.n_seqs, v.n_total, p0, n_win);
	hipLaunchKernelGGL(k_map_ends, dim3(nblk(n_win)), dim3(256), 0, st, C, O, v.offs, v.n_seqs, v.n_total, p0, n_win);
	hipLaunchKernelGGL(k_map_advance, dim3(1), dim3(1), 0, st, C, n_win);
	return hipGetLastError();
}

// behind the last chunk: the records are completed, the segments per read become the CSR (O.so[n_seqs] is 0 before)
hipError_t map_finish(const MapOut &O, const u64 *offs, u64 n_seqs, u64 n_total, int k, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	if (O.rec && n_seqs) hipLaunchKernelGGL(k_map_rec_finish, dim3(nblk(n_seqs)), dim3(256), 0, st, O.rec, O.so, offs, n_seqs, n_total, k);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const u64 *)O.so, O.so, (u64)0, (size_t)(n_seqs + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const u64 *)O.so, O.so, (u64)0, (size_t)(n_seqs + 1), rocprim::plus<u64>(), st));
	return hipGetLastError();
}

// ---- kmx_unitig_walk_segs* (walk_kernels.h): flags, the scan of (walk starts, step starts), heads, sums.  D.sc[D.n_segs] holds
// the two totals and D.cnt the five counters behind it; D.n_segs > 0
hipError_t walk_segs(const WalkDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.flag, 0, D.n_segs, st));
	RCHK(hipMemsetAsync(D.cnt, 0, WALK_C_N * sizeof(unsigned long long), st));
	if (D.n_seqs) hipLaunchKernelGGL(k_walk_first, dim3(nblk(D.n_seqs)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_walk_join, dim3(nblk(D.n_segs)), dim3(256), 0, st, D);
	auto tots = rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), WalkFlagTot{D.flag, D.n_segs});
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, tots, D.sc, WalkTot{0, 0}, (size_t)(D.n_segs + 1), WalkPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, tots, D.sc, WalkTot{0, 0}, (size_t)(D.n_segs + 1), WalkPlus(), st));
	const u64 n = D.n_segs > D.n_seqs + 1 ? D.n_segs : D.n_seqs + 1;
	hipLaunchKernelGGL(k_walk_heads, dim3(nblk(n)), dim3(256), 0, st, D);
	if (D.walks && D.walk_cap) hipLaunchKernelGGL(k_walk_sums, dim3(nblk(D.n_segs)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_contigs* (contig_kernels.h); D.U > 0.  D.cnt is zero before contig_links, D.circ before contig_cut.

// supports, verdicts with the four edge counters, the chain link in of every oriented unitig -> the rank state
void contig_links(const CtgDev &D, CtgRank *rank, u32 *mn, hipStream_t st)
{
	hipLaunchKernelGGL(k_ctg_sup, dim3(nblk(2 * D.U)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_ctg_keep, dim3(nblk(2 * D.U)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_ctg_init, dim3(nblk(2 * D.U)), dim3(256), 0, st, D, rank, mn);
}

void contig_round(const CtgRank *pin, const u32 *mnin, CtgRank *pout, u32 *mnout, u64 U, u32 *moved, hipStream_t st)
{
	hipLaunchKernelGGL(k_ctg_round, dim3(nblk(2 * U)), dim3(256), 0, st, pin, mnin, pout, mnout, 2 * U, moved);
}

void contig_cut(const CtgDev &D, const CtgRank *pin, const u32 *mnin, CtgRank *pout, hipStream_t st)
{
	hipLaunchKernelGGL(k_ctg_cut, dim3(nblk(2 * D.U)), dim3(256), 0, st, D, pin, mnin, pout);
}

// marks into tot[U + 1], then their exclusive scan into D.sc: D.sc[u] = (contigs, bytes, steps) in front of unitig u
hipError_t contig_mark(const CtgDev &D, const CtgRank *rank, CtgTot *tot, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	hipLaunchKernelGGL(k_ctg_mark, dim3(nblk(D.U + 1)), dim3(256), 0, st, D, rank, tot);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const CtgTot *)tot, D.sc, CtgTot{0, 0, 0}, (size_t)(D.U + 1), CtgPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const CtgTot *)tot, D.sc, CtgTot{0, 0, 0}, (size_t)(D.U + 1), CtgPlus(), st));
	return hipGetLastError();
}

// behind the marks: records, steps, places and coffsets, then the end counts, their scan and the contig graph
hipError_t contig_place(const CtgDev &D, const CtgRank *rank, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.clc, 0, (2 * D.U + 1) * 8, st));
	hipLaunchKernelGGL(k_ctg_rec_init, dim3(nblk(D.U)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_ctg_place, dim3(nblk(D.U + 1)), dim3(256), 0, st, D, rank);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const u64 *)D.clc, D.clsc, (u64)0, (size_t)(2 * D.U + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const u64 *)D.clc, D.clsc, (u64)0, (size_t)(2 * D.U + 1), rocprim::plus<u64>(), st));
	hipLaunchKernelGGL(k_ctg_clinks, dim3(nblk(2 * D.U + 1)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the bytes: one block per tile of the flat input (D.ubase as contig_place left it)
void contig_bytes(const CtgDev &D, hipStream_t st)
{
	if (D.n_ubases) hipLaunchKernelGGL(k_ctg_emit, dim3((unsigned)((D.n_ubases + CTG_TILE - 1) / CTG_TILE)), dim3(256), 0, st, D);
}

// ---- kmx_unitig_walk_through* (resolve_kernels.h): marks, then one lane per step.  D.cnt holds the three counters behind it;
// D.n_steps > 0 and D.U > 0
hipError_t walk_through(const ThroughDev &D, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.mark, 0, D.n_steps + 1, st));
	RCHK(hipMemsetAsync(D.cnt, 0, THR_C_N * sizeof(unsigned long long), st));
	if (D.n_walks) hipLaunchKernelGGL(k_thr_mark, dim3(nblk(D.n_walks)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_thr_count, dim3(nblk(D.n_steps)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_resolve* (resolve_kernels.h); D.U > 0

// the edges without a mirror, then the verdict of every unitig and what the scan adds up (tot[U + 1])
hipError_t resolve_verdicts(const ResDev &D, CtgTot *tot, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.bad, 0, D.U, st));
	RCHK(hipMemsetAsync(D.cnt, 0, RES_C_N * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_res_bad, dim3(nblk(2 * D.U)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_res_verdict, dim3(nblk(D.U + 1)), dim3(256), 0, st, D, tot);
	return hipGetLastError();
}

// the exclusive scan of the triples into D.sc: D.sc[u] = (new unitigs, bytes, edges) in front of unitig u, D.sc[U] the totals
hipError_t resolve_scan(const ResDev &D, const CtgTot *tot, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, tot, D.sc, CtgTot{0, 0, 0}, (size_t)(D.U + 1), CtgPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, tot, D.sc, CtgTot{0, 0, 0}, (size_t)(D.U + 1), CtgPlus(), st));
	return hipGetLastError();
}

// rplace, origin, roffsets, records and row starts; the totals fit the capacities (the host has checked)
void resolve_records(const ResDev &D, hipStream_t st)
{
	hipLaunchKernelGGL(k_res_place, dim3(nblk(D.U + 1)), dim3(256), 0, st, D);
}

void resolve_links(const ResDev &D, hipStream_t st)
{
	hipLaunchKernelGGL(k_res_rows, dim3(nblk(2 * D.U)), dim3(256), 0, st, D);
}

// the bytes: one block per tile of the flat input
void resolve_bytes(const ResDev &D, hipStream_t st)
{
	if (D.n_ubases) hipLaunchKernelGGL(k_res_emit, dim3((unsigned)((D.n_ubases + RES_TILE - 1) / RES_TILE)), dim3(256), 0, st, D);
}

// ---- kmx_unitig_pair_walks* (pair_kernels.h): anchors, classes, then the fold of the work items into the list: sort by key,
// scan of the key changes, fold, store.  D.cnt holds the eight counters behind it and, with a list, D.sc[D.n_items] the merged
// count; D.n_pairs > 0
hipError_t pair_walks(const PairDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.anchor, 0, D.n_seqs * 8, st));
	RCHK(hipMemsetAsync(D.cnt, 0, PAIR_C_N * sizeof(unsigned long long), st));
	if (D.n_walks) hipLaunchKernelGGL(k_pair_anchor, dim3(nblk(D.n_walks)), dim3(256), 0, st, D);
	if (D.n_items && D.n_in) hipLaunchKernelGGL(k_pair_items, dim3(nblk(D.n_in)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_pair_classify, dim3(nblk(D.n_pairs)), dim3(256), 0, st, D);
	if (!D.n_items) return hipGetLastError();
	size_t b1 = 0, b2 = 0;
	auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), PairKeyFlag{D.skey, D.n_items});
	RCHK(rocprim::radix_sort_pairs(nullptr, b1, D.key, D.skey, D.idx, D.sidx, (size_t)D.n_items, 0, 64, st));
	RCHK(rocprim::exclusive_scan(nullptr, b2, flags, D.sc, (u64)0, (size_t)(D.n_items + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(b1 > b2 ? b1 : b2, st));
	RCHK(rocprim::radix_sort_pairs(tmp.get(), b1, D.key, D.skey, D.idx, D.sidx, (size_t)D.n_items, 0, 64, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), b2, flags, D.sc, (u64)0, (size_t)(D.n_items + 1), rocprim::plus<u64>(), st));
	RCHK(hipMemsetAsync(D.mrg, 0, D.n_items * sizeof(PairLink), st));
	hipLaunchKernelGGL(k_pair_fold, dim3(nblk(D.n_items)), dim3(256), 0, st, D);
	const u64 n_store = D.n_items < D.cap ? D.n_items : D.cap;
	if (n_store) hipLaunchKernelGGL(k_pair_store, dim3(nblk(n_store)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_scaffold* (scaffold_kernels.h); D.U > 0.  D.cnt and D.circ are zero before scaffold_links.

// bests, verdicts with the five entry counters, the chain link in of every oriented unitig -> the rank state.  The rounds are
// contig_round's.
hipError_t scaffold_links(const ScfDev &D, CtgRank *rank, u32 *mn, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.best, 0, 2 * D.U * 8, st));
	RCHK(hipMemsetAsync(D.nk, 0, 2 * D.U * 4, st));
	RCHK(hipMemsetAsync(D.only, 0xFF, 2 * D.U * 4, st));
	if (D.n_plinks) {
		hipLaunchKernelGGL(k_scf_best, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
		hipLaunchKernelGGL(k_scf_keep, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	}
	hipLaunchKernelGGL(k_scf_init, dim3(nblk(2 * D.U)), dim3(256), 0, st, D, rank, mn);
	return hipGetLastError();
}

void scaffold_cut(const ScfDev &D, const CtgRank *pin, const u32 *mnin, CtgRank *pout, hipStream_t st)
{
	hipLaunchKernelGGL(k_scf_cut, dim3(nblk(2 * D.U)), dim3(256), 0, st, D, pin, mnin, pout);
}

// marks into tot[U + 1], then their exclusive scan into D.sc: D.sc[u] = (scaffolds, bytes, steps) in front of unitig u
hipError_t scaffold_mark(const ScfDev &D, const CtgRank *rank, CtgTot *tot, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	hipLaunchKernelGGL(k_scf_mark, dim3(nblk(D.U + 1)), dim3(256), 0, st, D, rank, tot);
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const CtgTot *)tot, D.sc, CtgTot{0, 0, 0}, (size_t)(D.U + 1), CtgPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const CtgTot *)tot, D.sc, CtgTot{0, 0, 0}, (size_t)(D.U + 1), CtgPlus(), st));
	return hipGetLastError();
}

// behind the marks: records, steps, places and soffsets
void scaffold_place(const ScfDev &D, const CtgRank *rank, hipStream_t st)
{
	hipLaunchKernelGGL(k_scf_rec_init, dim3(nblk(D.U)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_scf_place, dim3(nblk(D.U + 1)), dim3(256), 0, st, D, rank);
}

// the bytes, n_sbases <= D.seq_cap of them: 'N' everywhere, then one block per tile of the flat input (D.ubase as scaffold_place
// left it)
hipError_t scaffold_bytes(const ScfDev &D, u64 n_sbases, hipStream_t st)
{
	if (n_sbases) RCHK(hipMemsetAsync(D.sseq, 'N', n_sbases, st));
	if (D.n_ubases) hipLaunchKernelGGL(k_scf_emit, dim3((unsigned)((D.n_ubases + CTG_TILE - 1) / CTG_TILE)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_pair_paths* (pair_path_kernels.h); D.U > 0 and D.n_plinks > 0

// the verdict of every entry with its seven counters; the first hit's steps into D.work
hipError_t pair_path_search(const PathDev &D, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.cnt, 0, PP_C_N * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_pp_search, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the exclusive scan of the PATH entries' steps into D.sc[n_plinks + 1]: D.sc[n_plinks] is what psteps has to hold
hipError_t pair_path_scan(const PathDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	auto t = rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), PairPathSteps{D.precs, D.n_plinks});
	RCHK(rocprim::exclusive_scan(nullptr, bytes, t, D.sc, (u64)0, (size_t)(D.n_plinks + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, t, D.sc, (u64)0, (size_t)(D.n_plinks + 1), rocprim::plus<u64>(), st));
	return hipGetLastError();
}

// first_step, the steps where they fit, the additions to through and path_hits, n_added and n_missing
hipError_t pair_path_apply(const PathDev &D, hipStream_t st)
{
	hipLaunchKernelGGL(k_pp_apply, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_scaffold_fill* (fill_kernels.h); D.U > 0

// the kind of every step with the call's counters, and what it writes: D.tot[U + 1]
hipError_t fill_kinds(const FillDev &D, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.tot, 0, (D.U + 1) * sizeof(FillTot), st));
	RCHK(hipMemsetAsync(D.cnt, 0, FILL_C_N * sizeof(unsigned long long), st));
	if (D.S) hipLaunchKernelGGL(k_fill_heads, dim3(nblk(D.S)), dim3(256), 0, st, D);
	hipLaunchKernelGGL(k_fill_kind, dim3(nblk(D.U)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the exclusive scan of D.tot into D.sc[U + 1]: D.sc[U] holds the scaffolds, the bytes, the pieces and the piece bytes of the call
hipError_t fill_scan(const FillDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::exclusive_scan(nullptr, bytes, (const FillTot *)D.tot, D.sc, FillTot{0, 0, 0, 0, 0}, (size_t)(D.U + 1), FillPlus(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, (const FillTot *)D.tot, D.sc, FillTot{0, 0, 0, 0, 0}, (size_t)(D.U + 1), FillPlus(), st));
	return hipGetLastError();
}

// behind the scan and the host's wait for its totals (D.n_pc, D.pbytes and the piece arrays are set): steps, records, foffsets,
// the words of the step emit and the pieces
hipError_t fill_place(const FillDev &D, hipStream_t st)
{
	if (D.S) RCHK(hipMemsetAsync(D.frec, 0, D.S * sizeof(ScfFill), st));
	RCHK(hipMemsetAsync(D.ubase, 0xFF, D.U * 8, st));
	hipLaunchKernelGGL(k_fill_place, dim3(nblk(D.U + 1)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the bytes, n_fbases <= D.seq_cap of them: 'N' everywhere, the steps' own bytes by the tile emit over the flat input, the path
// pieces by the gather emit over the piece bytes
hipError_t fill_bytes(const FillDev &D, u64 n_fbases, hipStream_t st)
{
	if (n_fbases) RCHK(hipMemsetAsync(D.fseq, 'N', n_fbases, st));
	if (D.n_ubases) hipLaunchKernelGGL(k_fill_step_emit, dim3((unsigned)((D.n_ubases + CTG_TILE - 1) / CTG_TILE)), dim3(256), 0, st, D);
	if (D.pbytes && D.n_pc) hipLaunchKernelGGL(k_fill_emit, dim3((unsigned)((D.pbytes + FILL_TILE - 1) / FILL_TILE)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_pair_reduce* (reduce_kernels.h); D.n_plinks > 0

// eligibility and g of every entry with the two counters, and its two rows
hipError_t reduce_rows(const RedDev &D, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.cnt, 0, RED_C_N * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_red_rows, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the table sorted by src << 32 | dst: the sort is stable, so rows of one key stay in entry order
hipError_t reduce_sort(const RedDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::radix_sort_pairs(nullptr, bytes, D.key, D.skey, D.val, D.sval, (size_t)(2 * D.n_plinks), 0, 64, st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::radix_sort_pairs(tmp.get(), bytes, D.key, D.skey, D.val, D.sval, (size_t)(2 * D.n_plinks), 0, 64, st));
	return hipGetLastError();
}

// the verdict of every entry with its counters and its keep flag, 8 lanes per entry
hipError_t reduce_verdicts(const RedDev &D, hipStream_t st)
{
	hipLaunchKernelGGL(k_red_verdict, dim3(nblk(8 * D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the exclusive scan of the keep flags into D.sc[n_plinks + 1]: D.sc[n_plinks] is what lout has to hold
hipError_t reduce_scan(const RedDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	auto t = rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), RedFlag{D.flag, D.n_plinks});
	RCHK(rocprim::exclusive_scan(nullptr, bytes, t, D.sc, (u64)0, (size_t)(D.n_plinks + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, t, D.sc, (u64)0, (size_t)(D.n_plinks + 1), rocprim::plus<u64>(), st));
	return hipGetLastError();
}

// behind the host's wait for D.sc[n_plinks] <= D.cap: the entries that stay, in input order, and where they came from
hipError_t reduce_compact(const RedDev &D, hipStream_t st)
{
	hipLaunchKernelGGL(k_red_compact, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// ---- kmx_unitig_pair_lift* (lift_kernels.h); D.n_plinks > 0

// the class and the record of every entry with the call's counters, and its work item
hipError_t lift_classify(const LiftDev &D, hipStream_t st)
{
	RCHK(hipMemsetAsync(D.cnt, 0, LIFT_C_N * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(k_lift_classify, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// the work items sorted by their contig key: the sort is stable, and the entries that are no LINK come last
hipError_t lift_sort(const LiftDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	RCHK(rocprim::radix_sort_pairs(nullptr, bytes, D.key, D.skey, D.idx, D.sidx, (size_t)D.n_plinks, 0, 64, st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::radix_sort_pairs(tmp.get(), bytes, D.key, D.skey, D.idx, D.sidx, (size_t)D.n_plinks, 0, 64, st));
	return hipGetLastError();
}

// the exclusive scan of the key changes into D.sc[n_plinks + 1] (D.sc[n_plinks] is what lout has to hold), then the fold of
// every run into D.mrg: whole wavefronts, since every lane takes part in the shuffles of the wave fold
hipError_t lift_fold(const LiftDev &D, DevBuf<unsigned char> &tmp, hipStream_t st)
{
	size_t bytes = 0;
	auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), LiftKeyFlag{D.skey, D.n_plinks});
	RCHK(rocprim::exclusive_scan(nullptr, bytes, flags, D.sc, (u64)0, (size_t)(D.n_plinks + 1), rocprim::plus<u64>(), st));
	RCHK(tmp.ensure(bytes, st));
	RCHK(rocprim::exclusive_scan(tmp.get(), bytes, flags, D.sc, (u64)0, (size_t)(D.n_plinks + 1), rocprim::plus<u64>(), st));
	RCHK(hipMemsetAsync(D.mrg, 0, D.n_plinks * sizeof(PairLink), st));
	if (D.fold == LIFT_FOLD_PLAIN) hipLaunchKernelGGL(k_lift_fold<LIFT_FOLD_PLAIN>, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	else hipLaunchKernelGGL(k_lift_fold<LIFT_FOLD_WAVE>, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

// lrec[].out of every LINK entry, and the merged records into lout where their count fits D.cap
hipError_t lift_store(const LiftDev &D, hipStream_t st)
{
	hipLaunchKernelGGL(k_lift_store, dim3(nblk(D.n_plinks)), dim3(256), 0, st, D);
	return hipGetLastError();
}

}   // namespace kmxk
