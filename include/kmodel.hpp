// include/kmodel.hpp -- drop-in C++ facade with the reference's own names over the C ABI (include/kmx.h).
//
// A program written against lzhLab/kmcEx's kmodel.hpp (README.md:64-93, main.cpp:143-149) compiles against
// this header and links libkmx.so instead of pulling in the header-only CPU implementation (tests/facade_query.cpp is
// written the way those snippets are: unqualified std names, Tools::get_file_name, KModel() + load(dir)):
//
//     KModel* km = get_model(ci, cs, n_hash, n_bit);      // kmodel.hpp:674
//     km->init(kmc_database);                              // kmodel.hpp:57   (README: init_KModel)
//     km->save(dir);                                       // kmodel.hpp:173  (README: save_model)
//     KModel* km2 = get_model(dir);                        // kmodel.hpp:680
//     std::vector<int> occ = km2->kmer_to_occ(kmers, 4);   // kmodel.hpp:90
//
// Error behaviour follows the reference: a message on stdout and exit(1) (kmodel.hpp:394-397, :682-685).
// Unlike the reference the object has a destructor, so the device memory can be released.
#pragma once
#ifndef KMODEL_H
#define KMODEL_H

// Everything the reference header makes visible to its includers (kmodel.hpp:6-21): main.cpp uses ifstream, strncmp,
// sprintf and system without including their headers itself.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "kmx.h"

// kmc_api/kmer_defs.h:27-28 (pulled in through kmc_api/kmc_file.h, kmodel.hpp:14): main.cpp's entry point is `_tmain`
#ifndef _WIN32
#ifndef _tmain
#define _TCHAR char
#define _tmain main
#endif
#endif

// The reference header leaks `using namespace std;` and its README snippets and main.cpp rely on it (unqualified string,
// vector<string>, cout); a drop-in has to leak it too.
using namespace std;

const string BASE_CHAR = "ACGT";          // kmodel.hpp:23-24 (visible to includers of the reference header)
const int BLOACK_SIZE = 1 << 19;

// the one helper of tools.hpp that main.cpp uses outside the class (tools.hpp:102-105)
class Tools {
public:
	static string get_file_name(string path)
	{
		const size_t pos = path.find_last_of('/');
		return pos == string::npos ? path : path.substr(pos + 1);
	}
};

class KModel {
public:
	KModel() : h_(nullptr) { abi(); }                                  // kmodel.hpp:43; fill it with load(dir)
	explicit KModel(kmx_model *h) : h_(h) { abi(); }
	~KModel() { kmx_destroy(h_); }
	// a binary built against an older kmx.h must not hand its structs to a newer libkmx.so
	static void abi()
	{
		if (kmx_abi_version() != KMX_ABI_VERSION) {
			std::cout << "libkmx.so has ABI version " << kmx_abi_version() << ", this program was built for " << KMX_ABI_VERSION << "; rebuild it" << std::endl;
			exit(1);
		}
	}
	KModel(const KModel &) = delete;
	KModel &operator=(const KModel &) = delete;

	// kmodel.hpp:57 -- two passes over the KMC listing, rest-table build
	// kmodel.hpp:57-86.  KMX_DEVICES=0,1,2,... (HIP device numbers, repeats allowed): the model is built by those GPUs
	// together, one host thread per device inside libkmx.so, and this object keeps the replica of the first one.
	// KMX_PARTITION=range: every coupled array cut by position range over the devices, the words of a round written
	// straight into the owners' memory through peer mappings (kmx_build_from_kmc_multi_ex, KMX_PARTITION_RANGE);
	// KMX_PARTITION=ring (the default): arrays owned whole, lists travel with peer copies.  Unset: the current device alone.
	// A value that does not parse is an error, like a bad argument of the reference's own command line.
	void init(std::string db_file)
	{
		std::vector<int> devs;
		if (const char *e = std::getenv("KMX_DEVICES")) {
			for (const char *p = e; *p;) {
				char *end = nullptr;
				const long v = std::strtol(p, &end, 10);
				if (end == p || v < 0 || (*end != ',' && *end != 0) || (*end == ',' && end[1] == 0)) {
					std::cout << "KMX_DEVICES=" << e << ": a comma-separated list of HIP device numbers is expected" << std::endl;
					exit(1);
				}
				devs.push_back((int)v);
				p = *end == ',' ? end + 1 : end;
			}
		}
		int partition = KMX_PARTITION_RING;
		if (const char *e = std::getenv("KMX_PARTITION")) {
			const std::string v(e);
			if (v == "range") partition = KMX_PARTITION_RANGE;
			else if (v == "range-rccl") partition = KMX_PARTITION_RANGE_RCCL;     // the same partition, the words as fixed-size RCCL messages (one device per entry of KMX_DEVICES)
			else if (v != "ring" && !v.empty()) { std::cout << "KMX_PARTITION=" << v << ": ring, range or range-rccl" << std::endl; exit(1); }
		}
		if (devs.empty()) { check(kmx_build_from_kmc(h_, db_file.c_str())); return; }
		kmx_stats st;
		check(kmx_get_stats(h_, &st));
		std::vector<kmx_model *> hs(devs.size(), nullptr);
		for (size_t d = 0; d < devs.size(); d++) {
			const int rc = kmx_create_on(devs[d], st.ci, st.cs, st.nh, st.nb, &hs[d]);
			if (rc) { for (size_t e2 = 0; e2 < d; e2++) kmx_destroy(hs[e2]); check(rc); }
		}
		const int rc = kmx_build_from_kmc_multi_ex(hs.data(), (int)hs.size(), db_file.c_str(), partition);
		if (rc) { for (kmx_model *h : hs) kmx_destroy(h); check(rc); }
		kmx_destroy(h_);
		h_ = hs[0];
		for (size_t d = 1; d < hs.size(); d++) kmx_destroy(hs[d]);
	}
	void init_KModel(std::string db_file) { init(db_file); }                 // README.md:76
	// KMC's counting step and init together (main.cpp:137-146): the k-mers of a FASTQ / FASTA file (plain or gzip) or "@list"
	// counted on the GPU, the model built from their listing (kmx_build_from_reads), k in [4, 64] like every model here (the
	// reference's rest table is undefined at k = 3).  Errors as init: a message, then exit(1).
	void init_reads(const std::string &input, int k) { check(kmx_build_from_reads(h_, k, input.c_str())); }

	// kmodel.hpp:90 -- t_num is accepted for source compatibility; the batch runs on the GPU
	// Safe to call from several threads on one object at once: the library serialises queries per handle.
	std::vector<int> kmer_to_occ(std::vector<std::string> kmer_v, int t_num = 4)
	{
		(void)t_num;
		const size_t n = kmer_v.size();
		std::vector<int> occ_v(n);
		if (!n) return occ_v;
		static_assert(sizeof(int) == sizeof(int32_t), "int is 32 bits on every supported target");
		// the reference answers every string on its own, whatever its length.  One length (the usual batch): the strings
		// go to the library as they lie, and it cuts them into chunks that worker threads pack while the GPU answers the
		// chunk before (kmx_query_strings).  Mixed lengths: one such call per length.
		const size_t len0 = kmer_v[0].size();
		bool uniform = true;
		for (size_t i = 1; i < n && uniform; i++) uniform = kmer_v[i].size() == len0;
		std::vector<const char *> ptrs;
		if (uniform) {
			ptrs.resize(n);
			for (size_t i = 0; i < n; i++) ptrs[i] = kmer_v[i].data();
			check(kmx_query_strings(h_, ptrs.data(), (int)len0, n, (int32_t *)occ_v.data()));
			return occ_v;
		}
		std::vector<size_t> order(n);
		for (size_t i = 0; i < n; i++) order[i] = i;
		std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return kmer_v[a].size() < kmer_v[b].size(); });
		for (size_t lo = 0; lo < n;) {
			const size_t len = kmer_v[order[lo]].size();
			size_t hi = lo;
			ptrs.clear();
			while (hi < n && kmer_v[order[hi]].size() == len) ptrs.push_back(kmer_v[order[hi++]].data());
			std::vector<int32_t> part(hi - lo);
			check(kmx_query_strings(h_, ptrs.data(), (int)len, hi - lo, part.data()));
			for (size_t j = lo; j < hi; j++) occ_v[order[j]] = part[j - lo];
			lo = hi;
		}
		return occ_v;
	}

	// kmodel.hpp:100 -- safe from several threads at once (an OpenMP loop over it, like the reference's): serialised per handle
	int kmer_to_occ(std::string kmer, uint32_t r_occ = 0)
	{
		(void)r_occ;
		int32_t occ = 0;
		check(kmx_query_ascii(h_, kmer.data(), (int)kmer.size(), (int)kmer.size(), 1, &occ));
		return occ;
	}

	// Every overlapping k-mer of a read or contig at once (what error correction, repeat detection and assembly ask for):
	// answer p = kmer_to_occ(seq.substr(p, k)), p = 0 .. len - k; none for a sequence shorter than k.  The bases go to the
	// device as they are and the windows are cut there (kmx_query_seqs), instead of len - k + 1 strings built here.
	std::vector<int> seq_to_occ(const std::string &seq)
	{
		const uint64_t off[2] = {0, (uint64_t)seq.size()};
		std::vector<int> occ(seq.size());
		if (!seq.empty()) check(kmx_query_seqs(h_, seq.data(), off, 1, (int32_t *)occ.data()));
		occ.resize(windows(seq.size(), model_k()));
		return occ;
	}
	std::vector<std::vector<int> > seq_to_occ(const std::vector<std::string> &seqs)
	{
		const Flat f(seqs);
		std::vector<int32_t> occ(f.bases.size());
		if (!occ.empty()) check(kmx_query_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), occ.data()));
		std::vector<std::vector<int> > out(seqs.size());
		const size_t k = model_k();
		for (size_t i = 0; i < seqs.size(); i++) out[i].assign(occ.begin() + (size_t)f.off[i], occ.begin() + (size_t)f.off[i] + windows(seqs[i].size(), k));
		return out;
	}
	// seq_to_occ's vector reduced per sequence on the device (kmx_summarise_seqs): n_windows, sum, min, max, the windows at or
	// above each of up to KMX_SEQ_THRESHOLDS thresholds, and the first / last window below thr[0]
	kmx_seq_summary seq_summary(const std::string &seq, const std::vector<int> &thr = std::vector<int>())
	{
		const uint64_t off[2] = {0, (uint64_t)seq.size()};
		kmx_seq_summary out;
		check(kmx_summarise_seqs(h_, seq.data(), off, 1, (const int32_t *)thr.data(), (int)thr.size(), &out));
		return out;
	}
	std::vector<kmx_seq_summary> seq_summary(const std::vector<std::string> &seqs, const std::vector<int> &thr = std::vector<int>())
	{
		const Flat f(seqs);
		std::vector<kmx_seq_summary> out(seqs.size());
		check(kmx_summarise_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), (const int32_t *)thr.data(), (int)thr.size(), out.data()));
		return out;
	}

	// Substitution errors corrected from the k-mer spectrum (kmx_correct_seqs; the rule is in kmx.h): a window is weak when its
	// answer is below thr, a site is tried when at least min_support windows verify it.  Returns the corrected read(s); rec, if
	// given, receives one record per read.
	std::string seq_correct(const std::string &seq, int thr, int min_support = 1, kmx_seq_correction *rec = 0)
	{
		const uint64_t off[2] = {0, (uint64_t)seq.size()};
		std::string out(seq.size(), '\0');
		check(kmx_correct_seqs(h_, seq.data(), off, 1, thr, min_support, &out[0], rec));
		return out;
	}
	std::vector<std::string> seq_correct(const std::vector<std::string> &seqs, int thr, int min_support = 1, std::vector<kmx_seq_correction> *rec = 0)
	{
		Flat f(seqs);
		if (rec) rec->assign(seqs.size(), kmx_seq_correction());
		if (!seqs.empty()) check(kmx_correct_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), thr, min_support, &f.bases[0], rec ? &(*rec)[0] : 0));
		return split(f.bases, f.off);
	}

	// Substitutions and single-base insertions / deletions found from the k-mer spectrum and applied (kmx_edit_seqs and
	// kmx_apply_edits; the rule is in kmx.h): returns the edited reads, whose lengths may differ from the input's.  ops is a
	// subset of KMX_EDIT_OPS_SUB | KMX_EDIT_OPS_DEL | KMX_EDIT_OPS_INS; rec, if given, receives one record per read.
	std::string seq_edit(const std::string &seq, int thr, int min_support = 1, int ops = 7, kmx_seq_edits *rec = 0)
	{
		std::vector<kmx_seq_edits> r;
		const std::string out = seq_edit(std::vector<std::string>(1, seq), thr, min_support, ops, &r)[0];
		if (rec) *rec = r[0];
		return out;
	}
	std::vector<std::string> seq_edit(const std::vector<std::string> &seqs, int thr, int min_support = 1, int ops = 7, std::vector<kmx_seq_edits> *rec = 0)
	{
		const Flat f(seqs);
		std::vector<uint64_t> off_out(seqs.size() + 1, 0);
		if (rec) rec->assign(seqs.size(), kmx_seq_edits());
		std::vector<kmx_edit> edits(f.bases.size() / 3 + 1);
		uint64_t n_edits = 0;
		if (!seqs.empty()) check(kmx_edit_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), thr, min_support, ops, &edits[0], edits.size(), &n_edits, rec ? &(*rec)[0] : 0));
		std::string fixed(f.bases.size() + (size_t)n_edits, '\0');
		check(kmx_apply_edits(f.bases.data(), f.off.data(), seqs.size(), &edits[0], n_edits, &fixed[0], fixed.size(), &off_out[0]));
		return split(fixed, off_out);
	}

	// Reads polished to a fixed point (kmx_polish_seqs; the rule is in kmx.h): seq_edit's rule iterated per read on the device
	// until a pass finds nothing in it, or max_passes passes ran.  Returns the polished reads; rec, if given, receives one
	// record per read (passes, whether it converged, the edits of every kind, the last pass's counters).
	std::string seq_polish(const std::string &seq, int thr, int min_support = 1, int ops = 7, int max_passes = 8, kmx_seq_polish *rec = 0)
	{
		std::vector<kmx_seq_polish> r;
		const std::string out = seq_polish(std::vector<std::string>(1, seq), thr, min_support, ops, max_passes, &r)[0];
		if (rec) *rec = r[0];
		return out;
	}
	std::vector<std::string> seq_polish(const std::vector<std::string> &seqs, int thr, int min_support = 1, int ops = 7, int max_passes = 8, std::vector<kmx_seq_polish> *rec = 0)
	{
		const Flat f(seqs);
		std::vector<uint64_t> off_out(seqs.size() + 1, 0);
		if (rec) rec->assign(seqs.size(), kmx_seq_polish());
		std::string fixed(f.bases.size() + f.bases.size() / 16 + 64, '\0');
		if (!seqs.empty()) {
			int rc = kmx_polish_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), thr, min_support, ops, max_passes, &fixed[0], fixed.size(), &off_out[0], rec ? &(*rec)[0] : 0, 0);
			if (rc == KMX_E_RANGE && off_out.back() > fixed.size()) {   // offsets_out is complete: once more with the room it asks for
				fixed.assign((size_t)off_out.back(), '\0');
				rc = kmx_polish_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), thr, min_support, ops, max_passes, &fixed[0], fixed.size(), &off_out[0], rec ? &(*rec)[0] : 0, 0);
			}
			check(rc);
		}
		return split(fixed, off_out);
	}

	// Seeds extended to the right along the unique path of k-mers answered >= thr (kmx_extend_seqs; the rule is in kmx.h):
	// at most max_ext bases each, ties broken by a lookahead of `depth` (0 ... 3).  Returns the appended bases; rec, if given,
	// receives one record per seed (why the walk stopped, the counts along it).
	std::string seq_extend(const std::string &seed, int thr, int max_ext, int depth = 2, kmx_seq_extension *rec = 0)
	{
		const uint64_t off[2] = {0, (uint64_t)seed.size()};
		std::string ext(max_ext > 0 ? (size_t)max_ext : 1, '\0');
		kmx_seq_extension r;
		check(kmx_extend_seqs(h_, seed.data(), off, 1, thr, max_ext, depth, &ext[0], &r));
		if (rec) *rec = r;
		ext.resize(r.n_ext);
		return ext;
	}
	std::vector<std::string> seq_extend(const std::vector<std::string> &seeds, int thr, int max_ext, int depth = 2, std::vector<kmx_seq_extension> *rec = 0)
	{
		const Flat f(seeds);
		const size_t row = max_ext > 0 ? (size_t)max_ext : 1;
		std::vector<char> ext(seeds.size() * row + 1);
		std::vector<kmx_seq_extension> r(seeds.size());
		if (!seeds.empty()) check(kmx_extend_seqs(h_, f.bases.data(), f.off.data(), seeds.size(), thr, max_ext, depth, &ext[0], &r[0]));
		std::vector<std::string> out(seeds.size());
		for (size_t i = 0; i < seeds.size(); i++) out[i].assign(&ext[i * row], r[i].n_ext);
		if (rec) rec->swap(r);
		return out;
	}

	// The unitigs of a counted listing (the rule: kmx.h): the maximal non-branching paths of the de Bruijn graph whose nodes are
	// the listed k-mers with count >= thr, one string each, in the rule's order; rec (optional) receives one kmx_unitig per
	// string.  count_unitigs reads the listing init_reads / the last kmx_count_finish kept on the device; unitigs takes a
	// listing of packed canonical k-mers (W = ceil(k/32) words each, strictly ascending) and needs no built model.  k is odd.
	// Each call is two C calls, the sizing call and the call with exact room, and both rank the whole graph: twice the
	// construction.  A caller who can bound the output calls kmx_count_unitigs / kmx_unitigs once.
	std::vector<std::string> count_unitigs(uint32_t thr = 1, std::vector<kmx_unitig> *rec = 0)
	{
		return unitig_call(UnitigAsk{"count_unitigs", 0, 0, 0, 0, thr, 0}, rec, 0, 0, 0, 0);
	}
	std::vector<std::string> unitigs(const std::vector<uint64_t> &kmers, const std::vector<uint32_t> &counts, int k, uint32_t thr = 1, std::vector<kmx_unitig> *rec = 0)
	{
		return unitig_call(UnitigAsk{"unitigs", 0, &kmers, &counts, k, thr, 0}, rec, 0, 0, 0, 0);
	}
	// the unitigs as FASTA: one record per unitig, its header ">u<index> n_kmers=<m> mean_count=<sum / m, two decimals> circular=<0|1>"
	static void write_unitigs_fasta(std::ostream &out, const std::vector<std::string> &strs, const std::vector<kmx_unitig> &rec)
	{
		char mean[32];
		for (size_t u = 0; u < strs.size(); u++) {
			std::snprintf(mean, sizeof mean, "%.2f", rec[u].n_kmers ? (double)rec[u].sum_count / (double)rec[u].n_kmers : 0.0);
			out << ">u" << u << " n_kmers=" << rec[u].n_kmers << " mean_count=" << mean << " circular=" << (int)rec[u].circular << "\n" << strs[u] << "\n";
		}
	}

	// The unitig graph (the rule: kmx.h): the unitigs as above and the edges between the oriented unitigs o = 2 u + d (d = 1: the
	// reverse complement) as CSR: the edges of o are links[link_offsets[o] .. link_offsets[o + 1]), each the target o'.  The
	// twins of count_unitigs and unitigs: a sizing call plus one call.
	std::vector<std::string> count_unitig_graph(uint32_t thr, std::vector<kmx_unitig> *rec, std::vector<uint64_t> *link_offsets, std::vector<uint32_t> *links)
	{
		return unitig_call(UnitigAsk{"count_unitig_graph", 1, 0, 0, 0, thr, 0}, rec, link_offsets, links, 0, 0);
	}
	std::vector<std::string> unitig_graph(const std::vector<uint64_t> &kmers, const std::vector<uint32_t> &counts, int k, uint32_t thr, std::vector<kmx_unitig> *rec,
	                                      std::vector<uint64_t> *link_offsets, std::vector<uint32_t> *links)
	{
		return unitig_call(UnitigAsk{"unitig_graph", 1, &kmers, &counts, k, thr, 0}, rec, link_offsets, links, 0, 0);
	}
	// The cleaned unitig graph (the rule: kmx.h): count_unitig_graph / unitig_graph after tips, islands and bubbles have been
	// removed round by round under params; stats (optional) receives what was removed, removed (optional) the round per listing
	// entry.  write_unitigs_fasta and write_unitigs_gfa take the result as they take the twins'.
	std::vector<std::string> count_unitig_graph_clean(uint32_t thr, const kmx_clean_params &params, std::vector<kmx_unitig> *rec, std::vector<uint64_t> *link_offsets,
	                                                  std::vector<uint32_t> *links, kmx_clean_stats *stats = 0)
	{
		return unitig_call(UnitigAsk{"count_unitig_graph_clean", 2, 0, 0, 0, thr, &params}, rec, link_offsets, links, stats, 0);
	}
	std::vector<std::string> unitig_graph_clean(const std::vector<uint64_t> &kmers, const std::vector<uint32_t> &counts, int k, uint32_t thr, const kmx_clean_params &params,
	                                            std::vector<kmx_unitig> *rec, std::vector<uint64_t> *link_offsets, std::vector<uint32_t> *links, kmx_clean_stats *stats = 0,
	                                            std::vector<uint8_t> *removed = 0)
	{
		return unitig_call(UnitigAsk{"unitig_graph_clean", 2, &kmers, &counts, k, thr, &params}, rec, link_offsets, links, stats, removed);
	}
	// the unitig graph as GFA 1: "H\tVN:Z:1.0", one "S\tu<index>\t<string>\tLN:i:<len>\tKC:i:<sum_count>" per unitig, and one
	// "L\tu<a>\t<+|->\tu<b>\t<+|->\t<k-1>M" per mirror pair of edges: a -> b is written iff (a, b) <= (b ^ 1, a ^ 1) as pairs, so
	// a self-mirror edge (a hairpin) once.  Rows follow the order of a, then the CSR order.
	static void write_unitigs_gfa(std::ostream &out, const std::vector<std::string> &strs, const std::vector<kmx_unitig> &rec, const std::vector<uint64_t> &link_offsets,
	                              const std::vector<uint32_t> &links, int k)
	{
		out << "H\tVN:Z:1.0\n";
		for (size_t u = 0; u < strs.size(); u++) out << "S\tu" << u << "\t" << strs[u] << "\tLN:i:" << strs[u].size() << "\tKC:i:" << rec[u].sum_count << "\n";
		for (uint64_t a = 0; a + 1 < link_offsets.size(); a++)
			for (uint64_t e = link_offsets[a]; e < link_offsets[a + 1] && e < links.size(); e++) {
				const uint64_t b = links[(size_t)e], mb = b ^ 1, ma = a ^ 1;
				if (a < mb || (a == mb && b <= ma))
					out << "L\tu" << (a >> 1) << "\t" << ((a & 1) ? '-' : '+') << "\tu" << (b >> 1) << "\t" << ((b & 1) ? '-' : '+') << "\t" << (k - 1) << "M\n";
			}
	}

	// Reads mapped onto the unitigs (the rule: kmx.h): a session on the object.  unitig_map_begin takes a listing (packed canonical
	// k-mers, strictly ascending, odd k) and a unitig set as any of the calls above returns it; count_unitig_map_begin works on the
	// listing init_reads / the last kmx_count_finish kept.  seq_to_unitigs maps a batch of reads: the segments in ascending
	// position, seg_offsets [n + 1] their CSR by read, rec one kmx_seq_map per read, and hits, which it ADDS the mapped windows
	// per unitig to (the caller sizes it to the unitig set and zeroes it).  It gives room for every window, so it never comes back
	// short; a caller who can bound the segments calls kmx_unitig_map_seqs itself.
	void unitig_map_begin(const std::vector<uint64_t> &kmers, int k, const std::vector<std::string> &unitigs)
	{
		const Flat f(unitigs);
		const uint64_t W = (uint64_t)((k + 31) / 32);
		if (kmers.size() % W) { std::cout << "unitig_map_begin: " << kmers.size() << " words are no whole k-mers" << std::endl; exit(1); }
		check(kmx_unitig_map_begin(h_, k, kmers.data(), kmers.size() / W, f.bases.data(), f.off.data(), unitigs.size()));
	}
	void count_unitig_map_begin(const std::vector<std::string> &unitigs)
	{
		const Flat f(unitigs);
		check(kmx_count_unitig_map_begin(h_, f.bases.data(), f.off.data(), unitigs.size()));
	}
	std::vector<kmx_map_segment> seq_to_unitigs(const std::vector<std::string> &seqs, std::vector<uint64_t> *seg_offsets = 0, std::vector<kmx_seq_map> *rec = 0, std::vector<uint64_t> *hits = 0)
	{
		const Flat f(seqs);
		std::vector<kmx_map_segment> segs((size_t)f.off.back() + 1);
		std::vector<uint64_t> so(seqs.size() + 1, 0);
		std::vector<kmx_seq_map> r(seqs.size() + 1);
		uint64_t n = 0;
		check(kmx_unitig_map_seqs(h_, f.bases.data(), f.off.data(), seqs.size(), &segs[0], f.off.back(), &n, &so[0], &r[0], hits && !hits->empty() ? &(*hits)[0] : 0));
		segs.resize((size_t)n);
		r.resize(seqs.size());
		if (seg_offsets) seg_offsets->swap(so);
		if (rec) rec->swap(r);
		return segs;
	}
	void unitig_map_end() { check(kmx_unitig_map_end(h_)); }
	// the segments as a table, one "<read>\t<start in read>\t<windows>\tu<unitig>\t<+|->\t<offset>" per segment; first_read is the
	// index of the batch's first read and offsets [n + 1] the batch's own (a segment's pos is flat inside its batch) ...
	static void write_paths_tsv(std::ostream &out, const std::vector<kmx_map_segment> &segs, const std::vector<uint64_t> &seg_offsets, const std::vector<uint64_t> &offsets, uint64_t first_read = 0)
	{
		for (size_t i = 0; i + 1 < seg_offsets.size() && i + 1 < offsets.size(); i++)
			for (uint64_t e = seg_offsets[i]; e < seg_offsets[i + 1] && e < segs.size(); e++) {
				const kmx_map_segment &s = segs[(size_t)e];
				out << first_read + i << "\t" << s.pos - offsets[i] << "\t" << s.n_windows << "\tu" << (s.o >> 1) << "\t" << ((s.o & 1) ? '-' : '+') << "\t" << s.off << "\n";
			}
	}
	// ... and the hits, one "u<unitig>\t<hits>" per unitig
	static void write_hits_tsv(std::ostream &out, const std::vector<uint64_t> &hits)
	{
		for (size_t u = 0; u < hits.size(); u++) out << "u" << u << "\t" << hits[u] << "\n";
	}

	// The walks of mapped reads (the rule: kmx.h), inside the map session: seq_walks takes the vectors seq_to_unitigs returned and
	// the CSR of the graph the session's unitigs came from, and returns one kmx_walk per walk in ascending position; walk_offsets
	// [n + 1] is their CSR by read, steps the oriented unitigs of every walk back to back, and link_hits, which it ADDS the reads
	// per traversed link to (the caller sizes it to links and zeroes it).  It gives room for every segment, so it never comes back
	// short.
	std::vector<kmx_walk> seq_walks(const std::vector<kmx_map_segment> &segs, const std::vector<uint64_t> &seg_offsets, const std::vector<uint64_t> &link_offsets,
	                                const std::vector<uint32_t> &links, const kmx_walk_params &params, std::vector<uint64_t> *walk_offsets = 0, std::vector<uint32_t> *steps = 0,
	                                std::vector<uint64_t> *link_hits = 0, kmx_walk_stats *stats = 0)
	{
		std::vector<kmx_walk> walks(segs.size() + 1);
		std::vector<uint32_t> st(segs.size() + 1);
		std::vector<uint64_t> wo(seg_offsets.empty() ? 1 : seg_offsets.size(), 0);
		kmx_walk_stats ws = kmx_walk_stats();
		if (seg_offsets.size() > 1)
			check(kmx_unitig_walk_segs(h_, segs.empty() ? 0 : &segs[0], segs.size(), &seg_offsets[0], seg_offsets.size() - 1, link_offsets.empty() ? 0 : &link_offsets[0],
			                           links.empty() ? 0 : &links[0], links.size(), &params, &walks[0], segs.size(), &wo[0], &st[0], segs.size(),
			                           link_hits && !link_hits->empty() ? &(*link_hits)[0] : 0, &ws));
		walks.resize((size_t)ws.n_walks);
		st.resize((size_t)ws.n_steps);
		if (walk_offsets) walk_offsets->swap(wo);
		if (steps) steps->swap(st);
		if (stats) *stats = ws;
		return walks;
	}
	// the walks as GAF, one line per walk: the read (first_read + its index in the batch, as write_paths_tsv names it), its length,
	// query start and end, '+', the path (">u<N>" / "<u<N>" per step, the names of write_unitigs_gfa), the path's length (the m of
	// its steps + k - 1), start (off_first) and end (the m of all steps but the last + off_last + k), matches (n_covered: a lower
	// bound), block length (the larger of the two spans), MAPQ 255, id:i:<indel> and bg:i:<bridges>.  offsets [n + 1] are the
	// batch's own, strs the unitigs of the session.
	static void write_walks_gaf(std::ostream &out, const std::vector<kmx_walk> &walks, const std::vector<uint64_t> &walk_offsets, const std::vector<uint32_t> &steps,
	                            const std::vector<uint64_t> &offsets, const std::vector<std::string> &strs, int k, uint64_t first_read = 0)
	{
		for (size_t i = 0; i + 1 < walk_offsets.size() && i + 1 < offsets.size(); i++)
			for (uint64_t e = walk_offsets[i]; e < walk_offsets[i + 1] && e < walks.size(); e++) {
				const kmx_walk &w = walks[(size_t)e];
				const uint64_t q0 = w.pos - offsets[i], q1 = q0 + w.n_span + (uint64_t)k - 1;
				uint64_t sum_m = 0, m_last = 0;
				out << first_read + i << "\t" << offsets[i + 1] - offsets[i] << "\t" << q0 << "\t" << q1 << "\t+\t";
				for (uint64_t s = w.first_step; s < w.first_step + w.n_steps && s < steps.size(); s++) {
					const uint32_t o = steps[(size_t)s];
					m_last = (o >> 1) < strs.size() ? (uint64_t)strs[o >> 1].size() - (uint64_t)k + 1 : 0;
					sum_m += m_last;
					out << ((o & 1) ? '<' : '>') << "u" << (o >> 1);
				}
				const uint64_t p0 = w.off_first, p1 = sum_m - m_last + w.off_last + (uint64_t)k;
				out << "\t" << sum_m + (uint64_t)k - 1 << "\t" << p0 << "\t" << p1 << "\t" << w.n_covered << "\t" << (q1 - q0 > p1 - p0 ? q1 - q0 : p1 - p0) << "\t255\tid:i:" << w.indel
				    << "\tbg:i:" << w.n_inside + w.n_across << "\n";
			}
	}
	// ... and the reads per link, one "<link index>\tu<source><+|->\tu<target><+|->\t<reads>" per link of the CSR
	static void write_link_hits_tsv(std::ostream &out, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links, const std::vector<uint64_t> &link_hits)
	{
		for (uint64_t a = 0; a + 1 < link_offsets.size(); a++)
			for (uint64_t e = link_offsets[a]; e < link_offsets[a + 1] && e < links.size() && e < link_hits.size(); e++) {
				const uint32_t b = links[(size_t)e];
				out << e << "\tu" << (a >> 1) << ((a & 1) ? '-' : '+') << "\tu" << (b >> 1) << ((b & 1) ? '-' : '+') << "\t" << link_hits[(size_t)e] << "\n";
			}
	}

	// Contigs (the rule: kmx.h): the unitigs merged along the edges the reads support.  unitig_contigs takes the vectors a graph call
	// returned (rec may be null: the contigs' counts are then 0) and the link_hits seq_walks accumulated; it needs no session.  The
	// result holds the contigs, one kmx_contig each, steps (the oriented unitigs of every contig back to back), place (one per
	// unitig: its contig, strand and k-mer offset there) and the contig graph as CSR with the reads behind every edge.
	struct Contigs {
		std::vector<std::string> strs;
		std::vector<kmx_contig> rec;
		std::vector<uint32_t> steps;
		std::vector<kmx_contig_place> place;
		std::vector<uint64_t> link_offsets;
		std::vector<uint32_t> links;
		std::vector<uint64_t> support;
		kmx_contig_stats stats;
	};
	Contigs unitig_contigs(const std::vector<std::string> &unitigs, const std::vector<kmx_unitig> *rec, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links,
	                       const std::vector<uint64_t> &link_hits, int k, const kmx_contig_params &params)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), nl = links.size();
		if (link_offsets.size() != 2 * U + 1 || link_hits.size() != nl || (rec && rec->size() != U)) { std::cout << "unitig_contigs: the vectors are not those of one graph" << std::endl; exit(1); }
		Contigs c;
		std::string cseq(f.bases.size() + 1, '\0');
		std::vector<uint64_t> coff(U + 1, 0);
		c.rec.resize(U + 1); c.steps.resize(U + 1); c.place.resize(U + 1); c.link_offsets.resize(2 * U + 1); c.links.resize(nl + 1); c.support.resize(nl + 1);
		uint64_t nc = 0, nb = 0, ncl = 0;
		check(kmx_unitig_contigs(h_, k, f.bases.data(), f.off.data(), U, rec && U ? &(*rec)[0] : 0, &link_offsets[0], nl ? &links[0] : 0, nl, nl ? &link_hits[0] : 0, &params, &cseq[0], &coff[0],
		                         &c.rec[0], &c.steps[0], &c.place[0], &c.link_offsets[0], &c.links[0], &c.support[0], &nc, &nb, &ncl, &c.stats));
		coff.resize((size_t)nc + 1);
		c.strs = split(cseq, coff);
		c.rec.resize((size_t)nc); c.steps.resize(U); c.place.resize(U); c.link_offsets.resize(2 * (size_t)nc + 1); c.links.resize((size_t)ncl); c.support.resize((size_t)ncl);
		return c;
	}
	// the contigs as FASTA, header ">c<index> n_kmers=<m> n_steps=<s> circular=<0|1>"
	static void write_contigs_fasta(std::ostream &out, const Contigs &c)
	{
		for (size_t i = 0; i < c.strs.size(); i++)
			out << ">c" << i << " n_kmers=" << c.rec[i].n_kmers << " n_steps=" << c.rec[i].n_steps << " circular=" << (int)c.rec[i].circular << "\n" << c.strs[i] << "\n";
	}
	// the contig graph as GFA 1: "S\tc<index>\t<string>\tLN:i:<len>\tKC:i:<sum_count>" per contig and, per mirror pair of edges (the
	// choice of write_unitigs_gfa), "L\tc<a>\t<+|->\tc<b>\t<+|->\t<k-1>M\tRC:i:<support>".  With the unitigs (and their records, for
	// KC) it first writes their segments as write_unitigs_gfa names them and, behind the links, one "P\tc<index>\t<u<N>+|-, ...>\t
	// <k-1>M, ..." per contig ("*" for a single step): a path line must name segments of the same file.
	static void write_contigs_gfa(std::ostream &out, const Contigs &c, int k, const std::vector<std::string> *unitigs = 0, const std::vector<kmx_unitig> *urec = 0)
	{
		out << "H\tVN:Z:1.0\n";
		if (unitigs)
			for (size_t u = 0; u < unitigs->size(); u++)
				out << "S\tu" << u << "\t" << (*unitigs)[u] << "\tLN:i:" << (*unitigs)[u].size() << "\tKC:i:" << (urec && u < urec->size() ? (*urec)[u].sum_count : 0) << "\n";
		for (size_t i = 0; i < c.strs.size(); i++) out << "S\tc" << i << "\t" << c.strs[i] << "\tLN:i:" << c.strs[i].size() << "\tKC:i:" << c.rec[i].sum_count << "\n";
		for (uint64_t a = 0; a + 1 < c.link_offsets.size(); a++)
			for (uint64_t e = c.link_offsets[a]; e < c.link_offsets[a + 1] && e < c.links.size(); e++) {
				const uint64_t b = c.links[(size_t)e], mb = b ^ 1, ma = a ^ 1;
				if (a < mb || (a == mb && b <= ma))
					out << "L\tc" << (a >> 1) << "\t" << ((a & 1) ? '-' : '+') << "\tc" << (b >> 1) << "\t" << ((b & 1) ? '-' : '+') << "\t" << (k - 1) << "M\tRC:i:" << c.support[(size_t)e] << "\n";
			}
		if (!unitigs) return;
		for (size_t i = 0; i < c.rec.size(); i++) {
			out << "P\tc" << i << "\t";
			for (uint64_t s = c.rec[i].first_step; s < c.rec[i].first_step + c.rec[i].n_steps && s < c.steps.size(); s++)
				out << (s > c.rec[i].first_step ? "," : "") << "u" << (c.steps[(size_t)s] >> 1) << ((c.steps[(size_t)s] & 1) ? '-' : '+');
			out << "\t";
			if (c.rec[i].n_steps < 2) out << "*";
			for (uint32_t s = 1; s < c.rec[i].n_steps; s++) out << (s > 1 ? "," : "") << (k - 1) << "M";
			out << "\n";
		}
	}
	// ... and every step as a table, one "c<contig>\t<step>\tu<unitig>\t<+|->\t<k-mer offset in the contig>" per step
	static void write_contig_paths_tsv(std::ostream &out, const Contigs &c)
	{
		for (size_t i = 0; i < c.rec.size(); i++)
			for (uint64_t s = 0; s < c.rec[i].n_steps && c.rec[i].first_step + s < c.steps.size(); s++) {
				const uint32_t o = c.steps[(size_t)(c.rec[i].first_step + s)];
				out << "c" << i << "\t" << s << "\tu" << (o >> 1) << "\t" << ((o & 1) ? '-' : '+') << "\t" << ((o >> 1) < c.place.size() ? c.place[o >> 1].off : 0) << "\n";
			}
	}

	// Through hits and resolution (the rule: kmx.h).  unitig_through takes the walks and steps seq_walks returned and the CSR they
	// were made with, and ADDS the reads per (way in, way out) of every unitig to through (16 per unitig; an empty vector is sized
	// and zeroed).  unitig_resolve splits every unitig whose through hits pair its ways in with its ways out one to one; the result
	// is an ordinary unitig graph (strings, records when rec is given, CSR, link_hits when given) that unitig_contigs takes as it
	// is, with origin (the input unitig of every new one), place (per input unitig: its first copy and their number) and
	// link_origin (the input edge of every new one).  Neither needs a session.
	kmx_through_stats unitig_through(const std::vector<kmx_walk> &walks, const std::vector<uint32_t> &steps, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links,
	                                 std::vector<uint64_t> &through)
	{
		const size_t U = link_offsets.empty() ? 0 : (link_offsets.size() - 1) / 2;
		if (through.empty()) through.assign(16 * U, 0);
		if (through.size() != 16 * U || link_offsets.empty()) { std::cout << "unitig_through: the vectors are not those of one graph" << std::endl; exit(1); }
		kmx_through_stats st = kmx_through_stats();
		check(kmx_unitig_walk_through(h_, walks.empty() ? 0 : &walks[0], walks.size(), steps.empty() ? 0 : &steps[0], steps.size(), &link_offsets[0], links.empty() ? 0 : &links[0], links.size(), U,
		                              U ? &through[0] : 0, &st));
		return st;
	}
	struct Resolved {
		std::vector<std::string> strs;
		std::vector<kmx_unitig> rec;                 // empty when no records were given
		std::vector<uint32_t> origin;
		std::vector<kmx_resolve_place> place;
		std::vector<uint64_t> link_offsets;
		std::vector<uint32_t> links;
		std::vector<uint64_t> link_origin;
		std::vector<uint64_t> link_hits;             // empty when no link hits were given
		kmx_resolve_stats stats;
	};
	Resolved unitig_resolve(const std::vector<std::string> &unitigs, const std::vector<kmx_unitig> *rec, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links,
	                        const std::vector<uint64_t> *link_hits, const std::vector<uint64_t> &through, int k, const kmx_resolve_params &params)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), nl = links.size();
		if (link_offsets.size() != 2 * U + 1 || through.size() != 16 * U || (link_hits && link_hits->size() != nl) || (rec && rec->size() != U)) {
			std::cout << "unitig_resolve: the vectors are not those of one graph" << std::endl;
			exit(1);
		}
		const bool with_rec = rec && U, with_hits = link_hits && nl;
		Resolved r;
		uint64_t n = 0, nb = 0;
		check(kmx_unitig_resolve(h_, k, f.bases.data(), f.off.data(), U, with_rec ? &(*rec)[0] : 0, &link_offsets[0], nl ? &links[0] : 0, nl, with_hits ? &(*link_hits)[0] : 0, U ? &through[0] : 0, &params,
		                         0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &n, &nb, &r.stats));                                     // the sizing call
		std::string rseq((size_t)nb + 1, '\0');
		std::vector<uint64_t> roff((size_t)n + 1, 0);
		r.rec.resize(with_rec ? (size_t)n : 0); r.origin.resize((size_t)n + 1); r.place.resize(U + 1); r.link_offsets.resize(2 * (size_t)n + 1); r.links.resize(nl + 1); r.link_origin.resize(nl + 1);
		r.link_hits.resize(with_hits ? nl : 0);
		check(kmx_unitig_resolve(h_, k, f.bases.data(), f.off.data(), U, with_rec ? &(*rec)[0] : 0, &link_offsets[0], nl ? &links[0] : 0, nl, with_hits ? &(*link_hits)[0] : 0, U ? &through[0] : 0, &params,
		                         &rseq[0], nb, &roff[0], n, with_rec ? &r.rec[0] : 0, &r.origin[0], &r.place[0], &r.link_offsets[0], &r.links[0], &r.link_origin[0], with_hits ? &r.link_hits[0] : 0, &n, &nb,
		                         &r.stats));
		r.strs = split(rseq, roff);
		r.origin.resize((size_t)n); r.place.resize(U); r.links.resize(nl); r.link_origin.resize(nl);
		return r;
	}
	// the resolved set as a table, one "u<new unitig>\tu<origin>\t<copy>" per new unitig
	static void write_resolved_tsv(std::ostream &out, const Resolved &r)
	{
		for (size_t i = 0; i < r.origin.size(); i++) {
			const uint32_t u = r.origin[i];
			out << "u" << i << "\tu" << u << "\t" << (u < r.place.size() ? i - r.place[u].first : 0) << "\n";
		}
	}

	// Read pairs (the rule: kmx.h), inside the map session: seq_pairs takes the walks, walk_offsets and steps seq_walks returned for
	// a batch of interleaved mates (reads 2 p and 2 p + 1 are pair p) and the CSR of the session's graph, and returns one kmx_pair
	// per pair.  plinks is the list of pair links earlier batches left (empty at first) and becomes the merge with this batch;
	// hist (params.n_bins entries) and pair_hits (one per link) are ADDED to; a shorter vector is grown with zeros first.  It gives
	// the list room for every entry, so it never comes back short.
	std::vector<kmx_pair> seq_pairs(const std::vector<kmx_walk> &walks, const std::vector<uint64_t> &walk_offsets, const std::vector<uint32_t> &steps, const std::vector<uint64_t> &link_offsets,
	                                const std::vector<uint32_t> &links, const kmx_pair_params &params, std::vector<kmx_pair_link> *plinks = 0, std::vector<uint64_t> *hist = 0,
	                                std::vector<uint64_t> *pair_hits = 0, kmx_pair_stats *stats = 0)
	{
		const size_t n_seqs = walk_offsets.empty() ? 0 : walk_offsets.size() - 1, np = n_seqs / 2;
		std::vector<kmx_pair> pairs(np + 1);
		kmx_pair_stats ps = kmx_pair_stats();
		uint64_t n = plinks ? plinks->size() : 0;
		if (plinks) plinks->resize((size_t)n + np + 1);
		if (hist && hist->size() < params.n_bins) hist->resize(params.n_bins, 0);
		if (pair_hits && pair_hits->size() < links.size()) pair_hits->resize(links.size(), 0);
		check(kmx_unitig_pair_walks(h_, walks.empty() ? 0 : &walks[0], walks.size(), n_seqs ? &walk_offsets[0] : 0, n_seqs, steps.empty() ? 0 : &steps[0], steps.size(),
		                            link_offsets.empty() ? 0 : &link_offsets[0], links.empty() ? 0 : &links[0], links.size(), &params, &pairs[0], hist && !hist->empty() ? &(*hist)[0] : 0,
		                            pair_hits && !pair_hits->empty() ? &(*pair_hits)[0] : 0, plinks ? &(*plinks)[0] : 0, n + np, &n, &ps));
		if (plinks) plinks->resize((size_t)n);
		pairs.resize(np);
		if (stats) *stats = ps;
		return pairs;
	}
	// the pair links as a table, one "u<a><+|->\tu<b><+|->\t<pairs>\t<mean dist, one decimal>\t<min>\t<max>\t<link index or ->" per
	// entry: the index is that of the edge a -> b in the CSR (the first match among the first 4 entries of its row), "-" when the
	// two are not adjacent ...
	static void write_pair_links_tsv(std::ostream &out, const std::vector<kmx_pair_link> &plinks, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links)
	{
		for (size_t i = 0; i < plinks.size(); i++) {
			const kmx_pair_link &p = plinks[i];
			const uint64_t q = p.n_pairs ? (p.sum_dist * 10 + p.n_pairs / 2) / p.n_pairs : 0;
			out << "u" << (p.a >> 1) << ((p.a & 1) ? '-' : '+') << "\tu" << (p.b >> 1) << ((p.b & 1) ? '-' : '+') << "\t" << p.n_pairs << "\t" << q / 10 << "." << q % 10 << "\t" << p.min_dist << "\t"
			    << p.max_dist << "\t";
			uint64_t e = ~(uint64_t)0;
			if ((uint64_t)p.a + 1 < link_offsets.size())
				for (uint64_t t = link_offsets[p.a]; t < link_offsets[p.a + 1] && t < link_offsets[p.a] + 4 && t < links.size(); t++)
					if (links[(size_t)t] == p.b) { e = t; break; }
			if (e == ~(uint64_t)0) out << "-\n"; else out << e << "\n";
		}
	}
	// ... and the insert-size histogram, one "<bin start>\t<pairs>" per bin (the last bin also holds everything beyond it)
	static void write_insert_hist_tsv(std::ostream &out, const std::vector<uint64_t> &hist, uint32_t bin_width)
	{
		for (size_t i = 0; i < hist.size(); i++) out << (uint64_t)i * bin_width << "\t" << hist[i] << "\n";
	}

	// Scaffolds (the rule: kmx.h): unitigs or contigs ordered and oriented along the pair links seq_pairs left, spelled with runs of
	// N sized from the insert size.  unitig_scaffold takes the strings (rec may be null: the scaffolds' counts are then 0) and the
	// list; it needs no session.  The result holds the scaffolds, one kmx_scaffold each, steps (every scaffold's oriented unitigs
	// back to back, each with the N in front of it and the estimate they were sized from) and place (one per unitig: its scaffold,
	// strand, step and base offset there).  It sizes the bases with a first call, so it never comes back short.
	struct Scaffolds {
		std::vector<std::string> strs;
		std::vector<kmx_scaffold> rec;
		std::vector<kmx_scaffold_step> steps;
		std::vector<kmx_scaffold_place> place;
		kmx_scaffold_stats stats;
	};
	Scaffolds unitig_scaffold(const std::vector<std::string> &unitigs, const std::vector<kmx_unitig> *rec, const std::vector<kmx_pair_link> &plinks, int k, const kmx_scaffold_params &params)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), np = plinks.size();
		if (rec && rec->size() != U) { std::cout << "unitig_scaffold: the records are not those of the unitigs" << std::endl; exit(1); }
		Scaffolds s;
		std::vector<uint64_t> soff(U + 1, 0);
		s.rec.resize(U + 1); s.steps.resize(U + 1); s.place.resize(U + 1);
		uint64_t ns = 0, nb = 0;
		const int rc = kmx_unitig_scaffold(h_, k, f.bases.data(), f.off.data(), U, rec && U ? &(*rec)[0] : 0, np ? &plinks[0] : 0, np, &params, 0, 0, &soff[0], &s.rec[0], &s.steps[0], &s.place[0],
		                                   &ns, &nb, &s.stats);                                               // the sizing call
		if (rc != KMX_E_RANGE) check(rc);
		std::string sseq((size_t)nb + 1, '\0');
		if (rc == KMX_E_RANGE)
			check(kmx_unitig_scaffold(h_, k, f.bases.data(), f.off.data(), U, rec && U ? &(*rec)[0] : 0, np ? &plinks[0] : 0, np, &params, &sseq[0], nb, &soff[0], &s.rec[0], &s.steps[0], &s.place[0],
			                          &ns, &nb, &s.stats));
		soff.resize((size_t)ns + 1);
		s.strs = split(sseq, soff);
		s.rec.resize((size_t)ns); s.steps.resize(U); s.place.resize(U);
		return s;
	}
	// the scaffolds as FASTA, header ">s<index> n_bases=<b> n_steps=<s> n_gap_bases=<n> circular=<0|1>"
	static void write_scaffolds_fasta(std::ostream &out, const Scaffolds &s)
	{
		for (size_t i = 0; i < s.strs.size(); i++)
			out << ">s" << i << " n_bases=" << s.rec[i].n_bases << " n_steps=" << (s.rec[i].n_steps & ~KMX_SCAFFOLD_CIRCULAR) << " n_gap_bases=" << s.rec[i].n_gap_bases
			    << " circular=" << (s.rec[i].n_steps >> 31) << "\n" << s.strs[i] << "\n";
	}
	// ... every step as a table, one "s<scaffold>\t<step>\tu<unitig>\t<+|->\t<base offset in the scaffold>\t<N in front>\t<estimate>" per step ...
	static void write_scaffold_paths_tsv(std::ostream &out, const Scaffolds &s)
	{
		for (size_t i = 0; i < s.rec.size(); i++)
			for (uint64_t j = 0; j < (s.rec[i].n_steps & ~KMX_SCAFFOLD_CIRCULAR) && s.rec[i].first_step + j < s.steps.size(); j++) {
				const kmx_scaffold_step &t = s.steps[(size_t)(s.rec[i].first_step + j)];
				out << "s" << i << "\t" << j << "\tu" << (t.o >> 1) << "\t" << ((t.o & 1) ? '-' : '+') << "\t" << ((t.o >> 1) < s.place.size() ? s.place[t.o >> 1].off : 0) << "\t" << t.n_gap << "\t"
				    << (long long)t.est << "\n";
			}
	}
	// ... and as AGP 2.1: per step "s<scaffold>\t<begin>\t<end>\t<part>\tW\tu<unitig>\t1\t<length>\t<+|->", and in front of a later
	// step with N "s<scaffold>\t<begin>\t<end>\t<part>\tN\t<length>\tscaffold\tyes\tpaired-ends" (coordinates from 1, ends inclusive)
	static void write_scaffolds_agp(std::ostream &out, const Scaffolds &s, const std::vector<std::string> &unitigs)
	{
		out << "##agp-version\t2.1\n";
		for (size_t i = 0; i < s.rec.size(); i++) {
			uint64_t part = 0;
			for (uint64_t j = 0; j < (s.rec[i].n_steps & ~KMX_SCAFFOLD_CIRCULAR) && s.rec[i].first_step + j < s.steps.size(); j++) {
				const kmx_scaffold_step &t = s.steps[(size_t)(s.rec[i].first_step + j)];
				if ((t.o >> 1) >= s.place.size() || (t.o >> 1) >= unitigs.size()) continue;
				const uint64_t off = s.place[t.o >> 1].off, len = unitigs[t.o >> 1].size();
				if (j > 0 && t.n_gap > 0) out << "s" << i << "\t" << off - t.n_gap + 1 << "\t" << off << "\t" << ++part << "\tN\t" << t.n_gap << "\tscaffold\tyes\tpaired-ends\n";
				out << "s" << i << "\t" << off + 1 << "\t" << off + len << "\t" << ++part << "\tW\tu" << (t.o >> 1) << "\t1\t" << len << "\t" << ((t.o & 1) ? '-' : '+') << "\n";
			}
		}
	}

	// Pair paths (the rule: kmx.h): for every entry of the list seq_pairs left, the one path of the unitig graph between its two
	// ends whose windows fit the insert size.  pair_paths takes the unitig strings (only their lengths are used), the CSR and the
	// list; through (16 per unitig) and path_hits (one per link) are ADDED to, so the arrays unitig_through and seq_walks filled can
	// be passed as they are; an empty or shorter vector is grown with zeros first.  It needs no session, and it gives the steps
	// room for every entry, so it never comes back short.
	struct PairPaths {
		std::vector<kmx_pair_path> rec;              // one per entry of the list
		std::vector<uint32_t> steps;                 // the intermediates of the PATH entries, back to back
		kmx_pair_path_stats stats;
	};
	PairPaths pair_paths(const std::vector<std::string> &unitigs, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links, const std::vector<kmx_pair_link> &plinks, int k,
	                     const kmx_pair_path_params &params, std::vector<uint64_t> *through = 0, std::vector<uint64_t> *path_hits = 0)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), np = plinks.size(), nl = links.size();
		if (link_offsets.size() != 2 * U + 1) { std::cout << "pair_paths: the vectors are not those of one graph" << std::endl; exit(1); }
		if (through && through->size() < 16 * U) through->resize(16 * U, 0);
		if (path_hits && path_hits->size() < nl) path_hits->resize(nl, 0);
		PairPaths p;
		p.stats = kmx_pair_path_stats();
		p.rec.resize(np + 1);
		const uint64_t cap = (uint64_t)np * params.max_steps;
		p.steps.resize((size_t)cap + 1);
		uint64_t n = 0;
		check(kmx_unitig_pair_paths(h_, k, f.off.data(), U, &link_offsets[0], nl ? &links[0] : 0, nl, np ? &plinks[0] : 0, np, &params, &p.rec[0], &p.steps[0], cap, &n,
		                            through && U ? &(*through)[0] : 0, path_hits && nl ? &(*path_hits)[0] : 0, &p.stats));
		p.rec.resize(np);
		p.steps.resize((size_t)n);
		return p;
	}
	// the pair paths as a table, one "<entry>\tu<a><+|->\tu<b><+|->\t<pairs>\t<verdict>\t<windows>\t<steps>" per entry of the list: the
	// steps of a PATH with the orientation signs of reads.gaf (">u3<u5"), "*" for every other verdict
	static void write_pair_paths_tsv(std::ostream &out, const std::vector<kmx_pair_link> &plinks, const PairPaths &p)
	{
		static const char *const names[] = {"IGNORED", "BELOW_MIN", "NO_PATH", "ADJACENT", "PATH", "AMBIGUOUS", "COMPLEX"};
		for (size_t i = 0; i < plinks.size() && i < p.rec.size(); i++) {
			const kmx_pair_link &e = plinks[i];
			const kmx_pair_path &r = p.rec[i];
			out << i << "\tu" << (e.a >> 1) << ((e.a & 1) ? '-' : '+') << "\tu" << (e.b >> 1) << ((e.b & 1) ? '-' : '+') << "\t" << e.n_pairs << "\t" << (r.verdict <= KMX_PATH_COMPLEX ? names[r.verdict] : "?")
			    << "\t" << r.windows << "\t";
			uint64_t n = 0;
			if (r.verdict == KMX_PATH_PATH)
				for (uint64_t j = 0; j < r.n_steps && r.first_step + j < p.steps.size(); j++, n++) {
					const uint32_t o = p.steps[(size_t)(r.first_step + j)];
					out << ((o & 1) ? '<' : '>') << "u" << (o >> 1);
				}
			out << (n ? "\n" : "*\n");
		}
	}

	// Reduced pair lists (the rule: kmx.h): the list seq_pairs left without the entries that skip a unitig, so that the entries on
	// both sides of a short unitig become the scaffold's chain links.  pair_reduce takes the unitig strings (only their lengths are
	// used) and the list; it needs no session and no graph, and it gives the list room for every entry, so it never comes back
	// short.  unitig_scaffold, pair_paths and scaffold_fill take `list` as they take the full one.
	struct PairReduced {
		std::vector<kmx_pair_reduce> rec;            // one per entry of the input list
		std::vector<kmx_pair_link> list;             // the entries that stay, in input order
		std::vector<uint32_t> origin;                // the input index of every entry of list
		kmx_pair_reduce_stats stats;
	};
	PairReduced pair_reduce(const std::vector<std::string> &unitigs, const std::vector<kmx_pair_link> &plinks, int k, const kmx_pair_reduce_params &params)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), np = plinks.size();
		PairReduced r;
		r.stats = kmx_pair_reduce_stats();
		r.rec.resize(np + 1);
		r.list.resize(np + 1);
		r.origin.resize(np + 1);
		uint64_t n = 0;
		check(kmx_unitig_pair_reduce(h_, k, f.off.data(), U, np ? &plinks[0] : 0, np, &params, &r.rec[0], &r.list[0], &r.origin[0], np, &n, &r.stats));
		r.rec.resize(np);
		r.list.resize((size_t)n);
		r.origin.resize((size_t)n);
		return r;
	}
	// the verdicts as a table, one "<entry>\tu<a><+|->\tu<b><+|->\t<pairs>\t<verdict>\t<via>\t<n_via>\t<g>\t<delta>" per entry of the
	// input list: via with the orientation signs of reads.gaf (">u3", "<u3"), "*" for none
	static void write_pair_reduce_tsv(std::ostream &out, const std::vector<kmx_pair_link> &plinks, const PairReduced &p)
	{
		static const char *const names[] = {"IGNORED", "BELOW_MIN", "KEPT", "TRANSITIVE", "COMPLEX"};
		for (size_t i = 0; i < plinks.size() && i < p.rec.size(); i++) {
			const kmx_pair_link &e = plinks[i];
			const kmx_pair_reduce &r = p.rec[i];
			out << i << "\tu" << (e.a >> 1) << ((e.a & 1) ? '-' : '+') << "\tu" << (e.b >> 1) << ((e.b & 1) ? '-' : '+') << "\t" << e.n_pairs << "\t" << (r.verdict <= KMX_REDUCE_COMPLEX ? names[r.verdict] : "?")
			    << "\t";
			if (r.via == 0xFFFFFFFFu) out << "*";
			else out << ((r.via & 1) ? '<' : '>') << "u" << (r.via >> 1);
			out << "\t" << r.n_via << "\t" << (long long)r.g << "\t" << (long long)r.delta << "\n";
		}
	}

	// Lifted pair lists (the rule: kmx.h): the list seq_pairs left on a unitig set, rewritten in the coordinates of the contigs that
	// unitig_contigs chained those unitigs into, so that the pairs need not be mapped a second time.  pair_lift takes the unitig
	// strings (only their lengths are used), place and rec as unitig_contigs returned them and the list; it needs no session and no
	// graph, and it gives the list room for every entry, so it never comes back short.  unitig_scaffold, pair_reduce, pair_paths and
	// scaffold_fill on the contigs take `list` as they take a list mapped there.
	struct PairLifted {
		std::vector<kmx_pair_lift> rec;              // one per entry of the input list
		std::vector<kmx_pair_link> list;             // the list in contig coordinates, strictly ascending
		kmx_pair_lift_stats stats;
	};
	PairLifted pair_lift(const std::vector<std::string> &unitigs, const std::vector<kmx_contig_place> &place, const std::vector<kmx_contig> &crec, const std::vector<kmx_pair_link> &plinks, int k,
	                     const kmx_pair_lift_params &params)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), np = plinks.size();
		if (place.size() < U) die("pair_lift: place holds one entry per unitig");
		PairLifted r;
		r.stats = kmx_pair_lift_stats();
		r.rec.resize(np + 1);
		r.list.resize(np + 1);
		uint64_t n = 0;
		check(kmx_unitig_pair_lift(h_, k, f.off.data(), U, U ? &place[0] : 0, crec.empty() ? 0 : &crec[0], crec.size(), np ? &plinks[0] : 0, np, &params, &r.rec[0], &r.list[0], np, &n, &r.stats));
		r.rec.resize(np);
		r.list.resize((size_t)n);
		return r;
	}
	// the classes as a table, one "<entry>\tu<a><+|->\tu<b><+|->\t<pairs>\t<class>\tc<A><+|->\tc<B><+|->\t<shift>\t<out>" per entry of the
	// input list: "*" for the contigs of an IGNORED entry and for the out of an entry that is no LINK
	static void write_pair_lift_tsv(std::ostream &out, const std::vector<kmx_pair_link> &plinks, const PairLifted &p)
	{
		static const char *const names[] = {"IGNORED", "SAME", "INVERTED", "LINK", "FAR"};
		for (size_t i = 0; i < plinks.size() && i < p.rec.size(); i++) {
			const kmx_pair_link &e = plinks[i];
			const kmx_pair_lift &r = p.rec[i];
			out << i << "\tu" << (e.a >> 1) << ((e.a & 1) ? '-' : '+') << "\tu" << (e.b >> 1) << ((e.b & 1) ? '-' : '+') << "\t" << e.n_pairs << "\t" << (r.cls <= KMX_LIFT_FAR ? names[r.cls] : "?") << "\t";
			if (r.cls == KMX_LIFT_IGNORED) out << "*\t*";
			else out << "c" << (r.A >> 1) << ((r.A & 1) ? '-' : '+') << "\tc" << (r.B >> 1) << ((r.B & 1) ? '-' : '+');
			out << "\t" << (long long)r.shift << "\t";
			if (r.out == 0xFFFFFFFFu) out << "*";
			else out << r.out;
			out << "\n";
		}
	}

	// Filled scaffolds (the rule: kmx.h): the scaffolds spelled again, with the graph's own bases in every gap that pair_paths found
	// the one path for (kinds bit 0) and the k - 1 overlap trimmed where two steps share a graph edge (bit 1).  scaffold_fill takes
	// the unitig strings the scaffolds were made of, what unitig_scaffold and pair_paths returned on the same list, and the list;
	// it needs no session and no graph.  The result holds the strings, one kmx_scaffold_fill each, one kmx_fill_step per step in the
	// order of the scaffold's steps, and the oriented unitigs of every filled path back to back.  It sizes the bases with a first
	// call, so it never comes back short.
	struct FilledScaffolds {
		std::vector<std::string> strs;
		std::vector<kmx_scaffold_fill> rec;
		std::vector<kmx_fill_step> steps;
		std::vector<uint32_t> pieces;
		std::vector<uint32_t> n_steps;               // of the scaffold, with its circular bit
		std::vector<uint32_t> first_step;
		kmx_fill_stats stats;
	};
	FilledScaffolds scaffold_fill(const std::vector<std::string> &unitigs, const Scaffolds &scaffolds, const std::vector<kmx_pair_link> &plinks, const PairPaths &paths, int k, const kmx_fill_params &params)
	{
		const Flat f(unitigs);
		const size_t U = unitigs.size(), S = scaffolds.rec.size(), np = plinks.size(), ns = paths.steps.size();
		if (scaffolds.steps.size() != U || paths.rec.size() != np) { std::cout << "scaffold_fill: the scaffolds and paths are not those of the unitigs and the list" << std::endl; exit(1); }
		FilledScaffolds r;
		r.stats = kmx_fill_stats();
		std::vector<uint64_t> foff(S + 1, 0);
		r.rec.resize(S + 1); r.steps.resize(U + 1);
		const uint64_t pcap = (uint64_t)ns;                      // a link has one entry, so no step of a path is spelled twice
		r.pieces.resize((size_t)pcap + 1);
		uint64_t nb = 0, npc = 0;
		const int rc = kmx_unitig_scaffold_fill(h_, k, f.bases.data(), f.off.data(), U, S ? &scaffolds.rec[0] : 0, S, U ? &scaffolds.steps[0] : 0, np ? &plinks[0] : 0, np, np ? &paths.rec[0] : 0,
		                                        ns ? &paths.steps[0] : 0, ns, &params, 0, 0, &foff[0], &r.rec[0], &r.steps[0], &r.pieces[0], pcap, &nb, &npc, &r.stats);   // the sizing call
		if (rc != KMX_E_RANGE) check(rc);
		std::string fseq((size_t)nb + 1, '\0');
		if (rc == KMX_E_RANGE)
			check(kmx_unitig_scaffold_fill(h_, k, f.bases.data(), f.off.data(), U, S ? &scaffolds.rec[0] : 0, S, U ? &scaffolds.steps[0] : 0, np ? &plinks[0] : 0, np, np ? &paths.rec[0] : 0,
			                               ns ? &paths.steps[0] : 0, ns, &params, &fseq[0], nb, &foff[0], &r.rec[0], &r.steps[0], &r.pieces[0], pcap, &nb, &npc, &r.stats));
		r.strs = split(fseq, foff);
		r.rec.resize(S); r.steps.resize(U); r.pieces.resize((size_t)npc);
		for (size_t i = 0; i < S; i++) { r.n_steps.push_back(scaffolds.rec[i].n_steps); r.first_step.push_back(scaffolds.rec[i].first_step); }
		return r;
	}
	// the filled scaffolds as FASTA, header ">s<index> n_bases=<b> n_steps=<s> n_gap_bases=<n> n_fill_bases=<f> circular=<0|1>"
	static void write_filled_scaffolds_fasta(std::ostream &out, const FilledScaffolds &s)
	{
		for (size_t i = 0; i < s.strs.size() && i < s.rec.size() && i < s.n_steps.size(); i++)
			out << ">s" << i << " n_bases=" << s.rec[i].n_bases << " n_steps=" << (s.n_steps[i] & ~KMX_SCAFFOLD_CIRCULAR) << " n_gap_bases=" << s.rec[i].n_gap_bases << " n_fill_bases=" << s.rec[i].n_fill_bases
			    << " circular=" << (s.n_steps[i] >> 31) << "\n" << s.strs[i] << "\n";
	}
	// ... and every step as a table, one "s<scaffold>\t<step>\tu<unitig>\t<+|->\t<kind>\t<entry>\t<off>\t<bytes in front>\t<path>" per
	// step: "*" for no entry; the path with the orientation signs of reads.gaf (">u3<u5"), "*" for none
	static void write_scaffold_fill_tsv(std::ostream &out, const FilledScaffolds &s)
	{
		static const char *const names[] = {"HEAD", "N", "ADJACENT", "PATH"};
		for (size_t i = 0; i < s.rec.size() && i < s.n_steps.size(); i++) {
			uint64_t at = s.rec[i].first_piece;
			for (uint64_t j = 0; j < (s.n_steps[i] & ~KMX_SCAFFOLD_CIRCULAR) && s.first_step[i] + j < s.steps.size(); j++) {
				const kmx_fill_step &t = s.steps[(size_t)(s.first_step[i] + j)];
				out << "s" << i << "\t" << j << "\tu" << (t.o >> 1) << "\t" << ((t.o & 1) ? '-' : '+') << "\t" << (t.kind <= KMX_FILL_PATH ? names[t.kind] : "?") << "\t";
				if (t.entry == KMX_FILL_NO_ENTRY) out << "*"; else out << t.entry;
				out << "\t" << t.off << "\t" << t.n_front << "\t";
				uint64_t n = 0;
				for (uint64_t p = 0; p < t.n_pieces && at + p < s.pieces.size(); p++, n++) {
					const uint32_t o = s.pieces[(size_t)(at + p)];
					out << ((o & 1) ? '<' : '>') << "u" << (o >> 1);
				}
				at += t.n_pieces;
				out << (n ? "\n" : "*\n");
			}
		}
	}

	void save(std::string save_dir) { check(kmx_save(h_, save_dir.c_str())); }       // kmodel.hpp:173
	void save_model(std::string save_dir) { save(save_dir); }                          // README.md:78

	// kmodel.hpp:209 -- the model directory replaces whatever this object held (parameters come from its header)
	void load(std::string save_dir)
	{
		kmx_model *h = nullptr;
		check(kmx_load(save_dir.c_str(), &h));
		kmx_destroy(h_);
		h_ = h;
	}
	void load_model(std::string save_dir) { load(save_dir); }

	// kmodel.hpp:118, :127 -- same table, figures from kmx_get_stats
	void show_header_info()
	{
		kmx_stats st;
		kmx_get_stats(h_, &st);
		std::cout << "KMCEX:" << std::endl;
		std::cout << "   kmodel number hash                 :     " << st.nh << std::endl;
		std::cout << "   kmodel bit array                   :     " << st.nb << std::endl;
		std::cout << "   total kmercount                    :     " << st.n_total << std::endl;
		std::cout << "   kmercount in blommfilter           :     " << st.n_total - st.n_km << std::endl;
		std::cout << "   kmercount in kmodel                :     " << st.n_km << std::endl;
	}
	void show_kmodel_info()
	{
		kmx_stats st;
		kmx_get_stats(h_, &st);
		uint64_t bf = 0;
		for (int i = 0; i < st.bf_num; i++) bf += st.byte_bf[i] + st.byte_bf_back[i];
		const uint64_t km = 2 * st.km_byte_size * (uint64_t)st.nb, mb = 1024 * 1024;
		double total_s = 0;
		kmx_last_build_seconds(h_, nullptr, &total_s);
		std::cout << "   kmercount hash map                 :     " << st.rest_entries << std::endl;
		std::cout << "   memory bloomfilter                 :     " << bf / mb << "MB" << std::endl;
		std::cout << "   memory bit array                   :     " << km / mb << "MB" << std::endl;
		std::cout << "   memory rest map                    :     " << st.rest_bytes / mb << "MB" << std::endl;
		std::cout << "   total memory                       :     " << (bf + km + st.rest_bytes + st.byte_km_back) / mb << "MB" << std::endl;
		std::cout << "   build time cost                    :     " << total_s << std::endl;
	}

	kmx_model *handle() { return h_; }

private:
	size_t model_k()
	{
		kmx_stats st;
		check(kmx_get_stats(h_, &st));
		return st.k > 0 ? (size_t)st.k : 0;
	}
	static size_t windows(size_t len, size_t k) { return k && len >= k ? len - k + 1 : 0; }
	// a vector of reads as the C calls take them: the bases joined end to end and offsets[n + 1]
	struct Flat {
		std::vector<uint64_t> off;
		std::string bases;
		explicit Flat(const std::vector<std::string> &seqs) : off(seqs.size() + 1, 0)
		{
			for (size_t i = 0; i < seqs.size(); i++) off[i + 1] = off[i] + seqs[i].size();
			bases.reserve((size_t)off.back());
			for (size_t i = 0; i < seqs.size(); i++) bases += seqs[i];
		}
	};
	// ... and back: the sequences of a buffer, by its offsets
	static std::vector<std::string> split(const std::string &buf, const std::vector<uint64_t> &off)
	{
		std::vector<std::string> out(off.size() - 1);
		for (size_t i = 0; i + 1 < off.size(); i++) out[i] = buf.substr((size_t)off[i], (size_t)(off[i + 1] - off[i]));
		return out;
	}
	// one of the six unitig calls: tier 0 the strings, 1 with the links, 2 cleaned under params; kmers == 0: the counted session's
	// listing.  room: seq, seq_capacity, offsets, rec, rec_capacity, link_offsets, links, link_capacity as the C calls take them.
	struct UnitigAsk {
		const char *name;
		int tier;
		const std::vector<uint64_t> *kmers;
		const std::vector<uint32_t> *counts;
		int k;
		uint32_t thr;
		const kmx_clean_params *params;
	};
	struct UnitigRoom {
		char *seq;
		uint64_t seq_cap;
		uint64_t *off;
		kmx_unitig *rec;
		uint64_t rec_cap;
		uint64_t *lo;
		uint32_t *lk;
		uint64_t link_cap;
	};
	int unitig_c_call(const UnitigAsk &a, const UnitigRoom &r, uint64_t *nu, uint64_t *nb, uint64_t *nl, uint8_t *removed, kmx_clean_stats *stats)
	{
		if (!a.kmers)
			return a.tier == 0 ? kmx_count_unitigs(h_, a.thr, r.seq, r.seq_cap, r.off, r.rec, r.rec_cap, nu, nb)
			     : a.tier == 1 ? kmx_count_unitig_graph(h_, a.thr, r.seq, r.seq_cap, r.off, r.rec, r.rec_cap, r.lo, r.lk, r.link_cap, nu, nb, nl)
			                   : kmx_count_unitig_graph_clean(h_, a.thr, a.params, r.seq, r.seq_cap, r.off, r.rec, r.rec_cap, r.lo, r.lk, r.link_cap, nu, nb, nl, removed, stats);
		const uint64_t *km = a.kmers->data();
		const uint32_t *cnt = a.counts->data();
		const uint64_t n = a.counts->size();
		return a.tier == 0 ? kmx_unitigs(h_, a.k, km, cnt, n, a.thr, r.seq, r.seq_cap, r.off, r.rec, r.rec_cap, nu, nb)
		     : a.tier == 1 ? kmx_unitig_graph(h_, a.k, km, cnt, n, a.thr, r.seq, r.seq_cap, r.off, r.rec, r.rec_cap, r.lo, r.lk, r.link_cap, nu, nb, nl)
		                   : kmx_unitig_graph_clean(h_, a.k, km, cnt, n, a.thr, a.params, r.seq, r.seq_cap, r.off, r.rec, r.rec_cap, r.lo, r.lk, r.link_cap, nu, nb, nl, removed, stats);
	}
	// the sizing call, room for exactly that, the call, and the strings split; every output but the strings is optional
	std::vector<std::string> unitig_call(const UnitigAsk &a, std::vector<kmx_unitig> *rec, std::vector<uint64_t> *link_offsets, std::vector<uint32_t> *links, kmx_clean_stats *stats,
	                                     std::vector<uint8_t> *removed)
	{
		uint64_t nu = 0, nb = 0, nl = 0;
		const uint64_t n = a.kmers ? a.counts->size() : 0;
		if (a.kmers && a.kmers->size() != n * (uint64_t)((a.k + 31) / 32)) { std::cout << a.name << ": " << a.kmers->size() << " words for " << n << " counts" << std::endl; exit(1); }
		const UnitigRoom none = {0, 0, 0, 0, 0, 0, 0, 0};
		check(unitig_c_call(a, none, &nu, &nb, &nl, 0, 0));
		std::string bases((size_t)nb + 1, '\0');
		std::vector<uint64_t> off((size_t)nu + 1, 0), lo(2 * (size_t)nu + 1, 0);
		std::vector<kmx_unitig> r((size_t)nu + 1);
		std::vector<uint32_t> lk((size_t)nl + 1, 0);
		std::vector<uint8_t> rm((size_t)n + 1, 0);
		const UnitigRoom room = {&bases[0], nb, &off[0], &r[0], nu, &lo[0], &lk[0], nl};
		check(unitig_c_call(a, room, &nu, &nb, &nl, removed ? &rm[0] : 0, stats));
		r.resize((size_t)nu);
		lk.resize((size_t)nl);
		rm.resize((size_t)n);
		if (rec) rec->swap(r);
		if (link_offsets) link_offsets->swap(lo);
		if (links) links->swap(lk);
		if (removed) removed->swap(rm);
		return split(bases, off);
	}
	static void die(const char *msg)
	{
		std::cout << msg << std::endl;
		std::exit(1);
	}
	static void check(int rc)
	{
		if (rc != KMX_OK) die(kmx_last_error());
	}
	kmx_model *h_;
};

// kmodel.hpp:674-677
inline KModel *get_model(int ci = 1, int cs = 1023, int num_hash = 7, int num_bit = 5)
{
	kmx_model *h = nullptr;
	if (kmx_create(ci, cs, num_hash, num_bit, &h) != KMX_OK) {
		std::cout << kmx_last_error() << std::endl;
		std::exit(1);
	}
	return new KModel(h);
}

// kmodel.hpp:680-696 (load_model in the README's vocabulary)
inline KModel *get_model(std::string save_dir)
{
	kmx_model *h = nullptr;
	if (kmx_load(save_dir.c_str(), &h) != KMX_OK) {
		std::cout << kmx_last_error() << std::endl;
		std::exit(1);
	}
	return new KModel(h);
}
inline KModel *load_model(std::string save_dir) { return get_model(save_dir); }

#endif
