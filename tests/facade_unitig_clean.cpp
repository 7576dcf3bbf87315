// Test program for include/kmodel.hpp's cleaned unitig graph: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads),
// clean the graph of the kept listing with count_unitig_graph_clean(thr, ops = 7, caps 2 k, 16 rounds), check that the
// uncleaned graph is afterwards what it was before, that the uncleaned sizes would have sufficed, and that unitig_graph_clean()
// on a listing read from a text file (one "word0 [word1] count" line per k-mer; "-" = none given) gives the same outputs and
// statistics, and write the cleaned graph as GFA 1 to stdout; the test compares that with the restatement's text.
// With the single argument "--compile-only" it needs no device: it checks the sizes of the two structs.
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_clean_params) != 16 || sizeof(kmx_clean_stats) != 64 || (KMX_CLEAN_TIPS | KMX_CLEAN_ISLANDS | KMX_CLEAN_BUBBLES) != 7 || KMX_CLEAN_MAX_ROUNDS != 64) return 3;
	if (argc == 2 && !strcmp(argv[1], "--compile-only")) { std::cout << "ok\n"; return 0; }
	if (argc < 5) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_clean_params P = {7, (uint32_t)(2 * k), (uint32_t)(2 * k), 16};
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec0, rec, rec1, rec2;
	std::vector<uint64_t> lo0, lo, lo1, lo2;
	std::vector<uint32_t> lk0, lk, lk1, lk2;
	kmx_clean_stats st, st2;
	const std::vector<std::string> before = km->count_unitig_graph(thr, &rec0, &lo0, &lk0);
	const std::vector<std::string> strs = km->count_unitig_graph_clean(thr, P, &rec, &lo, &lk, &st);
	if (strs.size() != rec.size() || lo.size() != 2 * strs.size() + 1 || lo[0] != 0 || lo.back() != lk.size()) return 4;
	if (st.n_unitigs_before != before.size() || st.n_links_before != lk0.size() || strs.size() > before.size() || lk.size() > lk0.size()) return 5;
	if (km->count_unitig_graph(thr, &rec1, &lo1, &lk1) != before || lo1 != lo0 || lk1 != lk0 || (rec0.size() && memcmp(&rec0[0], &rec1[0], rec0.size() * sizeof(kmx_unitig)))) return 7;
	if (km->count_unitig_graph_clean(thr, P, 0, 0, 0) != strs) return 8;
	if (strcmp(argv[4], "-")) {
		std::ifstream in(argv[4]);
		std::vector<uint64_t> kmers;
		std::vector<uint32_t> counts;
		const int W = (k + 31) / 32;
		for (std::string line; std::getline(in, line);) {
			std::istringstream ls(line);
			uint64_t w;
			for (int j = 0; j < W; j++) { ls >> w; kmers.push_back(w); }
			uint32_t c;
			ls >> c;
			counts.push_back(c);
		}
		std::vector<uint8_t> removed;
		if (km->unitig_graph_clean(kmers, counts, k, thr, P, &rec2, &lo2, &lk2, &st2, &removed) != strs || rec2.size() != rec.size() ||
		    (rec.size() && memcmp(&rec[0], &rec2[0], rec.size() * sizeof(kmx_unitig))) || lo2 != lo || lk2 != lk || memcmp(&st, &st2, sizeof st))
			return 6;
		uint64_t gone = 0;
		for (size_t i = 0; i < removed.size(); i++) gone += removed[i] != 0;
		if (removed.size() != counts.size() || gone != st.n_kmers_removed) return 9;
	}
	KModel::write_unitigs_gfa(std::cout, strs, rec, lo, lk, k);
	delete km;
	return 0;
}
