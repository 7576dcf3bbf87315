// Test program for include/kmodel.hpp's unitig graph: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take
// the graph of the kept listing with count_unitig_graph(thr), check that its strings and records are count_unitigs' and that
// unitig_graph() on a listing read from a text file (one "word0 [word1] count" line per k-mer; "-" = none given) gives the
// same five outputs, and write it as GFA 1 to stdout; the test compares that with the restatement's text.
// With the single argument "--gfa-only" it needs no device: it formats a hand-made graph of three unitigs at k = 5.
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_unitig) != 40) return 3;
	if (argc == 2 && !strcmp(argv[1], "--gfa-only")) {
		// u0 -> u1 and u0 -> u2- (with their mirrors), a hairpin u1+ -> u1-, a self-loop u2+ -> u2+ (its mirror u2- -> u2-)
		std::vector<std::string> strs;
		strs.push_back("ACGTACG");
		strs.push_back("TTTTTGA");
		strs.push_back("CCCCC");
		std::vector<kmx_unitig> rec(3);
		memset(&rec[0], 0, 3 * sizeof(kmx_unitig));
		rec[0].n_kmers = 3; rec[0].sum_count = 10;
		rec[1].n_kmers = 3; rec[1].sum_count = 3;
		rec[2].n_kmers = 1; rec[2].sum_count = 4294967296ULL * 3;
		const uint64_t lo[] = {0, 2, 2, 3, 4, 6, 7};
		const uint32_t lk[] = {2, 5, 3, 1, 4, 1, 5};
		KModel::write_unitigs_gfa(std::cout, strs, rec, std::vector<uint64_t>(lo, lo + 7), std::vector<uint32_t>(lk, lk + 7), 5);
		return 0;
	}
	if (argc < 5) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec, rec1, rec2;
	std::vector<uint64_t> lo, lo2;
	std::vector<uint32_t> lk, lk2;
	const std::vector<std::string> strs = km->count_unitig_graph(thr, &rec, &lo, &lk), plain = km->count_unitigs(thr, &rec1);
	if (strs.size() != rec.size() || plain != strs || rec1.size() != rec.size() || (rec.size() && memcmp(&rec[0], &rec1[0], rec.size() * sizeof(kmx_unitig)))) return 4;
	if (lo.size() != 2 * strs.size() + 1 || lo[0] != 0 || lo.back() != lk.size()) return 5;
	if (km->count_unitig_graph(thr, 0, 0, 0) != strs) return 7;
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
		if (km->unitig_graph(kmers, counts, k, thr, &rec2, &lo2, &lk2) != strs || rec2.size() != rec.size() || (rec.size() && memcmp(&rec[0], &rec2[0], rec.size() * sizeof(kmx_unitig))) ||
		    lo2 != lo || lk2 != lk)
			return 6;
	}
	KModel::write_unitigs_gfa(std::cout, strs, rec, lo, lk, k);
	delete km;
	return 0;
}
