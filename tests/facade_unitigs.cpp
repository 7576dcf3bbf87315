// Test program for include/kmodel.hpp's unitigs: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the
// unitigs of the kept listing with count_unitigs(thr), check them against unitigs() on a listing read from a text file (one
// "word0 [word1] count" line per k-mer; "-" = none given), and write them as FASTA to stdout; the test parses that back.
// With the single argument "--fasta-only" it needs no device: it formats two hand-made records.
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
	if (argc == 2 && !strcmp(argv[1], "--fasta-only")) {
		std::vector<std::string> strs;
		strs.push_back("ACGTACG");
		strs.push_back("TTTTTGA");
		std::vector<kmx_unitig> rec(2);
		memset(&rec[0], 0, 2 * sizeof(kmx_unitig));
		rec[0].n_kmers = 3; rec[0].sum_count = 10;
		rec[1].n_kmers = 3; rec[1].sum_count = 3; rec[1].circular = 1;
		KModel::write_unitigs_fasta(std::cout, strs, rec);
		return 0;
	}
	if (argc < 5) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec, rec2;
	const std::vector<std::string> strs = km->count_unitigs(thr, &rec), plain = km->count_unitigs(thr);
	if (strs.size() != rec.size() || plain != strs) return 4;
	for (size_t u = 0; u < strs.size(); u++)
		if (strs[u].size() != rec[u].n_kmers + k - 1) return 5;
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
		if (km->unitigs(kmers, counts, k, thr, &rec2) != strs || rec2.size() != rec.size() || (rec.size() && memcmp(&rec[0], &rec2[0], rec.size() * sizeof(kmx_unitig)))) return 6;
	}
	KModel::write_unitigs_fasta(std::cout, strs, rec);
	delete km;
	return 0;
}
