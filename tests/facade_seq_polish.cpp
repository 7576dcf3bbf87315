// Test program for include/kmodel.hpp's read polishing: load a model directory, read one sequence per line ("-" = an empty
// one), polish them with seq_polish(vector) and every 7th also with seq_polish(read), and print the polished reads and the
// records' twelve fields, one line per read; the test compares them with the loop of seq_edit and apply_edits.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (argc < 7) return 2;
	if (sizeof(kmx_seq_polish) != 96 || KMX_POLISH_MAX_PASSES != 16) return 3;
	KModel *km = load_model(argv[1]);
	const int thr = atoi(argv[3]), min_support = atoi(argv[4]), ops = atoi(argv[5]), max_passes = atoi(argv[6]);
	std::ifstream in(argv[2]);
	std::vector<std::string> reads;
	for (std::string line; std::getline(in, line);) reads.push_back(line == "-" ? std::string() : line);
	std::vector<kmx_seq_polish> rec;
	std::vector<std::string> fixed = km->seq_polish(reads, thr, min_support, ops, max_passes, &rec), plain = km->seq_polish(reads, thr, min_support, ops, max_passes);
	if (fixed.size() != reads.size() || rec.size() != reads.size() || plain != fixed) return 4;
	for (size_t i = 0; i < reads.size(); i++) {
		if (fixed[i].size() != rec[i].out_len) return 5;
		if (i % 7 == 0) {
			kmx_seq_polish one;
			if (km->seq_polish(reads[i], thr, min_support, ops, max_passes, &one) != fixed[i] || memcmp(&one, &rec[i], sizeof one) || km->seq_polish(reads[i], thr, min_support, ops, max_passes) != fixed[i]) {
				std::cout << "read " << i << " differs (single)" << std::endl;
				return 6;
			}
		}
		const kmx_seq_polish &r = rec[i];
		std::cout << (fixed[i].empty() ? "-" : fixed[i]) << " " << r.n_passes << " " << r.converged << " " << r.n_sub << " " << r.n_del << " " << r.n_ins << " " << r.out_len << " "
		          << r.n_windows << " " << r.n_weak << " " << r.n_runs << " " << r.n_sites << " " << r.n_ambiguous << " " << r.n_unfixable << "\n";
	}
	if (!km->seq_polish(std::vector<std::string>(), thr, min_support, ops, max_passes).empty()) return 7;
	delete km;
	std::cout << "ok" << std::endl;
	return 0;
}
