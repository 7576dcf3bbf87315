// Test program for include/kmodel.hpp's read correction: load a model directory, read one sequence per line ("-" = an empty
// one), correct them with seq_correct(vector) and every 7th also with seq_correct(read), and print the corrected reads and
// the records' counters, one line per read; the test compares them with the reference rule.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (argc < 5) return 2;
	if (sizeof(kmx_seq_correction) != 64) return 3;
	KModel *km = load_model(argv[1]);
	const int thr = atoi(argv[3]), min_support = atoi(argv[4]);
	std::ifstream in(argv[2]);
	std::vector<std::string> reads;
	for (std::string line; std::getline(in, line);) reads.push_back(line == "-" ? std::string() : line);
	std::vector<kmx_seq_correction> rec;
	std::vector<std::string> fixed = km->seq_correct(reads, thr, min_support, &rec), plain = km->seq_correct(reads, thr, min_support);
	if (fixed.size() != reads.size() || rec.size() != reads.size() || plain != fixed) return 4;
	for (size_t i = 0; i < reads.size(); i++) {
		if (fixed[i].size() != reads[i].size()) return 5;
		if (i % 7 == 0) {
			kmx_seq_correction one;
			if (km->seq_correct(reads[i], thr, min_support, &one) != fixed[i] || memcmp(&one, &rec[i], sizeof one) || km->seq_correct(reads[i], thr, min_support) != fixed[i]) {
				std::cout << "read " << i << " differs (single)" << std::endl;
				return 6;
			}
		}
		const kmx_seq_correction &r = rec[i];
		std::cout << (fixed[i].empty() ? "-" : fixed[i]) << " " << r.n_windows << " " << r.n_weak << " " << r.n_runs << " " << r.n_sites << " " << r.n_corrected << " "
		          << r.n_ambiguous << " " << r.n_unfixable << " " << r.reserved << "\n";
	}
	if (!km->seq_correct(std::vector<std::string>(), thr, min_support).empty()) return 7;
	delete km;
	std::cout << "ok" << std::endl;
	return 0;
}
