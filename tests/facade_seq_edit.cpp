// Test program for include/kmodel.hpp's read editing: load a model directory, read one sequence per line ("-" = an empty
// one), edit them with seq_edit(vector) and every 7th also with seq_edit(read), and print the edited reads and the
// records' counters, one line per read; the test compares them with the reference rule.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (argc < 6) return 2;
	if (sizeof(kmx_seq_edits) != 80 || sizeof(kmx_edit) != 8) return 3;
	KModel *km = load_model(argv[1]);
	const int thr = atoi(argv[3]), min_support = atoi(argv[4]), ops = atoi(argv[5]);
	std::ifstream in(argv[2]);
	std::vector<std::string> reads;
	for (std::string line; std::getline(in, line);) reads.push_back(line == "-" ? std::string() : line);
	std::vector<kmx_seq_edits> rec;
	std::vector<std::string> fixed = km->seq_edit(reads, thr, min_support, ops, &rec), plain = km->seq_edit(reads, thr, min_support, ops);
	if (fixed.size() != reads.size() || rec.size() != reads.size() || plain != fixed) return 4;
	for (size_t i = 0; i < reads.size(); i++) {
		if (fixed[i].size() != rec[i].out_len) return 5;
		if (i % 7 == 0) {
			kmx_seq_edits one;
			if (km->seq_edit(reads[i], thr, min_support, ops, &one) != fixed[i] || memcmp(&one, &rec[i], sizeof one) || km->seq_edit(reads[i], thr, min_support, ops) != fixed[i]) {
				std::cout << "read " << i << " differs (single)" << std::endl;
				return 6;
			}
		}
		const kmx_seq_edits &r = rec[i];
		std::cout << (fixed[i].empty() ? "-" : fixed[i]) << " " << r.n_windows << " " << r.n_weak << " " << r.n_runs << " " << r.n_sites << " " << r.n_sub << " " << r.n_del << " "
		          << r.n_ins << " " << r.n_ambiguous << " " << r.n_unfixable << " " << r.out_len << "\n";
	}
	if (!km->seq_edit(std::vector<std::string>(), thr, min_support, ops).empty()) return 7;
	delete km;
	std::cout << "ok" << std::endl;
	return 0;
}
