// Test program for include/kmodel.hpp's path extension: load a model directory, read one seed per line ("-" = an empty
// one), extend them with seq_extend(vector) and every 7th also with seq_extend(seed), and print the appended bases and the
// records' fields, one line per seed; the test compares them with the reference rule.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (argc < 6) return 2;
	if (sizeof(kmx_seq_extension) != 32) return 3;
	KModel *km = load_model(argv[1]);
	const int thr = atoi(argv[3]), max_ext = atoi(argv[4]), depth = atoi(argv[5]);
	std::ifstream in(argv[2]);
	std::vector<std::string> seeds;
	for (std::string line; std::getline(in, line);) seeds.push_back(line == "-" ? std::string() : line);
	std::vector<kmx_seq_extension> rec;
	std::vector<std::string> ext = km->seq_extend(seeds, thr, max_ext, depth, &rec), plain = km->seq_extend(seeds, thr, max_ext, depth);
	if (ext.size() != seeds.size() || rec.size() != seeds.size() || plain != ext) return 4;
	for (size_t i = 0; i < seeds.size(); i++) {
		if (ext[i].size() != rec[i].n_ext) return 5;
		if (i % 7 == 0) {
			kmx_seq_extension one;
			if (km->seq_extend(seeds[i], thr, max_ext, depth, &one) != ext[i] || memcmp(&one, &rec[i], sizeof one) || km->seq_extend(seeds[i], thr, max_ext, depth) != ext[i]) {
				std::cout << "seed " << i << " differs (single)" << std::endl;
				return 6;
			}
		}
		const kmx_seq_extension &r = rec[i];
		std::cout << (ext[i].empty() ? "-" : ext[i]) << " " << r.n_ext << " " << r.stop << " " << r.seed_occ << " " << r.min_occ << " " << r.max_occ << " " << r.n_lookahead << " "
		          << r.sum_occ << "\n";
	}
	if (!km->seq_extend(std::vector<std::string>(), thr, max_ext, depth).empty()) return 7;
	delete km;
	std::cout << "ok" << std::endl;
	return 0;
}
