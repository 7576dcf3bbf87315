// Test program for include/kmodel.hpp's per-sequence summary: load a model directory, read one sequence per line ("-" = an
// empty one) and check seq_summary(read) and seq_summary(vector) against a reduction of seq_to_occ's vectors written here.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

static kmx_seq_summary reduce(const std::vector<int> &occ, const std::vector<int> &thr)
{
	kmx_seq_summary r;
	memset(&r, 0, sizeof r);
	r.n_windows = occ.size();
	r.min = r.max = -1;
	r.first_below = r.last_below = occ.size();
	for (size_t p = 0; p < occ.size(); p++) {
		r.sum += (uint64_t)occ[p];
		if (p == 0 || occ[p] < r.min) r.min = occ[p];
		if (p == 0 || occ[p] > r.max) r.max = occ[p];
		for (size_t j = 0; j < thr.size(); j++) r.n_ge[j] += occ[p] >= thr[j];
		if (!thr.empty() && occ[p] < thr[0]) {
			if (r.first_below == occ.size()) r.first_below = p;
			r.last_below = p;
		}
	}
	return r;
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	if (sizeof(kmx_seq_summary) != 64) return 3;
	KModel *km = load_model(argv[1]);
	std::ifstream in(argv[2]);
	std::vector<std::string> reads;
	for (std::string line; std::getline(in, line);) reads.push_back(line == "-" ? std::string() : line);
	std::vector<int> thr;
	thr.push_back(1); thr.push_back(3); thr.push_back(8);
	std::vector<std::vector<int> > occ = km->seq_to_occ(reads);
	std::vector<kmx_seq_summary> batch = km->seq_summary(reads, thr), plain = km->seq_summary(reads);
	if (batch.size() != reads.size() || plain.size() != reads.size()) return 4;
	size_t windows = 0;
	for (size_t i = 0; i < reads.size(); i++) {
		const kmx_seq_summary want = reduce(occ[i], thr), want0 = reduce(occ[i], std::vector<int>());
		if (memcmp(&batch[i], &want, sizeof want) || memcmp(&plain[i], &want0, sizeof want0)) { std::cout << "read " << i << " differs (batch)" << std::endl; return 5; }
		if (i % 7 == 0) {
			const kmx_seq_summary one = km->seq_summary(reads[i], thr), one0 = km->seq_summary(reads[i]);
			if (memcmp(&one, &want, sizeof want) || memcmp(&one0, &want0, sizeof want0)) { std::cout << "read " << i << " differs (single)" << std::endl; return 6; }
		}
		windows += (size_t)want.n_windows;
	}
	if (!km->seq_summary(std::vector<std::string>(), thr).empty()) return 7;
	delete km;
	std::cout << windows << " windows ok" << std::endl;
	return 0;
}
