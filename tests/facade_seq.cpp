// Test program for include/kmodel.hpp's sequence query: load a model directory, read one sequence per line ("-" = an empty
// one) and check seq_to_occ(read) and seq_to_occ(vector) against kmer_to_occ(vector<string>) of the read's windows.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	KModel *km = load_model(argv[1]);
	kmx_stats st;
	if (kmx_get_stats(km->handle(), &st) != KMX_OK) return 3;
	const size_t k = (size_t)st.k;
	std::ifstream in(argv[2]);
	std::vector<std::string> reads;
	for (std::string line; std::getline(in, line);) reads.push_back(line == "-" ? std::string() : line);
	std::vector<std::vector<int> > batch = km->seq_to_occ(reads);
	if (batch.size() != reads.size()) return 4;
	size_t windows = 0;
	for (size_t i = 0; i < reads.size(); i++) {
		const std::string &r = reads[i];
		std::vector<int> one = km->seq_to_occ(r);
		const size_t n = r.size() >= k ? r.size() - k + 1 : 0;
		if (one.size() != n || batch[i].size() != n) return 5;
		if (one != batch[i]) return 6;
		if (!n) continue;
		std::vector<std::string> cut;
		for (size_t p = 0; p < n; p++) cut.push_back(r.substr(p, k));
		std::vector<int> want = km->kmer_to_occ(cut, 4);
		if (want != one) { std::cout << "read " << i << " differs" << std::endl; return 7; }
		windows += n;
	}
	delete km;
	std::cout << windows << " windows ok" << std::endl;
	return 0;
}
