// Test program for include/kmodel.hpp under concurrent callers: load a model directory, answer a file of k-mer strings
// (1) the way the reference's own batch query does it -- an OpenMP loop over the single-string overload on ONE object
//     (kmodel.hpp:90-98) -- and (2) from 4 std::threads, each sending its own slice through the vector<string> overload
//     (the last slice with strings of other lengths mixed in); print the answers of (1), then those of (2), one per line.
// Exit status 3: a mixed-length answer differs from the same string asked alone, after the threads have finished.
#include <cstddef>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	KModel *km = load_model(argv[1]);
	std::ifstream in(argv[2]);
	std::vector<std::string> q;
	for (std::string line; std::getline(in, line);)
		if (!line.empty()) q.push_back(line);
	const long n = (long)q.size();

	std::vector<int> scalar(n, -1);
#pragma omp parallel for num_threads(8)
	for (long i = 0; i < n; i++) scalar[i] = km->kmer_to_occ(q[i]);

	const int T = 4;
	std::vector<int> batch(n, -1);
	std::vector<std::string> mixed;                                  // the last slice, with shorter strings interleaved
	std::vector<long> mixed_at;                                      // its entries' index in q, or -1 for an inserted string
	std::vector<int> mixed_occ;
	std::vector<std::thread> th;
	for (int t = 0; t < T; t++) {
		const long lo = n * t / T, hi = n * (t + 1) / T;
		if (t == T - 1) {
			for (long i = lo; i < hi; i++) {
				mixed.push_back(q[i]);
				mixed_at.push_back(i);
				if (i % 5 == 0) { mixed.push_back(q[i].substr(0, 20 + i % 9)); mixed_at.push_back(-1); }
			}
			th.emplace_back([&] { mixed_occ = km->kmer_to_occ(mixed, 4); });
			continue;
		}
		th.emplace_back([&, lo, hi] {
			std::vector<std::string> part(q.begin() + lo, q.begin() + hi);
			std::vector<int> occ = km->kmer_to_occ(part, 4);
			for (long i = lo; i < hi; i++) batch[i] = occ[i - lo];
		});
	}
	for (auto &x : th) x.join();
	for (size_t j = 0; j < mixed.size(); j++) {
		if (mixed_at[j] >= 0) batch[mixed_at[j]] = mixed_occ[j];
		else if (km->kmer_to_occ(mixed[j]) != mixed_occ[j]) return 3;
	}

	for (long i = 0; i < n; i++) std::cout << scalar[i] << "\n";
	for (long i = 0; i < n; i++) std::cout << batch[i] << "\n";
	delete km;
	cout.flush();
	return 0;
}
