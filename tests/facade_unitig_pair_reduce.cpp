// Test program for include/kmodel.hpp's reduced pair lists.  With the single argument "--text-only" it needs no device: it formats
// a hand-made result of five entries with write_pair_reduce_tsv.  Otherwise: <k> <min_pairs> <inner> <tol> <max_row> <unitig
// lengths, comma separated> <list file: one "a b n_pairs sum_dist min_dist max_dist" per line>: it reduces the list on the GPU
// (pair_reduce on unitigs of those lengths) and writes to stdout, each block closed by a line "#": the stats, the verdict table,
// the entries that stay with their origin.  The test compares them with the restatement.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_pair_reduce) != 32 || sizeof(kmx_pair_reduce_stats) != 80 || sizeof(kmx_pair_reduce_params) != 24) return 3;
	if (argc == 2 && !strcmp(argv[1], "--text-only")) {
		const kmx_pair_link l[] = {{0, 4, 61, 3660, 60, 60}, {0, 6, 21, 3990, 190, 190}, {3, 9, 7, 70, 10, 10}, {5, 5, 0, 0, 0, 0}, {8, 2, 1, 5, 5, 5}};
		const kmx_pair_reduce r[] = {{KMX_REDUCE_TRANSITIVE, 7, 2, 1, 160, -3}, {KMX_REDUCE_KEPT, 0xFFFFFFFFu, 0, 0, 30, 0}, {KMX_REDUCE_COMPLEX, 0xFFFFFFFFu, 0, 1, -12, 0},
		                             {KMX_REDUCE_IGNORED, 0xFFFFFFFFu, 0, 0, 0, 0}, {KMX_REDUCE_BELOW_MIN, 0xFFFFFFFFu, 0, 0, 0, 0}};
		KModel::PairReduced p;
		p.rec.assign(r, r + 5);
		KModel::write_pair_reduce_tsv(std::cout, std::vector<kmx_pair_link>(l, l + 5), p);
		return 0;
	}
	if (argc < 8) return 2;
	const int k = atoi(argv[1]);
	const kmx_pair_reduce_params par = {(uint64_t)atoll(argv[2]), (uint32_t)atol(argv[3]), (uint32_t)atol(argv[4]), (uint32_t)atol(argv[5]), 0};
	std::vector<std::string> strs;
	std::stringstream lens(argv[6]);
	for (std::string t; std::getline(lens, t, ',');) strs.push_back(std::string((size_t)atol(t.c_str()), 'A'));
	std::vector<kmx_pair_link> plinks;
	std::ifstream in(argv[7]);
	for (std::string line; std::getline(in, line);) {
		std::stringstream s(line);
		kmx_pair_link e;
		if (s >> e.a >> e.b >> e.n_pairs >> e.sum_dist >> e.min_dist >> e.max_dist) plinks.push_back(e);
	}
	KModel *km = get_model(1, 1023, 3, 2);
	const KModel::PairReduced p = km->pair_reduce(strs, plinks, k, par);
	if (p.rec.size() != plinks.size() || p.stats.n_entries != plinks.size() || p.list.size() != p.stats.n_out || p.origin.size() != p.list.size()) return 4;
	const kmx_pair_reduce_stats &t = p.stats;
	std::cout << t.n_entries << " " << t.n_ignored << " " << t.n_below_min << " " << t.n_kept << " " << t.n_transitive << " " << t.n_complex << " " << t.n_out << " " << t.n_rows << " "
	          << t.n_examined << "\n#\n";
	KModel::write_pair_reduce_tsv(std::cout, plinks, p);
	std::cout << "#\n";
	for (size_t i = 0; i < p.list.size(); i++) std::cout << p.origin[i] << " " << p.list[i].a << " " << p.list[i].b << " " << p.list[i].n_pairs << " " << p.list[i].sum_dist << "\n";
	delete km;
	return 0;
}
