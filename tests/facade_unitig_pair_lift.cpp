// Test program for include/kmodel.hpp's lifted pair lists.  With the single argument "--text-only" it needs no device: it formats
// a hand-made result of five entries with write_pair_lift_tsv.  Otherwise: <k> <max_dist> <unitig lengths, comma separated>
// <place file: one "oc off" per line> <contig file: one "n_kmers" per line> <list file: one "a b n_pairs sum_dist min_dist
// max_dist" per line>: it lifts the list on the GPU (pair_lift on unitigs of those lengths) and writes to stdout, each block
// closed by a line "#": the stats, the class table, the lifted list.  The test compares them with the restatement.
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
	if (sizeof(kmx_pair_lift) != 32 || sizeof(kmx_pair_lift_stats) != 128 || sizeof(kmx_pair_lift_params) != 8) return 3;
	if (argc == 2 && !strcmp(argv[1], "--text-only")) {
		const kmx_pair_link l[] = {{0, 4, 61, 3660, 60, 60}, {0, 6, 21, 3990, 190, 190}, {3, 9, 7, 70, 10, 10}, {5, 5, 0, 0, 0, 0}, {8, 2, 1, 5, 5, 5}};
		const kmx_pair_lift r[] = {{KMX_LIFT_LINK, 2, 7, 4, 160, 1, 0}, {KMX_LIFT_SAME, 0xFFFFFFFFu, 0, 0, -33, 0, 0}, {KMX_LIFT_FAR, 0xFFFFFFFFu, 1, 9, 4000000000LL, 0, 0},
		                           {KMX_LIFT_IGNORED, 0xFFFFFFFFu, 0, 0, 0, 0, 0}, {KMX_LIFT_INVERTED, 0xFFFFFFFFu, 6, 7, 0, 0, 0}};
		KModel::PairLifted p;
		p.rec.assign(r, r + 5);
		KModel::write_pair_lift_tsv(std::cout, std::vector<kmx_pair_link>(l, l + 5), p);
		return 0;
	}
	if (argc < 7) return 2;
	const int k = atoi(argv[1]);
	const kmx_pair_lift_params par = {(uint32_t)atoll(argv[2]), 0};
	std::vector<std::string> strs;
	std::stringstream lens(argv[3]);
	for (std::string t; std::getline(lens, t, ',');) strs.push_back(std::string((size_t)atol(t.c_str()), 'A'));
	std::vector<kmx_contig_place> place;
	std::ifstream pin(argv[4]);
	for (std::string line; std::getline(pin, line);) {
		std::stringstream s(line);
		kmx_contig_place e;
		if (s >> e.oc >> e.off) place.push_back(e);
	}
	std::vector<kmx_contig> crec;
	std::ifstream cin_(argv[5]);
	for (std::string line; std::getline(cin_, line);) {
		std::stringstream s(line);
		kmx_contig e = kmx_contig();
		if (s >> e.n_kmers) crec.push_back(e);
	}
	std::vector<kmx_pair_link> plinks;
	std::ifstream in(argv[6]);
	for (std::string line; std::getline(in, line);) {
		std::stringstream s(line);
		kmx_pair_link e;
		if (s >> e.a >> e.b >> e.n_pairs >> e.sum_dist >> e.min_dist >> e.max_dist) plinks.push_back(e);
	}
	KModel *km = get_model(1, 1023, 3, 2);
	const KModel::PairLifted p = km->pair_lift(strs, place, crec, plinks, k, par);
	if (p.rec.size() != plinks.size() || p.stats.n_entries != plinks.size() || p.list.size() != p.stats.n_out) return 4;
	const kmx_pair_lift_stats &t = p.stats;
	std::cout << t.n_entries << " " << t.n_ignored << " " << t.n_same << " " << t.n_inverted << " " << t.n_link << " " << t.n_far << " " << t.n_same_back << " " << t.n_out << " " << t.pairs_ignored
	          << " " << t.pairs_same << " " << t.pairs_inverted << " " << t.pairs_link << " " << t.pairs_far << " " << t.pairs_same_back << " " << (long long)t.sum_same_d << "\n#\n";
	KModel::write_pair_lift_tsv(std::cout, plinks, p);
	std::cout << "#\n";
	for (size_t i = 0; i < p.list.size(); i++)
		std::cout << p.list[i].a << " " << p.list[i].b << " " << p.list[i].n_pairs << " " << p.list[i].sum_dist << " " << p.list[i].min_dist << " " << p.list[i].max_dist << "\n";
	delete km;
	return 0;
}
