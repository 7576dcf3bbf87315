// Test program for include/kmodel.hpp's scaffolds: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the
// unitig graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the interleaved reads of a
// text file (one per line), thread them through the graph (seq_walks), place the pairs (seq_pairs), close the session, scaffold the
// unitigs from the list (unitig_scaffold) and write to stdout, each block closed by a line "#": the stats, the FASTA, the path
// table and the AGP.  The test compares them with the restatement.
// With the single argument "--text-only" it needs no device: it formats a hand-made result of three unitigs.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_scaffold) != 64 || sizeof(kmx_scaffold_step) != 16 || sizeof(kmx_scaffold_place) != 16 || sizeof(kmx_scaffold_stats) != 80 || sizeof(kmx_scaffold_params) != 32) return 3;
	if (argc == 2 && !strcmp(argv[1], "--text-only")) {
		// k = 5; the list (0, 3, 5, 50, 10, 10) with inner = 30, min_n = 0, max_n = 100: u0+ then 15 N then u1-, and u2 alone
		const char *u[] = {"ACGTA", "CCGGT", "TTTGA"};
		KModel::Scaffolds s;
		s.strs.push_back("ACGTANNNNNNNNNNNNNNNACCGG");
		s.strs.push_back("TTTGA");
		const kmx_scaffold r0 = {25, 2, 0, 0, 0, 0, 2, 15, 5, 5}, r1 = {5, 1, 0, 0, 0, 2, 1, 0, 0, 0};
		s.rec.push_back(r0);
		s.rec.push_back(r1);
		const kmx_scaffold_step t[] = {{0, 0, 0}, {3, 15, 15}, {4, 0, 0}};
		const kmx_scaffold_place p[] = {{0, 0, 0}, {1, 1, 20}, {2, 0, 0}};
		s.steps.assign(t, t + 3);
		s.place.assign(p, p + 3);
		KModel::write_scaffolds_fasta(std::cout, s);
		std::cout << "#\n";
		KModel::write_scaffold_paths_tsv(std::cout, s);
		std::cout << "#\n";
		KModel::write_scaffolds_agp(std::cout, s, std::vector<std::string>(u, u + 3));
		return 0;
	}
	if (argc < 12) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_pair_params par = {(uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]), 10, 64};
	const kmx_scaffold_params spar = {(uint64_t)atoll(argv[7]), (uint32_t)atol(argv[8]), (uint32_t)atol(argv[9]), (uint32_t)atol(argv[10]), (uint32_t)atol(argv[11]), 0};
	const kmx_walk_params wpar = {(uint32_t)k, 0, {0, 0}};
	std::vector<std::string> reads;
	std::ifstream in(argv[4]);
	for (std::string line; std::getline(in, line);) reads.push_back(line);
	if (reads.size() % 2) return 2;
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec;
	std::vector<uint64_t> link_offsets, so, wo;
	std::vector<uint32_t> links, steps;
	const std::vector<std::string> strs = km->count_unitig_graph(thr, &rec, &link_offsets, &links);
	km->count_unitig_map_begin(strs);
	std::vector<kmx_pair_link> plinks;
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so);
	const std::vector<kmx_walk> walks = km->seq_walks(segs, so, link_offsets, links, wpar, &wo, &steps);
	km->seq_pairs(walks, wo, steps, link_offsets, links, par, &plinks);
	km->unitig_map_end();
	const KModel::Scaffolds s = km->unitig_scaffold(strs, &rec, plinks, k, spar);
	if (s.steps.size() != strs.size() || s.place.size() != strs.size() || s.rec.size() != s.strs.size() || s.stats.n_scaffolds != s.rec.size()) return 4;
	const kmx_scaffold_stats &t = s.stats;
	std::cout << t.n_entries << " " << t.n_links << " " << t.n_ignored << " " << t.n_below_min << " " << t.n_below_ratio << " " << t.n_kept << " " << t.n_chain << " " << t.n_scaffolds << " "
	          << t.n_circular << " " << t.n_multi << "\n#\n";
	KModel::write_scaffolds_fasta(std::cout, s);
	std::cout << "#\n";
	KModel::write_scaffold_paths_tsv(std::cout, s);
	std::cout << "#\n";
	KModel::write_scaffolds_agp(std::cout, s, strs);
	delete km;
	return 0;
}
