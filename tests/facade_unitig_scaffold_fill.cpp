// Test program for include/kmodel.hpp's filled scaffolds: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take
// the unitig graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the interleaved reads of
// a text file (one per line), thread them through the graph (seq_walks), place the pairs (seq_pairs), close the session, build
// the scaffolds (unitig_scaffold), find the pair paths (pair_paths) and fill the gaps (scaffold_fill), and write to stdout, each
// block closed by a line "#": the stats, the FASTA, the step table.  The test compares them with the restatement.
// With the single argument "--text-only" it needs no device: it formats a hand-made result of two scaffolds.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_scaffold_fill) != 64 || sizeof(kmx_fill_step) != 32 || sizeof(kmx_fill_stats) != 80 || sizeof(kmx_fill_params) != 8) return 3;
	if (argc == 2 && !strcmp(argv[1], "--text-only")) {
		const kmx_scaffold_fill r[] = {{14, 2, 5, 1, 1, 1, 3, 0}, {4, 0, 0, 0, 0, 0, 0, 3}};
		const kmx_fill_step s[] = {{3, KMX_FILL_HEAD, KMX_FILL_NO_ENTRY, 0, 0, 0}, {0, KMX_FILL_PATH, 7, 3, 5, 5}, {4, KMX_FILL_ADJACENT, 2, 0, 6, 0}, {9, KMX_FILL_N, KMX_FILL_NO_ENTRY, 0, 12, 2},
		                           {10, KMX_FILL_HEAD, KMX_FILL_NO_ENTRY, 0, 0, 0}};
		const uint32_t p[] = {6, 11, 12};
		KModel::FilledScaffolds f;
		f.strs.push_back("ACGTACGTACNNAC");
		f.strs.push_back("GGCC");
		f.rec.assign(r, r + 2);
		f.steps.assign(s, s + 5);
		f.pieces.assign(p, p + 3);
		f.n_steps.push_back(4 | KMX_SCAFFOLD_CIRCULAR);
		f.n_steps.push_back(1);
		f.first_step.push_back(0);
		f.first_step.push_back(4);
		KModel::write_filled_scaffolds_fasta(std::cout, f);
		std::cout << "#\n";
		KModel::write_scaffold_fill_tsv(std::cout, f);
		return 0;
	}
	if (argc < 12) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_pair_params par = {1, (uint32_t)atol(argv[5]), 10, 64};
	const kmx_scaffold_params spar = {(uint64_t)atoll(argv[6]), 0, (uint32_t)atol(argv[7]), (uint32_t)atol(argv[8]), (uint32_t)atol(argv[9]), 0};
	const kmx_pair_path_params ppar = {(uint64_t)atoll(argv[6]), (uint32_t)atol(argv[7]), (uint32_t)atol(argv[10]), 8, 4096, 0};
	const kmx_fill_params fpar = {(uint32_t)atol(argv[11]), 0};
	const kmx_walk_params wpar = {(uint32_t)k, 0, {0, 0}};
	std::vector<std::string> reads;
	std::ifstream in(argv[4]);
	for (std::string line; std::getline(in, line);) reads.push_back(line);
	if (reads.size() % 2) return 2;
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec;
	std::vector<uint64_t> link_offsets, so, wo, hits;
	std::vector<uint32_t> links, steps;
	const std::vector<std::string> strs = km->count_unitig_graph(thr, &rec, &link_offsets, &links);
	km->count_unitig_map_begin(strs);
	std::vector<kmx_pair_link> plinks;
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so);
	const std::vector<kmx_walk> walks = km->seq_walks(segs, so, link_offsets, links, wpar, &wo, &steps, &hits);
	km->seq_pairs(walks, wo, steps, link_offsets, links, par, &plinks, 0, &hits);
	km->unitig_map_end();
	const KModel::Scaffolds s = km->unitig_scaffold(strs, 0, plinks, k, spar);
	const KModel::PairPaths p = km->pair_paths(strs, link_offsets, links, plinks, k, ppar);
	const KModel::FilledScaffolds f = km->scaffold_fill(strs, s, plinks, p, k, fpar);
	if (f.rec.size() != s.rec.size() || f.steps.size() != strs.size()) return 4;
	const kmx_fill_stats &t = f.stats;
	std::cout << t.n_head << " " << t.n_path << " " << t.n_adjacent << " " << t.n_n << " " << t.n_no_entry << " " << t.n_mirror << " " << t.n_removed << " " << t.n_filled << "\n#\n";
	KModel::write_filled_scaffolds_fasta(std::cout, f);
	std::cout << "#\n";
	KModel::write_scaffold_fill_tsv(std::cout, f);
	delete km;
	return 0;
}
