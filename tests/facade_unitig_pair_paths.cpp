// Test program for include/kmodel.hpp's pair paths: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the
// unitig graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the interleaved reads of a
// text file (one per line), thread them through the graph (seq_walks), count the through hits (unitig_through), place the pairs
// (seq_pairs), close the session, find the pair paths (pair_paths, added to the walks' through and link hits), resolve
// (unitig_resolve) and merge (unitig_contigs), and write to stdout, each block closed by a line "#": the stats, the path table,
// the resolve counts, the contigs one per line.  The test compares them with the restatement.
// With the single argument "--text-only" it needs no device: it formats a hand-made result of five entries.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_pair_path) != 32 || sizeof(kmx_pair_path_stats) != 80 || sizeof(kmx_pair_path_params) != 32) return 3;
	if (argc == 2 && !strcmp(argv[1], "--text-only")) {
		const kmx_pair_link l[] = {{0, 4, 91, 8190, 90, 90}, {0, 6, 130, 28600, 220, 220}, {3, 9, 7, 70, 10, 10}, {5, 5, 0, 0, 0, 0}, {8, 2, 1, 5, 5, 5}};
		const kmx_pair_path r[] = {{KMX_PATH_PATH, 1, 0, 130, 1, 2}, {KMX_PATH_ADJACENT, 0, 1, 0, 1, 1}, {KMX_PATH_PATH, 3, 1, 73, 1, 4}, {KMX_PATH_IGNORED, 0, 0, 0, 0, 0},
		                           {KMX_PATH_BELOW_MIN, 0, 0, 0, 0, 0}};
		const uint32_t s[] = {6, 11, 12, 15};
		KModel::PairPaths p;
		p.rec.assign(r, r + 5);
		p.steps.assign(s, s + 4);
		KModel::write_pair_paths_tsv(std::cout, std::vector<kmx_pair_link>(l, l + 5), p);
		return 0;
	}
	if (argc < 13) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_pair_params par = {(uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]), 10, 64};
	const kmx_pair_path_params ppar = {(uint64_t)atoll(argv[7]), (uint32_t)atol(argv[8]), (uint32_t)atol(argv[9]), (uint32_t)atol(argv[10]), (uint32_t)atol(argv[11]), 0};
	const kmx_resolve_params rpar = {(uint64_t)atoll(argv[12]), 0};
	const kmx_walk_params wpar = {(uint32_t)k, 0, {0, 0}};
	std::vector<std::string> reads;
	std::ifstream in(argv[4]);
	for (std::string line; std::getline(in, line);) reads.push_back(line);
	if (reads.size() % 2) return 2;
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec;
	std::vector<uint64_t> link_offsets, so, wo, hits, through;
	std::vector<uint32_t> links, steps;
	const std::vector<std::string> strs = km->count_unitig_graph(thr, &rec, &link_offsets, &links);
	km->count_unitig_map_begin(strs);
	std::vector<kmx_pair_link> plinks;
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so);
	const std::vector<kmx_walk> walks = km->seq_walks(segs, so, link_offsets, links, wpar, &wo, &steps, &hits);
	km->unitig_through(walks, steps, link_offsets, links, through);
	km->seq_pairs(walks, wo, steps, link_offsets, links, par, &plinks, 0, &hits);
	km->unitig_map_end();
	const KModel::PairPaths p = km->pair_paths(strs, link_offsets, links, plinks, k, ppar, &through, &hits);
	if (p.rec.size() != plinks.size() || p.stats.n_entries != plinks.size()) return 4;
	const kmx_pair_path_stats &t = p.stats;
	std::cout << t.n_entries << " " << t.n_ignored << " " << t.n_below_min << " " << t.n_no_path << " " << t.n_adjacent << " " << t.n_path << " " << t.n_ambiguous << " " << t.n_complex << " "
	          << t.n_added << " " << t.n_missing << "\n#\n";
	KModel::write_pair_paths_tsv(std::cout, plinks, p);
	std::cout << "#\n";
	const KModel::Resolved r = km->unitig_resolve(strs, &rec, link_offsets, links, &hits, through, k, rpar);
	std::cout << r.stats.n_candidates << " " << r.stats.n_resolved << " " << r.stats.n_unsupported << "\n#\n";
	const kmx_contig_params cpar = {1, 0, 0};
	const KModel::Contigs c = km->unitig_contigs(r.strs, &r.rec, r.link_offsets, r.links, r.link_hits, k, cpar);
	for (size_t i = 0; i < c.strs.size(); i++) std::cout << c.strs[i] << "\n";
	delete km;
	return 0;
}
