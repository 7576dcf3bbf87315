// Test program for include/kmodel.hpp's walks: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the unitig
// graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the reads of a text file (one per
// line), thread the segments through the graph (seq_walks) and write to stdout, each block closed by a line "#": every field of
// every walk, walk_offsets, the steps, link_hits, the stats, the GAF text and the link table.  The test compares them with the
// restatement.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_walk) != 80 || sizeof(kmx_walk_stats) != 64 || sizeof(kmx_walk_params) != 16) return 3;
	if (argc < 7) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_walk_params par = {(uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]), {0, 0}};
	std::vector<std::string> reads;
	std::ifstream in(argv[4]);
	for (std::string line; std::getline(in, line);) reads.push_back(line);
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec;
	std::vector<uint64_t> link_offsets;
	std::vector<uint32_t> links;
	const std::vector<std::string> strs = km->count_unitig_graph(thr, &rec, &link_offsets, &links);
	km->count_unitig_map_begin(strs);
	std::vector<uint64_t> so, wo, off(reads.size() + 1, 0), link_hits(links.size(), 0);
	std::vector<uint32_t> steps;
	kmx_walk_stats st;
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so);
	const std::vector<kmx_walk> walks = km->seq_walks(segs, so, link_offsets, links, par, &wo, &steps, &link_hits, &st);
	if (wo.size() != reads.size() + 1 || wo.back() != walks.size() || st.n_walks != walks.size() || st.n_steps != steps.size()) return 4;
	if (km->seq_walks(segs, so, link_offsets, links, par).size() != walks.size()) return 5;   // without the optional outputs
	km->unitig_map_end();
	for (size_t i = 0; i < reads.size(); i++) off[i + 1] = off[i] + reads[i].size();
	for (size_t i = 0; i < walks.size(); i++) {
		const kmx_walk &w = walks[i];
		std::cout << w.pos << " " << w.n_span << " " << w.n_mapped << " " << w.n_covered << " " << w.first_seg << " " << w.first_step << " " << w.n_segs << " " << w.n_steps << " "
		          << w.off_first << " " << w.off_last << " " << w.n_inside << " " << w.n_across << " " << w.indel << " " << w.reserved << "\n";
	}
	std::cout << "#\n";
	for (size_t i = 0; i < wo.size(); i++) std::cout << wo[i] << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < steps.size(); i++) std::cout << steps[i] << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < link_hits.size(); i++) std::cout << link_hits[i] << "\n";
	std::cout << "#\n";
	std::cout << st.n_walks << " " << st.n_steps << " " << st.n_edge << " " << st.n_inside << " " << st.n_across << " " << st.n_unlinked << " " << st.n_breaks << " " << st.reserved << "\n#\n";
	KModel::write_walks_gaf(std::cout, walks, wo, steps, off, strs, k);
	std::cout << "#\n";
	KModel::write_link_hits_tsv(std::cout, link_offsets, links, link_hits);
	delete km;
	return 0;
}
