// Test program for include/kmodel.hpp's through hits and resolution: count the k-mers of a FASTA / FASTQ file on the GPU
// (init_reads), take the unitig graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the reads
// of a text file (one per line), thread them through the graph (seq_walks at max_gap, max_indel), count the through hits
// (unitig_through), resolve (unitig_resolve at min_reads, max_cross), build the contigs of the resolved graph (unitig_contigs at
// (1, 0)) and write to stdout, each block closed by a line "#": the through hits, the new strings, origin, place, the new CSR with
// link_origin and the hits, the two stats, the resolved table, the contigs' FASTA.  The test compares them with the restatement.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_resolve_params) != 16 || sizeof(kmx_resolve_place) != 8 || sizeof(kmx_resolve_stats) != 64 || sizeof(kmx_through_stats) != 64) return 3;
	if (argc < 9) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_walk_params par = {(uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]), {0, 0}};
	const kmx_resolve_params rp = {(uint64_t)atoll(argv[7]), (uint64_t)atoll(argv[8])};
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
	std::vector<uint64_t> so, link_hits(links.size(), 0), through;
	std::vector<uint32_t> steps;
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so);
	const std::vector<kmx_walk> walks = km->seq_walks(segs, so, link_offsets, links, par, 0, &steps, &link_hits);
	km->unitig_map_end();
	const kmx_through_stats ts = km->unitig_through(walks, steps, link_offsets, links, through);
	const KModel::Resolved r = km->unitig_resolve(strs, &rec, link_offsets, links, &link_hits, through, k, rp);
	if (r.origin.size() != r.strs.size() || r.rec.size() != r.strs.size() || r.place.size() != strs.size() || r.link_offsets.size() != 2 * r.strs.size() + 1 || r.links.size() != links.size()) return 4;
	if (km->unitig_resolve(strs, 0, link_offsets, links, 0, through, k, rp).links != r.links) return 5;   // without records and hits
	for (size_t i = 0; i < through.size(); i++) std::cout << through[i] << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < r.strs.size(); i++) std::cout << r.strs[i] << " " << r.origin[i] << " " << (int)r.rec[i].n_pred << " " << (int)r.rec[i].n_succ << " " << r.rec[i].sum_count << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < r.place.size(); i++) std::cout << r.place[i].first << " " << r.place[i].n_copies << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < r.link_offsets.size(); i++) std::cout << r.link_offsets[i] << "\n";
	for (size_t i = 0; i < r.links.size(); i++) std::cout << r.links[i] << " " << r.link_origin[i] << " " << r.link_hits[i] << "\n";
	std::cout << "#\n";
	std::cout << ts.n_walks << " " << ts.n_steps << " " << ts.n_interior << " " << ts.n_added << " " << ts.n_missing << "\n";
	const kmx_resolve_stats &st = r.stats;
	std::cout << st.n_candidates << " " << st.n_resolved << " " << st.n_crossed << " " << st.n_unsupported << " " << st.n_ambiguous << " " << st.n_copies_added << " " << st.n_unitigs_out << " "
	          << st.reserved << "\n#\n";
	KModel::write_resolved_tsv(std::cout, r);
	std::cout << "#\n";
	const kmx_contig_params cp = {1, 0, 0};
	KModel::write_contigs_fasta(std::cout, km->unitig_contigs(r.strs, &r.rec, r.link_offsets, r.links, r.link_hits, k, cp));
	delete km;
	return 0;
}
