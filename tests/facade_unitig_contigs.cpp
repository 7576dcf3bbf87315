// Test program for include/kmodel.hpp's contigs: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the unitig
// graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the reads of a text file (one per
// line), thread them through the graph (seq_walks at max_gap, max_indel), build the contigs (unitig_contigs at min_reads, ratio)
// and write to stdout, each block closed by a line "#": every field of every contig, the steps, the places, the contig graph, the
// stats, the FASTA text, the paths table, the GFA text without and with the unitig segments.  The test compares them with the
// restatement.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_contig) != 64 || sizeof(kmx_contig_stats) != 64 || sizeof(kmx_contig_params) != 16 || sizeof(kmx_contig_place) != 8) return 3;
	if (argc < 9) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_walk_params par = {(uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]), {0, 0}};
	const kmx_contig_params cp = {(uint64_t)atoll(argv[7]), (uint32_t)atol(argv[8]), 0};
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
	std::vector<uint64_t> so, link_hits(links.size(), 0);
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so);
	km->seq_walks(segs, so, link_offsets, links, par, 0, 0, &link_hits);
	km->unitig_map_end();
	const KModel::Contigs c = km->unitig_contigs(strs, &rec, link_offsets, links, link_hits, k, cp);
	if (c.rec.size() != c.strs.size() || c.steps.size() != strs.size() || c.place.size() != strs.size() || c.link_offsets.size() != 2 * c.strs.size() + 1 || c.links.size() != c.support.size()) return 4;
	if (km->unitig_contigs(strs, 0, link_offsets, links, link_hits, k, cp).steps != c.steps) return 5;   // without the records
	for (size_t i = 0; i < c.rec.size(); i++) {
		const kmx_contig &r = c.rec[i];
		std::cout << r.n_kmers << " " << r.sum_count << " " << r.min_count << " " << r.max_count << " " << r.first_step << " " << r.n_steps << " " << (int)r.circular << " " << (int)r.n_pred << " "
		          << (int)r.n_succ << " " << (int)r.reserved << " " << r.min_support << " " << r.sum_support << " " << r.reserved2 << "\n";
	}
	std::cout << "#\n";
	for (size_t i = 0; i < c.steps.size(); i++) std::cout << c.steps[i] << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < c.place.size(); i++) std::cout << c.place[i].oc << " " << c.place[i].off << "\n";
	std::cout << "#\n";
	for (size_t i = 0; i < c.link_offsets.size(); i++) std::cout << c.link_offsets[i] << "\n";
	for (size_t i = 0; i < c.links.size(); i++) std::cout << c.links[i] << " " << c.support[i] << "\n";
	std::cout << "#\n";
	const kmx_contig_stats &st = c.stats;
	std::cout << st.n_links << " " << st.n_kept << " " << st.n_below_min << " " << st.n_below_ratio << " " << st.n_chain << " " << st.n_contigs << " " << st.n_circular << " " << st.n_multi << "\n#\n";
	KModel::write_contigs_fasta(std::cout, c);
	std::cout << "#\n";
	KModel::write_contig_paths_tsv(std::cout, c);
	std::cout << "#\n";
	KModel::write_contigs_gfa(std::cout, c, k);
	std::cout << "#\n";
	KModel::write_contigs_gfa(std::cout, c, k, &strs, &rec);
	delete km;
	return 0;
}
