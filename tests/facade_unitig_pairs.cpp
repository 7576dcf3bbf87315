// Test program for include/kmodel.hpp's read pairs: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the
// unitig graph of the kept listing (count_unitig_graph(thr)), open a map session on its unitigs, map the interleaved reads of a
// text file (one per line), thread them through the graph (seq_walks), place the pairs (seq_pairs, in two batches cut at a pair
// boundary that merge into one list) and write to stdout, each block closed by a line "#": every field of every pair, the stats
// summed over the two batches, the link table and the histogram.  The test compares them with the restatement.
// With the single argument "--tsv-only" it needs no device: it formats a hand-made list and histogram.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

static void print_pairs(const std::vector<kmx_pair> &pairs, uint64_t base)
{
	for (size_t i = 0; i < pairs.size(); i++) {
		const kmx_pair &p = pairs[i];
		const uint64_t none = ~(uint64_t)0;
		std::cout << (p.walk_a == none ? none : p.walk_a + base) << " " << (p.walk_b == none ? none : p.walk_b + base) << " " << p.cls << " " << p.edge << " " << p.oa << " " << p.xa << " " << p.ob
		          << " " << p.xb << " " << p.d << " " << p.frag << " " << p.reserved << "\n";
	}
}

int main(int argc, char **argv)
{
	if (sizeof(kmx_pair) != 64 || sizeof(kmx_pair_link) != 32 || sizeof(kmx_pair_stats) != 80 || sizeof(kmx_pair_params) != 16) return 3;
	if (argc == 2 && !strcmp(argv[1], "--tsv-only")) {
		const uint64_t lo[] = {0, 2, 2, 7, 8, 8, 8, 8, 8};
		const uint32_t lk[] = {2, 5, 0, 1, 3, 4, 7, 6};
		const kmx_pair_link pl[] = {{0, 5, 3, 100, 10, 60}, {1, 6, 1, 0, 0, 0}, {2, 7, 7, 31, 1, 9}, {2, 4, (uint64_t)1 << 33, ((uint64_t)1 << 35) + 5, 0, 4000000000u}, {3, 6, 2, 5, 2, 3}};
		const uint64_t hist[] = {0, 5, 0, (uint64_t)1 << 40, 1};
		KModel::write_pair_links_tsv(std::cout, std::vector<kmx_pair_link>(pl, pl + 5), std::vector<uint64_t>(lo, lo + 9), std::vector<uint32_t>(lk, lk + 8));
		std::cout << "#\n";
		KModel::write_insert_hist_tsv(std::cout, std::vector<uint64_t>(hist, hist + 5), 25);
		return 0;
	}
	if (argc < 9) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	const kmx_pair_params par = {(uint32_t)atol(argv[5]), (uint32_t)atol(argv[6]), (uint32_t)atol(argv[7]), (uint32_t)atol(argv[8])};
	const kmx_walk_params wpar = {(uint32_t)k, 0, {0, 0}};
	std::vector<std::string> reads;
	std::ifstream in(argv[4]);
	for (std::string line; std::getline(in, line);) reads.push_back(line);
	if (reads.size() % 2) return 2;
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	std::vector<kmx_unitig> rec;
	std::vector<uint64_t> link_offsets;
	std::vector<uint32_t> links;
	const std::vector<std::string> strs = km->count_unitig_graph(thr, &rec, &link_offsets, &links);
	km->count_unitig_map_begin(strs);
	std::vector<kmx_pair_link> plinks;
	std::vector<uint64_t> hist(par.n_bins, 0), pair_hits(links.size(), 0);
	kmx_pair_stats tot = kmx_pair_stats();
	const size_t half = reads.size() / 4 * 2;                       // a pair boundary
	uint64_t base = 0;
	for (int b = 0; b < 2; b++) {
		const std::vector<std::string> part(reads.begin() + (b ? half : 0), b ? reads.end() : reads.begin() + half);
		std::vector<uint64_t> so, wo;
		std::vector<uint32_t> steps;
		kmx_pair_stats st;
		const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(part, &so);
		const std::vector<kmx_walk> walks = km->seq_walks(segs, so, link_offsets, links, wpar, &wo, &steps);
		const std::vector<kmx_pair> pairs = km->seq_pairs(walks, wo, steps, link_offsets, links, par, &plinks, &hist, &pair_hits, &st);
		if (pairs.size() != part.size() / 2 || st.n_pairs != pairs.size()) return 4;
		if (km->seq_pairs(walks, wo, steps, link_offsets, links, par).size() != pairs.size()) return 5;   // without the optional outputs
		print_pairs(pairs, base);
		base += walks.size();
		tot.n_pairs += st.n_pairs; tot.n_none += st.n_none; tot.n_single += st.n_single; tot.n_same += st.n_same; tot.n_negative += st.n_negative;
		tot.n_inverted += st.n_inverted; tot.n_link += st.n_link; tot.n_adjacent += st.n_adjacent; tot.n_far += st.n_far;
	}
	km->unitig_map_end();
	std::cout << "#\n" << tot.n_pairs << " " << tot.n_none << " " << tot.n_single << " " << tot.n_same << " " << tot.n_negative << " " << tot.n_inverted << " " << tot.n_link << " " << tot.n_adjacent
	          << " " << tot.n_far << " " << tot.reserved << "\n#\n";
	KModel::write_pair_links_tsv(std::cout, plinks, link_offsets, links);
	std::cout << "#\n";
	KModel::write_insert_hist_tsv(std::cout, hist, par.bin_width);
	std::cout << "#\n";
	for (size_t i = 0; i < pair_hits.size(); i++) std::cout << pair_hits[i] << "\n";
	delete km;
	return 0;
}
