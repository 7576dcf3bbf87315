// Test program for include/kmodel.hpp's read mapping: count the k-mers of a FASTA / FASTQ file on the GPU (init_reads), take the
// unitigs of the kept listing (count_unitigs(thr)), open a map session on them, map the reads of a text file (one per line) and
// write the segment table, a line "#", and the hits table to stdout; the test compares them with the restatement.
// With the single argument "--tsv-only" it needs no device: it formats two hand-made segments and their hits.
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "kmodel.hpp"

int main(int argc, char **argv)
{
	if (sizeof(kmx_map_segment) != 24 || sizeof(kmx_seq_map) != 64) return 3;
	if (argc == 2 && !strcmp(argv[1], "--tsv-only")) {
		std::vector<kmx_map_segment> segs(2);
		memset(&segs[0], 0, 2 * sizeof(kmx_map_segment));
		segs[0].pos = 3; segs[0].n_windows = 5; segs[0].o = 4; segs[0].off = 7;
		segs[1].pos = 12; segs[1].n_windows = 1; segs[1].o = 1; segs[1].off = 0;
		const uint64_t so[] = {0, 1, 1, 2}, off[] = {0, 10, 10, 40};
		KModel::write_paths_tsv(std::cout, segs, std::vector<uint64_t>(so, so + 4), std::vector<uint64_t>(off, off + 4), 100);
		std::vector<uint64_t> hits;
		hits.push_back(1); hits.push_back(0); hits.push_back(5);
		KModel::write_hits_tsv(std::cout, hits);
		return 0;
	}
	if (argc < 5) return 2;
	const int k = atoi(argv[2]);
	const uint32_t thr = (uint32_t)atol(argv[3]);
	std::vector<std::string> reads;
	std::ifstream in(argv[4]);
	for (std::string line; std::getline(in, line);) reads.push_back(line);
	KModel *km = get_model(1, 1023, 3, 2);
	km->init_reads(argv[1], k);
	const std::vector<std::string> strs = km->count_unitigs(thr);
	km->count_unitig_map_begin(strs);
	std::vector<uint64_t> so, hits(strs.size(), 0), off(reads.size() + 1, 0);
	std::vector<kmx_seq_map> rec;
	const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &so, &rec, &hits);
	if (so.size() != reads.size() + 1 || rec.size() != reads.size() || so.back() != segs.size()) return 4;
	if (km->seq_to_unitigs(reads).size() != segs.size()) return 5;   // without the optional outputs
	km->unitig_map_end();
	for (size_t i = 0; i < reads.size(); i++) off[i + 1] = off[i] + reads[i].size();
	KModel::write_paths_tsv(std::cout, segs, so, off);
	std::cout << "#\n";
	KModel::write_hits_tsv(std::cout, hits);
	delete km;
	return 0;
}
