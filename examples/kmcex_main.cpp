// examples/kmcex_main.cpp -- the reference's driver (main.cpp:64-150) against include/kmodel.hpp + libkmx.so.
//
//   kmcEx [options] <input_file_name> <output_file_name> <working_directory>
//     -k<len> -t<threads> -ci<min> -cs<max> -nh<hashes> -nb<arrays>         (main.cpp:46-51)
//     -g   count the input's k-mers on the GPU (KModel::init_reads) instead of running KMC; no KMC database is written
//     -u<thr>  with -g and an odd k: also write the unitigs of the counted k-mers with count >= thr (1 when omitted) as FASTA to
//          <working_directory>/<basename(output_file_name)>/unitigs.fa (KModel::count_unitigs)
//     -G   with -u: also write the unitig graph (the unitigs and the edges between them) as GFA 1 to unitigs.gfa beside
//          unitigs.fa (KModel::count_unitig_graph)
//     -C<len>  with -u<thr>, thr >= 1: clean the graph first (tips, islands and bubbles of at most len k-mers, 2 k when omitted, at
//          most 16 rounds; KModel::count_unitig_graph_clean): unitigs.fa, and unitigs.gfa with -G, then hold the cleaned graph
//     -M   with -u<thr>: read the input a second time (plain FASTA / FASTQ, not gzip, not @list) and map its reads onto the
//          unitigs written (KModel::count_unitig_map_begin, seq_to_unitigs): reads.paths.tsv (read, start in read, windows,
//          unitig, strand, offset) and unitigs.hits.tsv (unitig, mapped windows) beside unitigs.fa
//     -W<max_gap>  with -M: also thread every read's segments through the graph (KModel::seq_walks; gaps of at most max_gap
//          unmapped windows are bridged, k when omitted, with at most one base lost or gained per bridge): reads.gaf (one line
//          per walk) and unitigs.links.tsv (link index, source, target, reads that cross it).  Implies the graph, as -G does;
//          unitigs.gfa is still written only with -G
//     -X<min_reads>[,<ratio>]  with -M -W: drop the edges that fewer than min_reads reads cross (and, with ratio, those whose reads
//          times ratio stay below the best edge at either end), merge the unitigs along what is left (KModel::unitig_contigs):
//          contigs.fa and contigs.paths.tsv (contig, step, unitig, strand, k-mer offset); with -G also contigs.gfa (unitig and
//          contig segments, the kept edges with their reads, one path line per contig)
//     -R<min_reads>[,<max_cross>]  with -M -W -X: first split every unitig whose reads pair its ways in with its ways out one to one
//          (KModel::unitig_through per batch, then KModel::unitig_resolve: a pairing needs min_reads reads, every other pairing
//          at most max_cross, 0 when omitted), so that repeats shorter than a read no longer end the contigs: contigs.* are built
//          from the resolved graph, unitigs.resolved.tsv (new unitig, origin, copy) names its unitigs; unitigs.fa and unitigs.gfa
//          stay the unresolved graph
//     -P<max_dist>  with -M -W: the input is INTERLEAVED paired reads (reads 2 p and 2 p + 1 are the mates of pair p, forward-reverse);
//          place the two mates of every pair in the graph (KModel::seq_pairs; a mate needs one mapped window, two unitigs are
//          linked at a distance of at most max_dist windows, 1000 when omitted): pairs.insert.tsv (bin start, pairs; bins of 10
//          bases up to 2000) and pairs.links.tsv (a, b, pairs, mean distance, min, max, link index or -).  A batch never splits a
//          pair.  With -X the pairs per edge are added to the reads per edge before the contigs are built
//     -S<min_pairs>[,<ratio>]  with -M -W -P: order and orient along the pair links that at least min_pairs pairs support (and, with
//          ratio, whose pairs times ratio reach the best link at either end) and spell scaffolds with runs of N sized from the
//          insert size (KModel::unitig_scaffold; inner is the floor of the mean d of the pairs on one unitig with frag >= 0, a run
//          has at least 10 N and at most 2 max_dist): scaffolds.fa, scaffolds.paths.tsv (scaffold, step, unitig, strand, base
//          offset, N in front, estimate) and scaffolds.agp (AGP 2.1).  Without -X it scaffolds the unitigs from pairs.links.tsv's
//          list; with -X it reads the input a third time, maps the pairs onto the contigs with the contig graph and scaffolds the
//          contigs ("unitig" in the two tables is then the contig).  Not with -R: a resolved set is no set to map onto
//     -T[<tol>[,<max_steps>]]  with -M -W -P -X -R: after the last batch, find for every pair link the one path of the graph between
//          its two unitigs whose windows fit the insert size within tol (k when omitted) in at most max_steps (8) unitigs
//          (KModel::pair_paths; links of at least -R's min_reads pairs, inner as -S takes it, at most 4096 prefixes per link) and
//          add the pairs of every such path to the reads through its unitigs and across its edges before -R and -X judge them,
//          so that repeats longer than a read and shorter than a fragment no longer end the contigs: pairs.paths.tsv (entry, a,
//          b, pairs, verdict, windows, steps)
//     -F[<kinds>]  with -S: spell the scaffolds again with the graph's own bases in the gaps (KModel::scaffold_fill).  After the
//          scaffolds it finds, for every pair link, the one path through the graph of what was scaffolded (the unitig graph, with
//          -X the contig graph; KModel::pair_paths at -S's min_pairs and inner, tol = k, at most 8 unitigs and 4096 prefixes per
//          link: -T's conventions) and fills the links the bits of kinds ask for (3 when omitted; 1: links with a path, 2: links
//          along one graph edge, whose two strings overlap by k - 1): scaffolds.filled.fa and scaffolds.fill.tsv (scaffold, step,
//          unitig, strand, kind, entry, offset, bytes in front, path).  scaffolds.fa stays as it is
//     -L[<tol>]  with -S: after the last batch, drop from the list that -S scaffolds the links that skip a unitig
//          (KModel::pair_reduce at -S's min_pairs and inner; a link a -> c goes when links a -> b and b -> c explain its distance
//          within tol windows, k when omitted; rows of more than 64 links are not searched: tol = k and 64 are conventions, not
//          measured choices): pairs.reduced.tsv (entry, a, b, pairs, verdict, via, witnesses, g, delta).  The scaffolds, and with -F
//          the pair paths and the fill, are then built from the reduced list.  -T keeps the full list
//     -J   with -X -S: the contigs are scaffolded from the list of the first pass, lifted to contig coordinates through the place of
//          every unitig (KModel::pair_lift at -P's max_dist), instead of reading the input once more and mapping every pair onto
//          the contigs: pairs.lifted.tsv (entry, a, b, pairs, class, A, B, shift, out).  inner is the floor of (the sum of d over
//          the first pass's pairs on one unitig + the lifted d of the forward SAME entries) / (their number + the pairs of those
//          entries): what the second pass would have averaged.  -L and -F work on the lifted list as on a mapped one.  Not with -R
//
// Same flow: run the KMC counter on the FASTQ input (the reference shells out to ./kmc_api/kmc, main.cpp:137-140;
// here the binary is taken from $KMC_BIN or ./kmc_api/kmc and skipped when absent so that an existing KMC
// database at <output_file_name> is used), build the model on the GPU, print the summary, save it under
// <working_directory>/<basename(output_file_name)>.  Unlike the reference, main returns a proper status.
#include "kmodel.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <sys/stat.h>
#include <unistd.h>

struct Params {
	int k = 31, num_hash = 7, num_bit = 5, ci = 1, cs = 1023, t = 4;
	bool gpu_count = false, gfa = false, map = false;
	long unitig_thr = -1;                                          // -u: the threshold, -1 = no unitigs
	long clean_len = -1;                                           // -C: the cap of tips and bubbles in k-mers, 0 = 2 k, -1 = no cleaning
	long walk_gap = -2;                                            // -W: max_gap, -1 = k, -2 = no walks
	long long min_reads = -1;                                      // -X: min_reads, -1 = no contigs
	long ratio = 0;                                                // -X<min_reads>,<ratio>
	long long res_min = -1, res_cross = 0;                         // -R<min_reads>[,<max_cross>], -1 = no resolution
	long pair_dist = -2;                                           // -P: max_dist, -1 = 1000, -2 = no pairs
	long long scaf_min = -1;                                       // -S: min_pairs, -1 = no scaffolds
	long scaf_ratio = 0;                                           // -S<min_pairs>,<ratio>
	long path_tol = -2, path_steps = 8;                            // -T[<tol>[,<max_steps>]]: tol, -1 = k, -2 = no pair paths
	long fill_kinds = -1;                                          // -F[<kinds>]: the links to fill, -1 = no filled scaffolds
	long reduce_tol = -2;                                          // -L[<tol>]: tol, -1 = k, -2 = the list is scaffolded as it is
	bool lift = false;                                             // -J: the contigs' pair list is lifted from the unitigs', not mapped again
	std::string input, output, workdir = "/tmp";
};

static bool parse(int argc, char **argv, Params &p)
{
	if (argc < 4) return false;
	int i = 1;
	for (; i < argc && argv[i][0] == '-'; ++i) {
		const char *a = argv[i];
		if (!strncmp(a, "-nh", 3)) p.num_hash = atoi(a + 3);
		else if (!strncmp(a, "-nb", 3)) p.num_bit = atoi(a + 3);
		else if (!strncmp(a, "-ci", 3)) p.ci = atoi(a + 3);
		else if (!strncmp(a, "-cs", 3)) p.cs = atoi(a + 3);
		else if (!strncmp(a, "-t", 2)) p.t = atoi(a + 2);
		else if (!strncmp(a, "-k", 2)) p.k = atoi(a + 2);
		else if (!strcmp(a, "-g")) p.gpu_count = true;
		else if (!strcmp(a, "-G")) p.gfa = true;
		else if (!strcmp(a, "-M")) p.map = true;
		else if (!strncmp(a, "-W", 2)) {
			char *end = nullptr;
			p.walk_gap = a[2] ? strtol(a + 2, &end, 10) : -1;
			if (a[2] && (*end || p.walk_gap < 0 || p.walk_gap > 0xFFFFFFFFL)) return false;   // not a number of windows
		}
		else if (!strncmp(a, "-X", 2)) {
			char *end = nullptr;
			if (!a[2]) return false;
			p.min_reads = strtoll(a + 2, &end, 10);
			if (end == a + 2 || p.min_reads < 0) return false;
			if (*end == ',') {
				const char *r = end + 1;
				p.ratio = strtol(r, &end, 10);
				if (end == r || p.ratio < 0 || p.ratio > 65536) return false;
			}
			if (*end) return false;
		}
		else if (!strncmp(a, "-R", 2)) {
			char *end = nullptr;
			if (!a[2]) return false;
			p.res_min = strtoll(a + 2, &end, 10);
			if (end == a + 2 || p.res_min < 0) return false;
			if (*end == ',') {
				const char *r = end + 1;
				p.res_cross = strtoll(r, &end, 10);
				if (end == r || p.res_cross < 0) return false;
			}
			if (*end) return false;
		}
		else if (!strncmp(a, "-S", 2)) {
			char *end = nullptr;
			if (!a[2]) return false;
			p.scaf_min = strtoll(a + 2, &end, 10);
			if (end == a + 2 || p.scaf_min < 0) return false;
			if (*end == ',') {
				const char *r = end + 1;
				p.scaf_ratio = strtol(r, &end, 10);
				if (end == r || p.scaf_ratio < 0 || p.scaf_ratio > 65536) return false;
			}
			if (*end) return false;
		}
		else if (!strncmp(a, "-T", 2)) {
			char *end = nullptr;
			p.path_tol = -1;
			if (a[2]) {
				p.path_tol = strtol(a + 2, &end, 10);
				if (end == a + 2 || p.path_tol < 0 || p.path_tol > 0xFFFFFFFFL) return false;   // not a number of windows
				if (*end == ',') {
					const char *r = end + 1;
					p.path_steps = strtol(r, &end, 10);
					if (end == r || p.path_steps < 1 || p.path_steps > KMX_PATH_MAX_STEPS) return false;
				}
				if (*end) return false;
			}
		}
		else if (!strncmp(a, "-F", 2)) {
			char *end = nullptr;
			p.fill_kinds = a[2] ? strtol(a + 2, &end, 10) : 3;
			if (a[2] && (*end || p.fill_kinds < 0 || p.fill_kinds > 3)) return false;   // not a set of kinds
		}
		else if (!strncmp(a, "-L", 2)) {
			char *end = nullptr;
			p.reduce_tol = a[2] ? strtol(a + 2, &end, 10) : -1;
			if (a[2] && (*end || p.reduce_tol < 0 || p.reduce_tol > 0xFFFFFFFFL)) return false;   // not a number of windows
		}
		else if (!strcmp(a, "-J")) p.lift = true;
		else if (!strncmp(a, "-P", 2)) {
			char *end = nullptr;
			p.pair_dist = a[2] ? strtol(a + 2, &end, 10) : -1;
			if (a[2] && (*end || p.pair_dist < 0 || p.pair_dist > 0xFFFFFFFFL)) return false;   // not a number of windows
		}
		else if (!strncmp(a, "-C", 2)) {
			char *end = nullptr;
			p.clean_len = a[2] ? strtol(a + 2, &end, 10) : 0;
			if (a[2] && (*end || p.clean_len < 1 || p.clean_len > 0xFFFFFFFFL)) return false;   // not a length
		}
		else if (!strncmp(a, "-u", 2)) {
			char *end = nullptr;
			p.unitig_thr = a[2] ? strtol(a + 2, &end, 10) : 1;
			if (a[2] && (*end || p.unitig_thr < 0 || p.unitig_thr > 0xFFFFFFFFL)) return false;   // not a count
		}
	}
	if (argc - i < 3) return false;
	p.input = argv[argc - 3];
	p.output = argv[argc - 2];
	p.workdir = argv[argc - 1];
	if (p.unitig_thr >= 0 && (!p.gpu_count || !(p.k & 1))) return false;   // the unitigs come from the listing -g keeps; the rule needs an odd k
	if (p.gfa && p.unitig_thr < 0) return false;                   // the graph is the unitigs' own
	if (p.clean_len >= 0 && p.unitig_thr < 1) return false;        // cleaning removes nodes by "count below thr"
	if (p.map && p.unitig_thr < 0) return false;                   // the reads are mapped onto the unitigs written
	if (p.walk_gap > -2 && !p.map) return false;                   // the walks are built from the map's segments
	if (p.min_reads >= 0 && (!p.map || p.walk_gap == -2)) {        // the contigs are built from the reads per link, which the walks count
		std::cout << "-X needs -M -W: the contigs are built from the reads that cross every link, which the walks count\n";
		return false;
	}
	if (p.res_min >= 0 && p.min_reads < 0) {                       // the resolved graph is what the contigs are built from
		std::cout << "-R needs -M -W -X: the repeats are resolved from the walks, and the contigs are built from the resolved graph\n";
		return false;
	}
	if (p.pair_dist > -2 && (!p.map || p.walk_gap == -2)) {        // the pairs are placed by their walks
		std::cout << "-P needs -M -W: the mates of a pair are placed by their walks\n";
		return false;
	}
	if (p.scaf_min >= 0 && p.pair_dist == -2) {                    // the scaffolds are built from the pair links
		std::cout << "-S needs -M -W -P: the scaffolds are built from the links the pairs leave\n";
		return false;
	}
	if (p.scaf_min >= 0 && p.res_min >= 0) {
		std::cout << "-S does not go with -R: the pairs are mapped onto what is scaffolded, and a resolved set, where a k-mer lies on several copies, is no set to map onto\n";
		return false;
	}
	if (p.path_tol > -2 && (p.pair_dist == -2 || p.res_min < 0)) {  // the paths are found for the pair links and credited to what -R reads
		std::cout << "-T needs -M -W -P -X -R: the paths are found for the links the pairs leave, and their pairs are added to what the repeats are resolved from\n";
		return false;
	}
	if (p.fill_kinds >= 0 && p.scaf_min < 0) {                     // the filled scaffolds are the scaffolds spelled again
		std::cout << "-F needs -S: it fills the gaps of the scaffolds\n";
		return false;
	}
	if (p.reduce_tol > -2 && p.scaf_min < 0) {                     // the reduced list is the one the scaffolds are built from
		std::cout << "-L needs -S: it reduces the list of pair links the scaffolds are built from\n";
		return false;
	}
	if (p.lift && (p.scaf_min < 0 || p.min_reads < 0)) {           // the lifted list is the one the contigs are scaffolded from
		std::cout << "-J needs -X -S: it lifts the list of pair links to the contigs that are scaffolded\n";
		return false;
	}
	if (p.lift && p.res_min >= 0) {
		std::cout << "-J does not go with -R: a resolved set, where a unitig lies on several copies, has no place to lift through\n";
		return false;
	}
	return !p.input.empty() && !p.output.empty() && !p.workdir.empty();
}

// the next reads of a plain FASTA (records may span lines) or FASTQ (four lines each) stream, up to about max_bases of them
static bool next_reads(std::istream &in, std::vector<std::string> &reads, size_t max_bases)
{
	reads.clear();
	size_t bases = 0;
	std::string line, seq;
	while (bases < max_bases && in.peek() != EOF) {
		if (!std::getline(in, line)) break;
		if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
		if (line.empty()) continue;
		if (line[0] == '@') {
			if (!std::getline(in, seq)) return false;
			if (!seq.empty() && seq[seq.size() - 1] == '\r') seq.erase(seq.size() - 1);
			if (!std::getline(in, line) || line.empty() || line[0] != '+' || !std::getline(in, line)) return false;
		} else if (line[0] == '>') {
			seq.clear();
			while (in.peek() != EOF && in.peek() != '>') {
				if (!std::getline(in, line)) break;
				if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
				seq += line;
			}
		} else
			return false;
		bases += seq.size();
		reads.push_back(seq);
	}
	return true;
}

// the typical d of a pair on one unitig: the floor of the mean over the SAME pairs with frag >= 0 (0 when there is none)
struct InnerSum {
	long double sum = 0;
	uint64_t n = 0;
	void add(const std::vector<kmx_pair> &pr)
	{
		for (size_t i = 0; i < pr.size(); i++)
			if (pr[i].cls == KMX_PAIR_SAME && pr[i].frag >= 0) { sum += (long double)pr[i].d; n++; }
	}
	uint32_t inner() const
	{
		if (!n || sum <= 0) return 0;
		const long double q = sum / (long double)n;
		return q >= 4294967295.0L ? 0xFFFFFFFFu : (uint32_t)q;
	}
};

// -S: the scaffolds of `strs` from `plinks`, written as scaffolds.fa, scaffolds.paths.tsv and scaffolds.agp; with -F also the
// scaffolds filled along the paths of the graph (link_offsets, links) of `strs`: scaffolds.filled.fa and scaffolds.fill.tsv
static bool write_scaffolds(KModel *km, const std::string &dir, const std::vector<std::string> &strs, const std::vector<kmx_unitig> *rec, const std::vector<kmx_pair_link> &full, const Params &p,
                            uint32_t inner, uint32_t max_dist, const char *what, const std::vector<uint64_t> &link_offsets, const std::vector<uint32_t> &links)
{
	KModel::PairReduced red;
	if (p.reduce_tol > -2) {                                       // -L: the links that skip a unitig go first
		const kmx_pair_reduce_params rp = {(uint64_t)p.scaf_min, inner, p.reduce_tol < 0 ? (uint32_t)p.k : (uint32_t)p.reduce_tol, 64, 0};
		red = km->pair_reduce(strs, full, p.k, rp);
		std::ofstream rt((dir + "/pairs.reduced.tsv").c_str());
		KModel::write_pair_reduce_tsv(rt, full, red);
		rt.close();
		if (!rt) { std::cout << "could not write " << dir << "/pairs.reduced.tsv" << std::endl; return false; }
		std::cout << "   pair links of " << what << " reduced (tol " << rp.tol << ", rows of <= " << rp.max_row << ", inner " << inner << ") :     " << red.stats.n_transitive << " of " << red.stats.n_entries
		          << " links skip a unitig (" << red.stats.n_kept << " kept, " << red.stats.n_complex << " complex, " << red.stats.n_below_min << " below " << p.scaf_min << " pairs, " << red.stats.n_ignored
		          << " ignored), " << red.stats.n_out << " links stay" << std::endl;
	}
	const std::vector<kmx_pair_link> &plinks = p.reduce_tol > -2 ? red.list : full;
	const uint64_t max_n = 2 * (uint64_t)max_dist;
	const kmx_scaffold_params sp = {(uint64_t)p.scaf_min, (uint32_t)p.scaf_ratio, inner, max_n < 10 ? (uint32_t)max_n : 10u, max_n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)max_n, 0};
	const KModel::Scaffolds sc = km->unitig_scaffold(strs, rec, plinks, p.k, sp);
	std::ofstream sf((dir + "/scaffolds.fa").c_str()), st((dir + "/scaffolds.paths.tsv").c_str()), sa((dir + "/scaffolds.agp").c_str());
	KModel::write_scaffolds_fasta(sf, sc);
	KModel::write_scaffold_paths_tsv(st, sc);
	KModel::write_scaffolds_agp(sa, sc, strs);
	sf.close();
	st.close();
	sa.close();
	if (!sf || !st || !sa) { std::cout << "could not write " << dir << "/scaffolds.fa, scaffolds.paths.tsv or scaffolds.agp" << std::endl; return false; }
	uint64_t gaps = 0;
	for (size_t i = 0; i < sc.rec.size(); i++) gaps += sc.rec[i].n_gap_bases;
	std::cout << "   scaffolds of " << what << " (links of >= " << p.scaf_min << " pairs" << (p.scaf_ratio ? ", ratio " : "") << (p.scaf_ratio ? std::to_string(p.scaf_ratio) : std::string()) << ", inner " << inner
	          << ") :     " << sc.stats.n_scaffolds << " scaffolds (" << sc.stats.n_multi << " of several, " << sc.stats.n_circular << " circular), " << sc.stats.n_chain << " of " << sc.stats.n_links
	          << " links joined, " << gaps << " N" << std::endl;
	if (p.fill_kinds < 0) return true;
	const kmx_pair_path_params tp = {(uint64_t)p.scaf_min, inner, (uint32_t)p.k, 8, 4096, 0};
	const kmx_fill_params fp = {(uint32_t)p.fill_kinds, 0};
	const KModel::PairPaths pa = km->pair_paths(strs, link_offsets, links, plinks, p.k, tp);
	const KModel::FilledScaffolds fs = km->scaffold_fill(strs, sc, plinks, pa, p.k, fp);
	std::ofstream ff((dir + "/scaffolds.filled.fa").c_str()), ft((dir + "/scaffolds.fill.tsv").c_str());
	KModel::write_filled_scaffolds_fasta(ff, fs);
	KModel::write_scaffold_fill_tsv(ft, fs);
	ff.close();
	ft.close();
	if (!ff || !ft) { std::cout << "could not write " << dir << "/scaffolds.filled.fa or scaffolds.fill.tsv" << std::endl; return false; }
	std::cout << "   filled scaffolds of " << what << " (kinds " << p.fill_kinds << ", tol " << tp.tol << ") :     " << fs.stats.n_path << " links filled along a path, " << fs.stats.n_adjacent << " along an edge, "
	          << fs.stats.n_n << " left as N (" << fs.stats.n_no_entry << " without an entry), " << fs.stats.n_removed << " N removed, " << fs.stats.n_filled << " bases filled" << std::endl;
	return true;
}

int main(int argc, char **argv)
{
	Params p;
	if (!parse(argc, argv, p)) {
		std::cout << "kmcEx (MI355X): counted k-mer encoding & decoding\n"
		             "USAGE  kmcEx [options] <input_file_name|@list> <output_file_name> <working_directory>\n"
		             "       -k<len> (31) -t<threads> (4) -ci<min count> (1) -cs<max count> (1023) -nh<hashes> (7) -nb<arrays> (5)\n"
		             "       -g  count the k-mers of the FASTQ / FASTA input on the GPU instead of running KMC\n"
		             "       -u<thr>  with -g and an odd k: write the unitigs of the k-mers with count >= thr (1) to <saved model>/unitigs.fa\n"
		             "       -G  with -u<thr>: also write the unitigs and the edges between them as GFA 1 to <saved model>/unitigs.gfa\n"
		             "       -C<len>  with -u<thr>, thr >= 1: clip tips, pop bubbles and drop islands of at most len k-mers (2 k) first\n"
		             "       -M  with -u<thr>: map the reads of the (plain FASTA / FASTQ) input onto the unitigs: reads.paths.tsv, unitigs.hits.tsv\n"
		             "       -W<max_gap>  with -M: join every read's segments into walks through the graph, bridging at most max_gap (k) unmapped windows:\n"
		             "           reads.gaf, unitigs.links.tsv (link index, source, target, reads)\n"
		             "       -X<min_reads>[,<ratio>]  with -M -W: merge the unitigs along the edges at least min_reads reads cross: contigs.fa,\n"
		             "           contigs.paths.tsv (contig, step, unitig, strand, offset), and contigs.gfa with -G\n"
		             "       -R<min_reads>[,<max_cross>]  with -M -W -X: first resolve the repeats that reads span: unitigs.resolved.tsv (new unitig,\n"
		             "           origin, copy); contigs.* are built from the resolved graph\n"
		             "       -P<max_dist>  with -M -W: the input is interleaved paired reads (forward-reverse); place the mates of every pair:\n"
		             "           pairs.insert.tsv (insert sizes), pairs.links.tsv (unitigs linked at up to max_dist (1000) windows); with -X the\n"
		             "           pairs per edge count as reads\n"
		             "       -S<min_pairs>[,<ratio>]  with -M -W -P, not with -R: join the unitigs (with -X: the contigs, from a second mapping of the\n"
		             "           pairs onto them) along the links at least min_pairs pairs support, with runs of N sized from the insert size:\n"
		             "           scaffolds.fa, scaffolds.paths.tsv (scaffold, step, unitig, strand, offset, N in front, estimate), scaffolds.agp\n"
		             "       -T[<tol>[,<max_steps>]]  with -M -W -P -X -R: find the one graph path every pair link stands for (windows within tol (k) of\n"
		             "           the insert size, at most max_steps (8) unitigs) and count its pairs as reads through its unitigs: pairs.paths.tsv\n"
		             "       -F[<kinds>]  with -S: fill the scaffolds' gaps with the bases of the one graph path that fits (kinds & 1) and trim the overlap\n"
		             "           of two steps along one edge (kinds & 2; 3 when omitted): scaffolds.filled.fa, scaffolds.fill.tsv (scaffold, step,\n"
		             "           unitig, strand, kind, entry, offset, bytes in front, path)\n"
		             "       -L[<tol>]  with -S: first drop the pair links that skip a unitig (a -> c where a -> b and b -> c explain its distance within tol\n"
		             "           (k) windows; rows of more than 64 links are not searched; both are conventions, not measured choices):\n"
		             "           pairs.reduced.tsv (entry, a, b, pairs, verdict, via, witnesses, g, delta); -S and -F then work on the reduced list\n"
		             "       -J   with -X -S: scaffold the contigs from the first pass's pair list lifted to contig coordinates, instead of reading the\n"
		             "           input once more: pairs.lifted.tsv (entry, a, b, pairs, class, A, B, shift, out); not with -R\n";
		return 2;
	}
	const char *env = getenv("KMC_BIN");
	std::string kmc = env ? env : "./kmc_api/kmc";
	if (p.gpu_count) {
		std::cout << "counting the k-mers of " << p.input << " on the GPU" << std::endl;
	} else if (access(kmc.c_str(), X_OK) == 0) {
		char cmd[4096];
		snprintf(cmd, sizeof cmd, "%s -k%d -t%d -ci%d -cs%d %s %s %s", kmc.c_str(), p.k, p.t, p.ci, p.cs, p.input.c_str(), p.output.c_str(), p.workdir.c_str());
		std::cout << cmd << std::endl;
		if (system(cmd) != 0) { std::cout << "the KMC counter failed" << std::endl; return 1; }
	} else {
		std::cout << "no KMC binary (" << kmc << "): using the existing database " << p.output << std::endl;
	}
	KModel *km = get_model(p.ci, p.cs, p.num_hash, p.num_bit);
	if (p.gpu_count) km->init_reads(p.input, p.k);
	else km->init(p.output);
	km->show_header_info();
	km->show_kmodel_info();
	const size_t slash = p.output.find_last_of('/');
	const std::string dir = p.workdir + "/" + (slash == std::string::npos ? p.output : p.output.substr(slash + 1));
	mkdir(dir.c_str(), 0777);
	km->save(dir);
	if (p.unitig_thr >= 0) {
		std::vector<kmx_unitig> rec;
		std::vector<uint64_t> link_offsets;
		std::vector<uint32_t> links;
		kmx_clean_stats cs;
		const bool walks = p.walk_gap > -2;
		const uint32_t cap = (uint32_t)(p.clean_len > 0 ? p.clean_len : 2 * p.k);
		const kmx_clean_params cp = {KMX_CLEAN_TIPS | KMX_CLEAN_ISLANDS | KMX_CLEAN_BUBBLES, cap, cap, 16};
		const std::vector<std::string> strs = p.clean_len >= 0 ? km->count_unitig_graph_clean((uint32_t)p.unitig_thr, cp, &rec, &link_offsets, &links, &cs)
		                                      : p.gfa || walks ? km->count_unitig_graph((uint32_t)p.unitig_thr, &rec, &link_offsets, &links)
		                                                       : km->count_unitigs((uint32_t)p.unitig_thr, &rec);
		if (p.clean_len >= 0)
			std::cout << "   cleaning (at most " << cap << " k-mers)        :     " << cs.rounds_run << " rounds" << (cs.converged ? "" : " (not converged)") << ", " << cs.n_tips << " tips, "
			          << cs.n_islands << " islands, " << cs.n_bubbles << " bubbles, " << cs.n_kmers_removed << " k-mers removed; " << cs.n_unitigs_before << " unitigs before" << std::endl;
		std::ofstream fa((dir + "/unitigs.fa").c_str());
		KModel::write_unitigs_fasta(fa, strs, rec);
		fa.close();
		if (!fa) { std::cout << "could not write " << dir << "/unitigs.fa" << std::endl; return 1; }
		std::cout << "   unitigs (count >= " << p.unitig_thr << ")              :     " << strs.size() << std::endl;
		if (p.gfa) {
			std::ofstream gf((dir + "/unitigs.gfa").c_str());
			KModel::write_unitigs_gfa(gf, strs, rec, link_offsets, links, p.k);
			gf.close();
			if (!gf) { std::cout << "could not write " << dir << "/unitigs.gfa" << std::endl; return 1; }
			std::cout << "   edges between unitigs                :     " << links.size() << std::endl;
		}
		if (p.map) {
			std::ifstream in(p.input.c_str());
			const int c0 = in.peek();
			if (!in || p.input[0] == '@' || (c0 != '>' && c0 != '@')) { std::cout << "-M reads a plain FASTA / FASTQ file, which " << p.input << " is not" << std::endl; return 1; }
			std::ofstream paths((dir + "/reads.paths.tsv").c_str());
			std::ofstream gaf;
			if (walks) gaf.open((dir + "/reads.gaf").c_str());
			const kmx_walk_params wp = {(uint32_t)(p.walk_gap >= 0 ? p.walk_gap : p.k), 1, {0, 0}};
			std::vector<uint64_t> link_hits(links.size(), 0), walk_offsets, through;
			std::vector<uint32_t> steps;
			kmx_walk_stats wt = kmx_walk_stats();
			std::vector<uint64_t> hits(strs.size(), 0), seg_offsets;
			std::vector<std::string> reads;
			uint64_t n_reads = 0, n_segs = 0, n_win = 0, n_mapped = 0;
			const bool pairs = p.pair_dist > -2;
			const kmx_pair_params pp = {1, (uint32_t)(p.pair_dist >= 0 ? p.pair_dist : 1000), 10, 200};
			std::vector<kmx_pair_link> plinks;
			std::vector<uint64_t> insert_hist(pairs ? pp.n_bins : 0, 0), pair_hits(pairs ? links.size() : 0, 0);
			std::vector<int64_t> frags;
			InnerSum inner;
			kmx_pair_stats pt = kmx_pair_stats();
			std::string carry;                                           // with -P: the first mate of a pair the last batch ended inside
			bool carried = false;
			km->count_unitig_map_begin(strs);
			for (bool ok = true; in.peek() != EOF;) {
				ok = next_reads(in, reads, size_t(1) << 26);
				if (!ok) { std::cout << p.input << " is no FASTA / FASTQ file at read " << n_reads + reads.size() << std::endl; return 1; }
				if (carried) { reads.insert(reads.begin(), carry); carried = false; }
				if (pairs && reads.size() % 2) {
					if (in.peek() == EOF) { std::cout << "-P reads interleaved pairs, and " << p.input << " holds an odd number of reads" << std::endl; return 1; }
					carry = reads.back();
					reads.pop_back();
					carried = true;
					if (reads.empty()) continue;
				}
				std::vector<kmx_seq_map> rec_m;
				const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &seg_offsets, &rec_m, &hits);
				std::vector<uint64_t> off(reads.size() + 1, 0);
				for (size_t i = 0; i < reads.size(); i++) { off[i + 1] = off[i] + reads[i].size(); n_win += rec_m[i].n_windows; n_mapped += rec_m[i].n_mapped; }
				KModel::write_paths_tsv(paths, segs, seg_offsets, off, n_reads);
				if (walks) {
					kmx_walk_stats ws;
					const std::vector<kmx_walk> wk = km->seq_walks(segs, seg_offsets, link_offsets, links, wp, &walk_offsets, &steps, &link_hits, &ws);
					KModel::write_walks_gaf(gaf, wk, walk_offsets, steps, off, strs, p.k, n_reads);
					if (p.res_min >= 0) km->unitig_through(wk, steps, link_offsets, links, through);
					if (pairs) {
						kmx_pair_stats ps;
						const std::vector<kmx_pair> pr = km->seq_pairs(wk, walk_offsets, steps, link_offsets, links, pp, &plinks, &insert_hist, &pair_hits, &ps);
						for (size_t i = 0; i < pr.size(); i++)
							if (pr[i].cls == KMX_PAIR_SAME && pr[i].frag >= 0) frags.push_back(pr[i].frag);
						inner.add(pr);
						pt.n_pairs += ps.n_pairs; pt.n_none += ps.n_none; pt.n_single += ps.n_single; pt.n_same += ps.n_same; pt.n_negative += ps.n_negative;
						pt.n_inverted += ps.n_inverted; pt.n_link += ps.n_link; pt.n_adjacent += ps.n_adjacent; pt.n_far += ps.n_far;
					}
					wt.n_walks += ws.n_walks; wt.n_steps += ws.n_steps; wt.n_edge += ws.n_edge; wt.n_inside += ws.n_inside; wt.n_across += ws.n_across;
					wt.n_unlinked += ws.n_unlinked; wt.n_breaks += ws.n_breaks;
				}
				n_reads += reads.size();
				n_segs += segs.size();
			}
			km->unitig_map_end();
			paths.close();
			std::ofstream ht((dir + "/unitigs.hits.tsv").c_str());
			KModel::write_hits_tsv(ht, hits);
			ht.close();
			if (!paths || !ht) { std::cout << "could not write " << dir << "/reads.paths.tsv or unitigs.hits.tsv" << std::endl; return 1; }
			std::cout << "   reads mapped onto the unitigs        :     " << n_reads << " reads, " << n_segs << " segments, " << n_mapped << " of " << n_win << " windows" << std::endl;
			if (walks) {
				gaf.close();
				std::ofstream lt((dir + "/unitigs.links.tsv").c_str());
				KModel::write_link_hits_tsv(lt, link_offsets, links, link_hits);
				lt.close();
				if (!gaf || !lt) { std::cout << "could not write " << dir << "/reads.gaf or unitigs.links.tsv" << std::endl; return 1; }
				std::cout << "   walks (gaps of at most " << wp.max_gap << " windows)    :     " << wt.n_walks << " walks, " << wt.n_steps << " steps, " << wt.n_edge << " edges crossed, " << wt.n_inside + wt.n_across
				          << " gaps bridged (" << wt.n_across << " across an edge), " << wt.n_breaks << " breaks" << std::endl;
				if (pairs) {
					std::ofstream pl((dir + "/pairs.links.tsv").c_str()), pi((dir + "/pairs.insert.tsv").c_str());
					KModel::write_pair_links_tsv(pl, plinks, link_offsets, links);
					KModel::write_insert_hist_tsv(pi, insert_hist, pp.bin_width);
					pl.close();
					pi.close();
					if (!pl || !pi) { std::cout << "could not write " << dir << "/pairs.links.tsv or pairs.insert.tsv" << std::endl; return 1; }
					if (!frags.empty()) std::nth_element(frags.begin(), frags.begin() + frags.size() / 2, frags.end());
					std::cout << "   pairs (links of at most " << pp.max_dist << " windows)  :     " << pt.n_pairs << " pairs: " << pt.n_same << " on one unitig (" << pt.n_negative << " negative, median fragment "
					          << (frags.empty() ? 0 : frags[frags.size() / 2]) << "), " << pt.n_link << " links (" << pt.n_adjacent << " adjacent, " << plinks.size() << " distinct), " << pt.n_far << " far, "
					          << pt.n_inverted << " inverted, " << pt.n_single << " single, " << pt.n_none << " unplaced" << std::endl;
					for (size_t e = 0; e < link_hits.size() && e < pair_hits.size(); e++) link_hits[e] += pair_hits[e];   // what -X and -R judge the edges by
				}
				if (p.path_tol > -2) {                                      // the pairs that span a repeat, credited along the one path that fits
					const kmx_pair_path_params tp = {(uint64_t)p.res_min, inner.inner(), (uint32_t)(p.path_tol >= 0 ? p.path_tol : p.k), (uint32_t)p.path_steps, 4096, 0};
					const KModel::PairPaths pa = km->pair_paths(strs, link_offsets, links, plinks, p.k, tp, &through, &link_hits);
					std::ofstream pf((dir + "/pairs.paths.tsv").c_str());
					KModel::write_pair_paths_tsv(pf, plinks, pa);
					pf.close();
					if (!pf) { std::cout << "could not write " << dir << "/pairs.paths.tsv" << std::endl; return 1; }
					std::cout << "   pair paths (tol " << tp.tol << ", <= " << tp.max_steps << " steps, inner " << tp.inner << ") :     " << pa.stats.n_path << " of " << pa.stats.n_entries << " links are one path ("
					          << pa.stats.n_adjacent << " adjacent, " << pa.stats.n_no_path << " none, " << pa.stats.n_ambiguous << " ambiguous, " << pa.stats.n_complex << " complex, " << pa.stats.n_below_min
					          << " below " << tp.min_pairs << " pairs, " << pa.stats.n_ignored << " ignored), " << pa.stats.n_added << " unitigs credited" << std::endl;
				}
				if (p.scaf_min >= 0 && p.min_reads < 0 && !write_scaffolds(km, dir, strs, &rec, plinks, p, inner.inner(), pp.max_dist, "unitigs", link_offsets, links)) return 1;
				if (p.min_reads >= 0) {
					const kmx_contig_params xp = {(uint64_t)p.min_reads, (uint32_t)p.ratio, 0};
					KModel::Resolved rs;
					if (p.res_min >= 0) {
						const kmx_resolve_params rp = {(uint64_t)p.res_min, (uint64_t)p.res_cross};
						if (through.empty()) through.assign(16 * strs.size(), 0);
						rs = km->unitig_resolve(strs, &rec, link_offsets, links, &link_hits, through, p.k, rp);
						std::ofstream rt((dir + "/unitigs.resolved.tsv").c_str());
						KModel::write_resolved_tsv(rt, rs);
						rt.close();
						if (!rt) { std::cout << "could not write " << dir << "/unitigs.resolved.tsv" << std::endl; return 1; }
						std::cout << "   repeats resolved (>= " << p.res_min << " reads, <= " << p.res_cross << " across) :     " << rs.stats.n_resolved << " of " << rs.stats.n_candidates << " candidates ("
						          << rs.stats.n_crossed << " crossed, " << rs.stats.n_unsupported << " unsupported, " << rs.stats.n_ambiguous << " ambiguous), " << rs.stats.n_unitigs_out << " unitigs"
						          << std::endl;
						if (links.empty()) rs.link_hits.clear();
					}
					const std::vector<std::string> &cstrs = p.res_min >= 0 ? rs.strs : strs;
					const std::vector<kmx_unitig> &crec = p.res_min >= 0 ? rs.rec : rec;
					const KModel::Contigs ct = p.res_min >= 0 ? km->unitig_contigs(rs.strs, &rs.rec, rs.link_offsets, rs.links, rs.link_hits, p.k, xp)
					                                          : km->unitig_contigs(strs, &rec, link_offsets, links, link_hits, p.k, xp);
					std::ofstream cf((dir + "/contigs.fa").c_str()), cp2((dir + "/contigs.paths.tsv").c_str());
					KModel::write_contigs_fasta(cf, ct);
					KModel::write_contig_paths_tsv(cp2, ct);
					cf.close();
					cp2.close();
					if (!cf || !cp2) { std::cout << "could not write " << dir << "/contigs.fa or contigs.paths.tsv" << std::endl; return 1; }
					if (p.gfa) {
						std::ofstream cg((dir + "/contigs.gfa").c_str());
						KModel::write_contigs_gfa(cg, ct, p.k, &cstrs, &crec);
						cg.close();
						if (!cg) { std::cout << "could not write " << dir << "/contigs.gfa" << std::endl; return 1; }
					}
					if (p.scaf_min >= 0 && p.lift) {                         // -J: the first pass's list in contig coordinates
						const kmx_pair_lift_params lp = {pp.max_dist, 0};
						const KModel::PairLifted lf = km->pair_lift(strs, ct.place, ct.rec, plinks, p.k, lp);
						std::ofstream lt2((dir + "/pairs.lifted.tsv").c_str());
						KModel::write_pair_lift_tsv(lt2, plinks, lf);
						lt2.close();
						if (!lt2) { std::cout << "could not write " << dir << "/pairs.lifted.tsv" << std::endl; return 1; }
						InnerSum linner = inner;                             // what the pairs on one contig would have averaged
						linner.sum += (long double)lf.stats.sum_same_d;
						linner.n += lf.stats.pairs_same - lf.stats.pairs_same_back;
						std::cout << "   pair links lifted to the contigs (at most " << lp.max_dist << " windows) :     " << lf.stats.n_link << " of " << lf.stats.n_entries << " links lie between contigs ("
						          << lf.stats.n_same << " on one contig, " << lf.stats.n_same_back << " of them backward, " << lf.stats.n_inverted << " inverted, " << lf.stats.n_far << " far, "
						          << lf.stats.n_ignored << " ignored), " << lf.stats.n_out << " distinct" << std::endl;
						if (!write_scaffolds(km, dir, ct.strs, 0, lf.list, p, linner.inner(), pp.max_dist, "contigs", ct.link_offsets, ct.links)) return 1;
					}
					else if (p.scaf_min >= 0) {                              // the pairs once more, on the contigs and their graph
						std::ifstream in2(p.input.c_str());
						std::vector<kmx_pair_link> cplinks;
						InnerSum cinner;
						carried = false;
						km->count_unitig_map_begin(ct.strs);
						while (in2.peek() != EOF) {
							if (!next_reads(in2, reads, size_t(1) << 26)) { std::cout << p.input << " is no FASTA / FASTQ file" << std::endl; return 1; }
							if (carried) { reads.insert(reads.begin(), carry); carried = false; }
							if (reads.size() % 2) {
								if (in2.peek() == EOF) break;                     // (the first pass has refused an odd number of reads)
								carry = reads.back();
								reads.pop_back();
								carried = true;
								if (reads.empty()) continue;
							}
							const std::vector<kmx_map_segment> segs = km->seq_to_unitigs(reads, &seg_offsets);
							const std::vector<kmx_walk> wk = km->seq_walks(segs, seg_offsets, ct.link_offsets, ct.links, wp, &walk_offsets, &steps);
							cinner.add(km->seq_pairs(wk, walk_offsets, steps, ct.link_offsets, ct.links, pp, &cplinks));
						}
						km->unitig_map_end();
						if (!write_scaffolds(km, dir, ct.strs, 0, cplinks, p, cinner.inner(), pp.max_dist, "contigs", ct.link_offsets, ct.links)) return 1;
					}
					std::cout << "   contigs (links of >= " << p.min_reads << " reads" << (p.ratio ? ", ratio " : "") << (p.ratio ? std::to_string(p.ratio) : std::string()) << ")    :     " << ct.stats.n_contigs
					          << " contigs (" << ct.stats.n_multi << " of several unitigs, " << ct.stats.n_circular << " circular), " << ct.stats.n_kept << " of " << ct.stats.n_links << " edges kept" << std::endl;
				}
			}
		}
	}
	delete km;
	return 0;
}
