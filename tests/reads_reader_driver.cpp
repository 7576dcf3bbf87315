// reads_reader_driver.cpp -- the FASTQ / FASTA reader of kmx_build_from_reads (kmcex_amd/csrc/reads_reader.cpp) as a
// stand-alone program for tests/test_reads_reader_cpu.py, which builds it with ASan + UBSan: no HIP, no GPU.
//   driver k batch_bases input        (input: a path or "@list")
// prints "BATCH <n_seqs>" and that batch's sequences one per line, for every batch, then "END"; "ERR <message>" instead of
// END when reads_inputs fails or next() returns -1.  The exit status is 0 either way (2 for a bad command line).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../kmcex_amd/csrc/reads_reader.h"

int main(int argc, char **argv)
{
	if (argc != 4) { fprintf(stderr, "usage: %s k batch_bases input\n", argv[0]); return 2; }
	const int k = atoi(argv[1]);
	const uint64_t batch = strtoull(argv[2], nullptr, 10);
	std::vector<std::string> files;
	std::string err;
	if (!kmx::reads_inputs(argv[3], files, err)) { printf("ERR %s\n", err.c_str()); return 0; }
	kmx::ReadsReader rd(files, k, batch);
	kmx::ReadBatch b;
	for (;;) {
		const int r = rd.next(b);
		if (r < 0) { printf("ERR %s\n", rd.error().c_str()); return 0; }
		if (r == 0) break;
		if (b.offs.empty() || b.offs[0] != 0 || b.offs.back() != b.bases.size()) { printf("ERR driver: the batch's offsets do not span its bases\n"); return 0; }
		printf("BATCH %zu\n", b.offs.size() - 1);
		for (size_t i = 0; i + 1 < b.offs.size(); i++) {
			if (b.offs[i + 1] < b.offs[i]) { printf("ERR driver: the batch's offsets decrease\n"); return 0; }
			if (b.offs[i + 1] > b.offs[i]) fwrite(b.bases.data() + b.offs[i], 1, (size_t)(b.offs[i + 1] - b.offs[i]), stdout);   // (a batch of empty sequences has no bases at all)
			fputc('\n', stdout);
		}
	}
	printf("END\n");
	return 0;
}
