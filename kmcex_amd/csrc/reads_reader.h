// reads_reader.h -- the reads kmx_build_from_reads counts: FASTQ or FASTA files, plain or gzip, one path or "@list".
// Host-only C++ (no HIP): batches of sequences in the layout of kmx_count_seqs (bases back to back + 64-bit offsets).
#ifndef KMX_READS_READER_H
#define KMX_READS_READER_H
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace kmx {

// input = one path, or "@file" holding one path per line (blank lines skipped) -> files; false + err when unreadable
bool reads_inputs(const char *input, std::vector<std::string> &files, std::string &err);

struct ReadBatch {
	std::vector<char> bases;        // the sequences back to back
	std::vector<uint64_t> offs;     // [n_seqs + 1], offs[0] = 0
};

class ByteSource;

// The files one after the other, parsed into batches of about `batch_bases` bases.  The format is detected per file from its
// content: gzip by its magic bytes, then FASTQ ('@': 4-line records, the sequence on one line) or FASTA ('>': the sequence
// lines of a record are joined).  A '\r' at a line end is dropped.  A record longer than a batch continues in the next
// batch behind a (k - 1)-base halo, so that every window of it is counted exactly once.
class ReadsReader {
public:
	ReadsReader(const std::vector<std::string> &files, int k, uint64_t batch_bases);
	~ReadsReader();
	// 1: *b holds the next batch; 0: no more input; -1: error() says which file and record failed
	int next(ReadBatch &b);
	const std::string &error() const { return err_; }

private:
	bool open_next();
	bool get_line(std::string &line);
	bool bad(const char *what);

	std::vector<std::string> files_;
	size_t fi_ = 0;
	int k_;
	uint64_t batch_;
	std::unique_ptr<ByteSource> src_;
	bool fastq_ = false;
	uint64_t record_ = 0;           // records begun in the current file
	bool open_seq_ = false;         // the last sequence of the batch is a record still being read
	std::vector<char> carry_;       // the halo of a record cut at a batch's end
	std::vector<char> buf_;
	size_t pos_ = 0, end_ = 0;
	bool eof_ = false;
	std::string err_;
};

}   // namespace kmx
#endif
