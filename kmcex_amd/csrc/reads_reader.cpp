// reads_reader.cpp -- FASTQ / FASTA parsing for kmx_build_from_reads (see reads_reader.h).
// zlib is opened with dlopen("libz.so.1") when a gzip file is met, as multi_build.h opens librccl: libkmx.so does not link it.
#include "reads_reader.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>

namespace kmx {

class ByteSource {
public:
	virtual ~ByteSource() {}
	virtual long read(char *p, size_t n) = 0;                      // bytes read, 0 at the end, < 0 on an error
};

namespace {

class FileSource : public ByteSource {
public:
	explicit FileSource(FILE *f) : f_(f) {}
	~FileSource() override { fclose(f_); }
	long read(char *p, size_t n) override
	{
		const size_t r = fread(p, 1, n, f_);
		return r ? (long)r : (ferror(f_) ? -1 : 0);
	}
private:
	FILE *f_;
};

struct Zlib {
	void *h = nullptr;
	void *(*open)(const char *, const char *) = nullptr;
	int (*read)(void *, void *, unsigned) = nullptr;
	int (*close)(void *) = nullptr;
	const char *(*error)(void *, int *) = nullptr;
};
static const Zlib &zlib()
{
	static const Zlib z = [] {
		Zlib r;
		r.h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
		if (r.h) {
			r.open = (void *(*)(const char *, const char *))dlsym(r.h, "gzopen");
			r.read = (int (*)(void *, void *, unsigned))dlsym(r.h, "gzread");
			r.close = (int (*)(void *))dlsym(r.h, "gzclose");
			r.error = (const char *(*)(void *, int *))dlsym(r.h, "gzerror");
		}
		return r;
	}();
	return z;
}

class GzSource : public ByteSource {
public:
	explicit GzSource(void *gz) : gz_(gz) {}
	~GzSource() override { zlib().close(gz_); }
	// gzread hands out what a stream that ends early (or is damaged after some good blocks) still decodes and then reports
	// the end of the file; only gzerror tells that from a whole stream (Z_OK = 0, Z_STREAM_END = 1)
	long read(char *p, size_t n) override
	{
		const int r = zlib().read(gz_, p, (unsigned)std::min<size_t>(n, 1u << 30));
		int e = 0;
		zlib().error(gz_, &e);
		return e < 0 ? -1 : r;
	}
private:
	void *gz_;
};

}   // namespace

bool reads_inputs(const char *input, std::vector<std::string> &files, std::string &err)
{
	files.clear();
	if (input[0] != '@') {
		files.push_back(input);
		return true;
	}
	FILE *f = fopen(input + 1, "rb");
	if (!f) { err = std::string("cannot open the list ") + (input + 1); return false; }
	char line[8192];
	while (fgets(line, sizeof line, f)) {
		size_t n = strlen(line);
		while (n && (line[n - 1] == '\n' || line[n - 1] == '\r' || line[n - 1] == ' ' || line[n - 1] == '\t')) line[--n] = 0;
		if (n) files.push_back(line);
	}
	fclose(f);
	if (files.empty()) { err = std::string("the list ") + (input + 1) + " names no file"; return false; }
	return true;
}

ReadsReader::ReadsReader(const std::vector<std::string> &files, int k, uint64_t batch_bases)
	: files_(files), k_(k), batch_(batch_bases), buf_(size_t(1) << 20) {}
ReadsReader::~ReadsReader() {}

bool ReadsReader::bad(const char *what)
{
	err_ = files_[fi_] + ": record " + std::to_string(record_) + ": " + what;
	return false;
}

// the next file, its compression and its format; false with err_ set when it cannot be read
bool ReadsReader::open_next()
{
	const std::string &path = files_[fi_];
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) { err_ = "cannot open " + path; return false; }
	unsigned char mg[2] = {0, 0};
	const size_t nm = fread(mg, 1, 2, f);
	if (nm == 2 && mg[0] == 0x1f && mg[1] == 0x8b) {
		fclose(f);
		const Zlib &z = zlib();
		if (!z.open || !z.read || !z.close || !z.error) { err_ = path + ": gzip input, but libz.so.1 cannot be loaded"; return false; }
		void *gz = z.open(path.c_str(), "rb");
		if (!gz) { err_ = "cannot open " + path; return false; }
		src_.reset(new GzSource(gz));
	} else {
		rewind(f);
		src_.reset(new FileSource(f));
	}
	pos_ = end_ = 0;
	eof_ = false;
	record_ = 0;
	// the format: the first byte that is not white space
	for (;;) {
		if (pos_ == end_) {
			const long r = src_->read(buf_.data(), buf_.size());
			if (r < 0) { err_ = path + ": read error"; return false; }
			if (r == 0) { eof_ = true; fastq_ = false; return true; }   // an empty file holds no record
			pos_ = 0;
			end_ = (size_t)r;
		}
		const char c = buf_[pos_];
		if (c == '@') { fastq_ = true; return true; }
		if (c == '>') { fastq_ = false; return true; }
		if (c != '\n' && c != '\r' && c != ' ' && c != '\t') { err_ = path + ": neither FASTQ ('@') nor FASTA ('>')"; return false; }
		pos_++;
	}
}

// one line without its '\n' (and a '\r' before it); false at the end of the file (err_ set on a read error)
bool ReadsReader::get_line(std::string &line)
{
	line.clear();
	bool any = false;
	for (;;) {
		if (pos_ == end_) {
			if (eof_) break;
			const long r = src_->read(buf_.data(), buf_.size());
			if (r < 0) { err_ = files_[fi_] + ": read error (a damaged gzip stream?)"; eof_ = true; return false; }
			if (r == 0) { eof_ = true; break; }
			pos_ = 0;
			end_ = (size_t)r;
		}
		any = true;
		const char *p = buf_.data() + pos_, *nl = (const char *)memchr(p, '\n', end_ - pos_);
		if (nl) {
			line.append(p, nl - p);
			pos_ += (size_t)(nl - p) + 1;
			break;
		}
		line.append(p, end_ - pos_);
		pos_ = end_;
	}
	if (!line.empty() && line.back() == '\r') line.pop_back();
	return any;
}

int ReadsReader::next(ReadBatch &b)
{
	b.bases.clear();
	b.offs.assign(1, 0);
	size_t part = 0;                                               // where the open FASTA record's part of this batch starts
	if (open_seq_) b.bases.assign(carry_.begin(), carry_.end());
	carry_.clear();
	std::string line, seq, plus, qual;
	for (;;) {
		if (!src_) {
			if (fi_ == files_.size()) return b.offs.size() > 1 ? 1 : 0;
			if (!open_next()) return -1;
		}
		if (fastq_) {
			do {
				if (!get_line(line)) break;
			} while (line.empty());
			if (line.empty()) {                                    // the end of the file
				if (!err_.empty()) return -1;
				src_.reset();
				fi_++;
				continue;
			}
			record_++;
			if (line[0] != '@') { bad("a FASTQ record does not start with '@'"); return -1; }
			if (!get_line(seq) || !get_line(plus) || !get_line(qual)) {
				if (err_.empty()) bad("truncated FASTQ record");
				return -1;
			}
			if (plus.empty() || plus[0] != '+') { bad("no '+' line after the sequence"); return -1; }
			if (qual.size() != seq.size()) { bad("the quality line and the sequence differ in length"); return -1; }
			b.bases.insert(b.bases.end(), seq.begin(), seq.end());
			b.offs.push_back(b.bases.size());
			if (b.bases.size() >= batch_) return 1;
			continue;
		}
		if (!get_line(line)) {                                     // the end of a FASTA file closes its last record
			if (!err_.empty()) return -1;
			if (open_seq_) b.offs.push_back(b.bases.size());
			open_seq_ = false;
			src_.reset();
			fi_++;
			continue;
		}
		if (line.empty()) continue;
		if (line[0] == '>') {
			if (open_seq_) b.offs.push_back(b.bases.size());
			record_++;
			open_seq_ = true;
			part = b.bases.size();
			continue;
		}
		if (!open_seq_) { bad("a FASTA sequence line before the first '>' header"); return -1; }
		b.bases.insert(b.bases.end(), line.begin(), line.end());
		if (b.bases.size() >= batch_) {                            // cut the record: its last k - 1 bases open the next batch
			const size_t len = b.bases.size() - part, h = std::min<size_t>(len, (size_t)(k_ - 1));
			carry_.assign(b.bases.end() - h, b.bases.end());
			b.offs.push_back(b.bases.size());
			return 1;
		}
	}
}

}   // namespace kmx
