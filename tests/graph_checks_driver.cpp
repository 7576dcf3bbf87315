// graph_checks_driver.cpp -- the argument checks of the graph calls (kmcex_amd/csrc/graph_checks.h) as a stand-alone program
// for tests/test_graph_checks_cpu.py, which builds it plain and with ASan + UBSan: no HIP, no GPU.  It defines what the header
// asks of its includer (fail, TRY, u32, u64; the KMX_* codes are include/kmx.h's), reads one case per line from stdin and
// prints the return code of each:
//   C strict U n_links n_offs offs... n_lk links...     check_link_csr (the arrays hold exactly what the line gives)
//   L U k n_offs offs...                                check_unitig_lengths
//   S n (address bytes out)...                          check_spans (the addresses are never dereferenced; 0 is NULL)
// The exit status is 0, or 2 for a line it cannot read.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/kmx.h"

typedef uint32_t u32;
typedef uint64_t u64;
static char g_err[512];
static int fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

#include "../kmcex_amd/csrc/graph_checks.h"

template <typename T> static bool read_array(std::istream &in, std::vector<T> &v)
{
	size_t n = 0;
	if (!(in >> n)) return false;
	v.resize(n);
	for (T &x : v) {
		u64 y = 0;
		if (!(in >> y)) return false;
		x = (T)y;
	}
	return true;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		char what = 0;
		if (!(in >> what)) continue;
		int rc = 0;
		bool ok = true;
		if (what == 'C') {
			int strict = 0;
			u64 U = 0, n_links = 0;
			std::vector<uint64_t> offs;
			std::vector<uint32_t> links;
			ok = (bool)(in >> strict >> U >> n_links) && read_array(in, offs) && read_array(in, links);
			if (ok) rc = check_link_csr(offs.empty() ? nullptr : offs.data(), links.empty() ? nullptr : links.data(), n_links, U, strict != 0);
		} else if (what == 'L') {
			u64 U = 0;
			int k = 0;
			std::vector<uint64_t> offs;
			ok = (bool)(in >> U >> k) && read_array(in, offs);
			if (ok) rc = check_unitig_lengths(offs.data(), U, k);
		} else if (what == 'S') {
			size_t n = 0;
			ok = (bool)(in >> n);
			std::vector<Span> s(ok ? n : 0);
			for (Span &x : s) {
				u64 p = 0, bytes = 0;
				int out = 0;
				ok = ok && (bool)(in >> p >> bytes >> out);
				x = Span{(const void *)(uintptr_t)p, bytes, out != 0};
			}
			if (ok) rc = check_spans(s.data(), (int)s.size());
		} else
			ok = false;
		if (!ok) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
		printf("%d\n", rc);
	}
	return 0;
}
