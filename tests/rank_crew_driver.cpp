// rank_crew_driver.cpp -- the crew of host threads behind the several-GPU build (kmcex_amd/csrc/rank_crew.h) as a stand-alone
// program for tests/test_rank_crew_cpu.py, which builds it plain, with TSan and with ASan + UBSan: no HIP, no GPU.  One case per
// line of stdin:
//   P S kind r1 r2 s      P ranks walk S steps; in step s: kind N nothing, E rank r1 notes code 100 + r1 with the message
//                         "rank r1 step s", D ranks r1 and r2 both do, A rank r1 throws std::bad_alloc, X std::runtime_error("x")
// and one line of tab-separated fields per case on stdout:
//   code, message, bodies that ran to their end, 1 if every rank's step() returned what rank 0's did at every step, the first
//   step whose return was not 0 (-1: none) and that return, then per rank "steps run:of them without a gap from step 0"
// The exit status is 0, or 2 for a line it cannot read.
#include <atomic>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../kmcex_amd/csrc/rank_crew.h"

enum { OOM = -6, INTERNAL = -1 };

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		int P = 0, S = 0, r1 = 0, r2 = 0, s_bad = 0;
		char kind = 0;
		if (!(in >> P >> S >> kind >> r1 >> r2 >> s_bad) || P < 1 || S < 1 || std::string("NEDAX").find(kind) == std::string::npos || r1 < 0 || r1 >= P || r2 < 0 || r2 >= P) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
		std::vector<std::vector<int>> ret((size_t)P, std::vector<int>((size_t)S, 0)), ran((size_t)P, std::vector<int>((size_t)S, 0));   // a row per rank: nobody shares a cell
		std::atomic<int> ended{0};
		RankCrew crew(P, OOM, INTERNAL);
		const int code = crew.run([&](int d) {
			for (int s = 0; s < S; s++)
				ret[(size_t)d][(size_t)s] = crew.step([&] {
					ran[(size_t)d][(size_t)s] = 1;
					if (s != s_bad || kind == 'N' || (d != r1 && !(kind == 'D' && d == r2))) return true;
					if (kind == 'A') throw std::bad_alloc();
					if (kind == 'X') throw std::runtime_error("x");
					char msg[64];
					snprintf(msg, sizeof msg, "rank %d step %d", d, s);
					return !crew.note(100 + d, msg);
				});
			ended++;
		});
		bool same = code == crew.code();
		int first = -1;
		for (int s = 0; s < S; s++) {
			for (int d = 1; d < P; d++) same = same && ret[(size_t)d][(size_t)s] == ret[0][(size_t)s];
			if (first < 0 && ret[0][(size_t)s]) first = s;
		}
		printf("%d\t%s\t%d\t%d\t%d\t%d", code, crew.message(), ended.load(), same ? 1 : 0, first, first < 0 ? 0 : ret[0][(size_t)first]);
		for (int d = 0; d < P; d++) {
			int n = 0, lead = 0;
			for (int s = 0; s < S; s++) { n += ran[(size_t)d][(size_t)s]; if (lead == s && ran[(size_t)d][(size_t)s]) lead++; }
			printf("\t%d:%d", n, lead);
		}
		printf("\n");
	}
	return 0;
}
