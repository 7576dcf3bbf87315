// rank_crew.h -- P host threads (ranks) that walk one list of steps and agree, at every barrier, on whether the work is still
// alive.  Host code without HIP and without the library's error plumbing: multi_build.h includes it, and so does a plain C++
// program (tests/rank_crew_driver.cpp).
//
// The rule: an error is NOTED into a live slot at any time (the first wins), and becomes the crew's AGREED error only at a barrier
// -- the last thread to arrive copies it before it releases the others.  A rank never reads the live slot: inside a piece of work
// it keeps an `ok` of its own, between two pieces it goes by the agreed error alone, which is the same on every rank.  So all
// ranks run or skip a piece together, and nobody is left waiting for a peer that gave up.
#pragma once
#include <atomic>
#include <cstdio>
#include <exception>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

namespace {
// The host threads only ENQUEUE (nobody waits for a device between two barriers of a round), so a barrier is crossed within
// microseconds: spin, and give the core away only when there are more threads than cores.  `last` runs on the thread that
// arrives last, before anybody is released.
struct HostBarrier {
	std::atomic<int> waiting{0};
	std::atomic<unsigned> gen{0};
	int n;
	explicit HostBarrier(int n_) : n(n_) {}
	template <typename F> void wait(F &&last)
	{
		const unsigned g = gen.load(std::memory_order_acquire);
		if (waiting.fetch_add(1, std::memory_order_acq_rel) + 1 == n) { last(); waiting.store(0, std::memory_order_relaxed); gen.fetch_add(1, std::memory_order_release); return; }
		for (int spins = 0; gen.load(std::memory_order_acquire) == g; spins++) { if (spins > 4000) std::this_thread::yield(); else __builtin_ia32_pause(); }
	}
};

class RankCrew {
	const int P_, oom_, internal_;                               // ranks; the caller's codes for bad_alloc and for any other exception
	HostBarrier bar_;
	std::mutex mu_;
	std::atomic<int> live_{0};                                   // the first error noted, with its message (under mu_)
	char msg_[512] = "";
	int agreed_ = 0;                                             // live_ as of the last barrier: written by its last arrival, read between barriers

public:
	RankCrew(int P, int oom_code, int internal_code) : P_(P), oom_(oom_code), internal_(internal_code), bar_(P) {}
	int note(int code, const char *message)
	{
		if (code) { std::lock_guard<std::mutex> lk(mu_); if (!live_.load()) { snprintf(msg_, sizeof msg_, "%s", message ? message : ""); live_ = code; } }
		return code;
	}
	// f() -> bool on this rank unless the crew has agreed on an error; an exception is noted, not passed on.  false: skipped or failed.
	template <typename F> bool work(F &&f)
	{
		if (agreed_) return false;
		try { return f(); }
		catch (const std::bad_alloc &) { note(oom_, "out of host memory"); }
		catch (const std::exception &e) { char b[480]; snprintf(b, sizeof b, "internal error: %s", e.what()); note(internal_, b); }
		catch (...) { note(internal_, "internal error"); }
		return false;
	}
	int sync() { bar_.wait([this] { agreed_ = live_.load(); }); return agreed_; }        // the barrier; what every rank agrees on from here
	template <typename F> int step(F &&f) { work(f); return sync(); }                     // a piece of work every rank runs or skips, then the barrier
	// body(d) on P - 1 new threads and, for d = 0, on the caller's: everything in it that may fail or throw goes through work / step,
	// and every rank calls sync / step equally often.  A thread that cannot be created ends the crew with an error before anybody waits.
	template <typename B> int run(B &&body)
	{
		std::vector<std::thread> th;
		std::atomic<bool> go{false}, cancel{false};
		try {
			th.reserve((size_t)P_);
			for (int d = 1; d < P_; d++)
				th.emplace_back([&, d] { while (!go.load(std::memory_order_acquire)) { if (cancel.load(std::memory_order_acquire)) return; std::this_thread::yield(); } body(d); });
		} catch (...) {
			cancel.store(true, std::memory_order_release);
			for (auto &x : th) x.join();
			char b[64];
			snprintf(b, sizeof b, "cannot start %d host threads", P_);
			return note(oom_, b);
		}
		go.store(true, std::memory_order_release);
		body(0);
		for (auto &x : th) x.join();
		return code();
	}
	int code() const { return live_.load(); }                    // (after run: the threads are joined)
	const char *message() const { return msg_; }
};
}   // namespace
