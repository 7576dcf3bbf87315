// graph_checks.h -- what the host forms of the graph calls validate before anything runs, and the buffer check of every call
// that takes more than one buffer.  No HIP: the includer provides include/kmx.h, fail(code, fmt, ...), TRY, u32 and u64
// (kmx_api.hip does; so does tests/graph_checks_driver.cpp, which runs these functions on the CPU under the sanitizers).
#pragma once
#include <cstdint>

// KMX_E_ARG when offsets[0] != 0 or the offsets decrease
static int check_offsets(const uint64_t *offsets, uint64_t n)
{
	if (!offsets) return fail(KMX_E_ARG, "null argument");
	if (offsets[0] != 0) return fail(KMX_E_ARG, "offsets[0] = %llu, not 0", (unsigned long long)offsets[0]);
	for (u64 i = 0; i < n; i++)
		if (offsets[i + 1] < offsets[i]) return fail(KMX_E_ARG, "offsets decrease at sequence %llu", (unsigned long long)i);
	return KMX_OK;
}

static int check_odd_k(int k)
{
	if (k < 5 || k > 63 || !(k & 1)) return fail(KMX_E_ARG, "the unitig graph needs an odd k in [5, 63], not %d (an even k has k-mers that are their own reverse complement)", k);
	return KMX_OK;
}

static int check_unitig_count(u64 U)
{
	if (U >> 31) return fail(KMX_E_ARG, "%llu unitigs: a graph call takes fewer than 2^31", (unsigned long long)U);
	return KMX_OK;
}

// uoffsets [U + 1] has passed check_offsets
static int check_unitig_lengths(const uint64_t *uoffsets, u64 U, int k)
{
	for (u64 u = 0; u < U; u++)
		if (uoffsets[u + 1] - uoffsets[u] < (u64)k) return fail(KMX_E_ARG, "unitig %llu has %llu bytes, fewer than k = %d", (unsigned long long)u, (unsigned long long)(uoffsets[u + 1] - uoffsets[u]), k);
	return KMX_OK;
}

// The edges between U < 2^31 unitigs: link_offsets [2 U + 1] starts at 0, does not decrease and ends at n_links, and every
// target is an oriented unitig.  strict (contigs, resolve): no row holds more than 4 entries, and every edge a -> b has its
// mirror b ^ 1 -> a ^ 1.
static int check_link_csr(const uint64_t *link_offsets, const uint32_t *links, u64 n_links, u64 U, bool strict)
{
	TRY(check_offsets(link_offsets, 2 * U));
	if (link_offsets[2 * U] != n_links) return fail(KMX_E_ARG, "link_offsets end at %llu, not at n_links = %llu", (unsigned long long)link_offsets[2 * U], (unsigned long long)n_links);
	if (n_links && !links) return fail(KMX_E_ARG, "null argument");
	for (u64 e = 0; e < n_links; e++)
		if ((u64)links[e] >= 2 * U) return fail(KMX_E_ARG, "links[%llu] = %u is no oriented unitig of %llu", (unsigned long long)e, links[e], (unsigned long long)U);
	if (!strict) return KMX_OK;
	for (u64 a = 0; a < 2 * U; a++)
		if (link_offsets[a + 1] - link_offsets[a] > 4) return fail(KMX_E_ARG, "the row of oriented unitig %llu has %llu entries, more than 4", (unsigned long long)a, (unsigned long long)(link_offsets[a + 1] - link_offsets[a]));
	for (u64 a = 0; a < 2 * U; a++)
		for (u64 e = link_offsets[a]; e < link_offsets[a + 1]; e++) {
			const u64 b1 = (u64)links[e] ^ 1;
			bool found = false;
			for (u64 f = link_offsets[b1]; f < link_offsets[b1 + 1]; f++) found = found || links[f] == (u32)(a ^ 1);
			if (!found) return fail(KMX_E_ARG, "the edge %llu -> %u has no mirror %llu -> %llu", (unsigned long long)a, links[e], (unsigned long long)b1, (unsigned long long)(a ^ 1));
		}
	return KMX_OK;
}

// a list of pair links (kmx_unitig_pair_walks leaves it, kmx_unitig_scaffold reads it) is strictly ascending by a << 32 | b
static int check_pair_list(const kmx_pair_link *plinks, u64 n)
{
	if (n && !plinks) return fail(KMX_E_ARG, "null argument");
	for (u64 i = 1; i < n; i++)
		if (((u64)plinks[i - 1].a << 32 | plinks[i - 1].b) >= ((u64)plinks[i].a << 32 | plinks[i].b))
			return fail(KMX_E_ARG, "the list of pair links is not strictly ascending at entry %llu", (unsigned long long)i);
	return KMX_OK;
}

// a buffer of a call: [p, p + bytes), written by the call (out) or only read
struct Span {
	const void *p;
	u64 bytes;
	bool out;
};
// a buffer the caller may leave out
static Span opt_span(const void *p, u64 bytes, bool out) { return Span{p, p ? bytes : 0, out}; }

// a and b share a byte
static bool spans_share(const Span &a, const Span &b)
{
	const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
	return a.p && b.p && a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}

// KMX_E_ARG for a null buffer of non-zero size and for an output that shares a byte with another buffer
static int check_spans(const Span *s, int n)
{
	for (int i = 0; i < n; i++)
		if (!s[i].p && s[i].bytes) return fail(KMX_E_ARG, "null argument (buffer %d of the call)", i);
	for (int i = 0; i < n; i++)
		for (int j = i + 1; j < n; j++)
			if ((s[i].out || s[j].out) && spans_share(s[i], s[j])) return fail(KMX_E_ARG, "an output buffer overlaps another buffer of the call (buffers %d and %d)", i, j);
	return KMX_OK;
}
