"""The cleaning rule of kmx_unitig_graph_clean (include/kmx.h) restated in plain Python on top of unitigs_ref and
unitig_links_ref: round by round, the unitig graph of the working counts, one verdict per unitig from its record and the rows
around it, then the counts of the removed unitigs' nodes set to 0.  With the checks of an output and hand-built shapes.  Not a
test."""
import random

import numpy as np

import unitig_links_ref as UL
import unitigs_ref as U

TIPS, ISLANDS, BUBBLES = 1, 2, 4
MAX_ROUNDS = 64
STATS = ("rounds_run", "converged", "n_tips", "n_islands", "n_bubbles", "n_kmers_removed", "n_unitigs_before", "n_links_before")


def ins(rows, t):
    """in(t) = { s ^ 1 : s in out(t ^ 1) }"""
    return [s ^ 1 for s in rows[t ^ 1]]


def short_tip(r, max_tip):
    return not r["circular"] and r["n_kmers"] <= max_tip and (r["n_pred"] == 0) != (r["n_succ"] == 0)


def arm(r, max_bubble):
    return not r["circular"] and r["n_kmers"] <= max_bubble and r["n_pred"] == 1 and r["n_succ"] == 1


def tip_beats(recs, w, u, max_tip):
    if not short_tip(recs[w], max_tip):
        return True
    kw, ku = (recs[w]["n_kmers"], recs[w]["sum_count"]), (recs[u]["n_kmers"], recs[u]["sum_count"])
    return kw > ku or (kw == ku and w < u)


def verdicts(recs, rows, ops, max_tip, max_bubble):
    """-> one of 0, TIPS, ISLANDS, BUBBLES per unitig: what removes it this round"""
    out = []
    for u, r in enumerate(recs):
        v = 0
        if r["circular"]:
            pass
        elif r["n_pred"] == 0 and r["n_succ"] == 0:
            if r["n_kmers"] <= max_tip and ops & ISLANDS:
                v = ISLANDS
        elif short_tip(r, max_tip):
            o = 2 * u if r["n_succ"] > 0 else 2 * u + 1
            if ops & TIPS and all(any(s >> 1 != u and tip_beats(recs, s >> 1, u, max_tip) for s in ins(rows, t)) for t in rows[o]):
                v = TIPS
        elif arm(r, max_bubble):
            (b,), (a,) = rows[2 * u], rows[2 * u + 1]
            if ops & BUBBLES and b >> 1 != u and a >> 1 != u:
                for p in ins(rows, b):
                    w = p >> 1
                    if w == u or not arm(recs[w], max_bubble) or rows[p] != [b] or rows[p ^ 1] != [a]:
                        continue
                    kw, ku = (recs[w]["sum_count"], recs[w]["n_kmers"]), (r["sum_count"], r["n_kmers"])
                    if kw > ku or (kw == ku and w < u):
                        v = BUBBLES
        out.append(v)
    return out


def clean(kmers, counts, k, thr, ops=7, max_tip=None, max_bubble=None, max_rounds=16):
    """-> dict: strs, recs, rows (the cleaned graph, in the original listing's indices and counts), removed (the round per
    entry), stats, log (per round: unitigs at its start and what it removed), work (the working counts at the end)"""
    assert thr >= 1 and 1 <= ops <= 7 and 1 <= max_rounds <= MAX_ROUNDS
    max_tip = 2 * k if max_tip is None else max_tip
    max_bubble = 2 * k if max_bubble is None else max_bubble
    idx = {x: i for i, x in enumerate(kmers)}
    work = list(counts)
    removed = [0] * len(kmers)
    st = dict.fromkeys(STATS, 0)
    log = []
    rnd = 0
    while True:
        strs, recs = U.unitigs(kmers, work, k, thr)
        rows = UL.links(kmers, work, k, thr, strs)
        if rnd == 0:
            st["n_unitigs_before"], st["n_links_before"] = len(strs), sum(len(r) for r in rows)
        if rnd == max_rounds:                                  # the last round still removed something
            st["rounds_run"], st["converged"] = rnd, 0
            break
        rnd += 1
        v = verdicts(recs, rows, ops, max_tip, max_bubble)
        entry = {"unitigs": len(strs), "tips": v.count(TIPS), "islands": v.count(ISLANDS), "bubbles": v.count(BUBBLES), "kmers": 0}
        for u, kind in enumerate(v):
            if kind:
                s = strs[u]
                for p in range(len(s) - k + 1):
                    i = idx[U.canon(s[p:p + k])]
                    assert work[i] >= thr and not removed[i]
                    work[i], removed[i] = 0, rnd
                    entry["kmers"] += 1
        log.append(entry)
        st["n_tips"] += entry["tips"]
        st["n_islands"] += entry["islands"]
        st["n_bubbles"] += entry["bubbles"]
        st["n_kmers_removed"] += entry["kmers"]
        if not any(v):
            st["rounds_run"], st["converged"] = rnd, 1
            break
    return {"strs": strs, "recs": recs, "rows": rows, "removed": removed, "stats": st, "log": log, "work": work}


def n50(strs):
    ls = sorted((len(s) for s in strs), reverse=True)
    half, acc = sum(ls) / 2, 0
    for x in ls:
        acc += x
        if acc >= half:
            return x
    return 0


def check_clean(kmers, counts, k, thr, ops, max_tip, max_bubble, max_rounds, res):
    """the four consequences of the rule and UL.check_links, asserted on an output of clean() (or of the library, in the same
    dict); the rounds are replayed from res["removed"]"""
    removed, st = res["removed"], res["stats"]
    n = len(kmers)
    assert len(removed) == n and all(0 <= r <= st["rounds_run"] for r in removed)
    assert all(r == 0 for r, c in zip(removed, counts) if c < thr), "an entry that never was a node is marked"
    assert sum(1 for r in removed if r) == st["n_kmers_removed"]
    assert 1 <= st["rounds_run"] <= max_rounds and st["converged"] in (0, 1)
    idx = {x: i for i, x in enumerate(kmers)}
    # 3. original coordinates and counts: the output is the unitig graph of the original listing with the removed counts at 0
    work = [0 if r else c for r, c in zip(removed, counts)]
    strs, recs = U.unitigs(kmers, work, k, thr)
    assert strs == res["strs"] and recs == res["recs"], "the output is not the unitig graph of the surviving nodes"
    U.check(kmers, work, k, thr, res["strs"], res["recs"])
    for s, r in zip(res["strs"], res["recs"]):
        cs = [counts[idx[U.canon(s[p:p + k])]] for p in range(len(s) - k + 1)]
        assert (r["sum_count"], r["min_count"], r["max_count"]) == (sum(cs), min(cs), max(cs)) and kmers[r["first_node"]] == U.canon(s[:k])
    off, lk = UL.flat_links(res["rows"])
    UL.check_links(kmers, work, k, thr, res["strs"], res["recs"], off, lk)
    # 2. the uncleaned capacities suffice
    strs0, recs0 = U.unitigs(kmers, counts, k, thr)
    rows0 = UL.links(kmers, counts, k, thr, strs0)
    assert (st["n_unitigs_before"], st["n_links_before"]) == (len(strs0), sum(len(r) for r in rows0))
    assert len(res["strs"]) <= len(strs0) and sum(map(len, res["strs"])) <= sum(map(len, strs0)) and len(lk) <= st["n_links_before"]
    # 4. a no-op is exact
    if not any(removed):
        assert (st["rounds_run"], st["converged"]) == (1, 1) and res["strs"] == strs0 and res["recs"] == recs0 and res["rows"] == rows0
    # 1. no junction is orphaned, round by round
    for rnd in range(1, st["rounds_run"] + 1):
        w = [0 if 0 < r < rnd else c for r, c in zip(removed, counts)]
        strs_r, recs_r = U.unitigs(kmers, w, k, thr)
        rows_r = UL.links(kmers, w, k, thr, strs_r)
        gone = [removed[idx[U.canon(s[:k])]] == rnd for s in strs_r]
        for u, s in enumerate(strs_r):                         # a unitig goes whole or not at all
            assert all((removed[idx[U.canon(s[p:p + k])]] == rnd) == gone[u] for p in range(len(s) - k + 1))
        for t in range(2 * len(strs_r)):
            if not gone[t >> 1] and ins(rows_r, t):
                assert any(not gone[s >> 1] for s in ins(rows_r, t)), "a junction lost every unitig that entered it"
        if rnd == st["rounds_run"] and st["converged"]:
            assert not any(gone)
        else:
            assert any(gone)


# ---- hand-built shapes: name -> (k, thr, sequences, params or None); params = (ops, max_tip, max_bubble, max_rounds)
def _rs(r, n):
    return "".join(r.choice("ACGT") for _ in range(n))


def _other(c, j=0):
    return [b for b in "ACGT" if b != c][j]


def y_shape(k, seed, long_len, short_len, short2=None, times=(2, 2, 2)):
    """a stem (given times[0] times) that forks into a branch of long_len k-mers and one of short_len (and a third of short2)"""
    r = random.Random(seed)
    stem = _rs(r, k + 30)
    first = r.sample("ACGT", 3)
    seqs = [stem] * times[0]
    seqs += [stem[-(k - 1):] + first[0] + _rs(r, long_len - 1)] * times[1]
    seqs += [stem[-(k - 1):] + first[1] + _rs(r, short_len - 1)] * times[2]
    if short2 is not None:
        seqs += [stem[-(k - 1):] + first[2] + _rs(r, short2 - 1)] * times[2]
    return seqs


def equal_tips(k, seed, extra_on_second=0):
    """a long stem into two branches of 10 k-mers; the second branch given 1 + extra_on_second times"""
    r = random.Random(seed)
    stem = _rs(r, 4 * k)
    a, b = r.sample("ACGT", 2)
    ta = stem[-(k - 1):] + a + _rs(r, 9)
    tb = stem[-(k - 1):] + b + _rs(r, 9)
    return [stem, ta] + [tb] * (1 + extra_on_second)


def two_junction_tip(k, seed):
    """a dead-end unitig x of 12 k-mers whose attached end has two successors, and a second, shorter dead end that enters the
    same two.  (In a de Bruijn graph every predecessor z + core has every successor core + c, so the sets in(t) of the targets
    of one end are equal: a tip is beaten at all of its junctions or at none.)  x wins at both and stays, the shorter goes."""
    r = random.Random(seed)
    x = _rs(r, k + 11)
    c1, c2 = r.sample("ACGT", 2)
    core = x[-(k - 1):]
    short = _rs(r, 4) + _other(x[-k]) + core
    return [x + c1 + _rs(r, 5 * k), x + c2 + _rs(r, 5 * k), short + c1]


def snp_bubble(k, seed, times_a=2, times_b=1):
    r = random.Random(seed)
    left, right = _rs(r, 3 * k), _rs(r, 3 * k)
    a, b = r.sample("ACGT", 2)
    return [left + a + right] * times_a + [left + b + right] * times_b


def hairpin_arm(k, seed):
    """q forks into p + h + rc(h) and into a long x: the unitig that runs from the fork into the palindromic junction has
    n_pred = n_succ = 1, and its one edge out is the hairpin onto its own reverse complement; and a homopolymer run between
    two random flanks shorter than a tip: once they are clipped, C^k alone is an arm whose edges are its self-loop"""
    r = random.Random(seed)
    q, h, x = _rs(r, 3 * k), _rs(r, k + 8), _rs(r, 3 * k)
    c = _other(h[0])
    return [q + h + U.rc(h), q + c + x, _rs(r, k) + "C" * (k + 5) + _rs(r, k)]


def stem_merge(k, seed):
    """left - (junction with a tip) - middle - (junction with a tip) - right: clipping both tips merges three unitigs into one"""
    r = random.Random(seed)
    g = _rs(r, 9 * k)
    p1, p2 = 3 * k, 6 * k
    t1 = g[p1 - (k - 1):p1] + _other(g[p1]) + _rs(r, 6)
    t2 = g[p2 - (k - 1):p2] + _other(g[p2]) + _rs(r, 8)
    return [g, g, g, t1, t2]


def geometry_listing(n_uni, seed, k=31):
    """a listing of exactly n_uni unitigs before cleaning: one Y whose short branch is a clippable tip (3 unitigs), one SNP
    bubble (4 unitigs), and disjoint long paths for the rest -> (k-mers, counts)"""
    r = random.Random(seed)
    seqs = y_shape(k, seed + 1, 3 * k, 5) + snp_bubble(k, seed + 2)
    seqs += [_rs(r, 3 * k + 5) for _ in range(n_uni - 7)]
    km, cnt = U.listing_of(U.count_kmers(seqs, k))
    return km, cnt


CLEAN_CASES = {
    "y_short_branch_goes": lambda: (21, 1, y_shape(21, 1, 80, 10), None),
    "y_two_equal_short_lower_index_survives": lambda: (21, 1, equal_tips(21, 2), None),
    "y_equal_length_sum_decides": lambda: (21, 1, equal_tips(21, 3, 1), None),
    "tip_into_two_junctions_stays": lambda: (21, 1, two_junction_tip(21, 4), None),
    "tip_on_a_cycle_closes_it": lambda: (21, 1, U.cycle_and_tip(), None),
    "snp_bubble_unequal": lambda: (31, 1, snp_bubble(31, 5, 2, 1), None),
    "snp_bubble_equal": lambda: (31, 1, snp_bubble(31, 6, 1, 1), None),
    "hairpin_and_self_loop_arms_stay": lambda: (21, 1, hairpin_arm(21, 7), None),
    "tip_of_exactly_max_tip": lambda: (21, 1, y_shape(21, 8, 80, 12), (7, 12, 42, 16)),
    "tip_of_max_tip_plus_one": lambda: (21, 1, y_shape(21, 8, 80, 13), (7, 12, 42, 16)),
    "k63_y_and_bubble": lambda: (63, 1, y_shape(63, 9, 200, 10) + snp_bubble(63, 10), None),
    "stem_merges_three": lambda: (21, 1, stem_merge(21, 11), None),
}


def params_of(k, p):
    return (7, 2 * k, 2 * k, 16) if p is None else p


def clean_case(name):
    """-> (k, thr, k-mers, counts, params, result of clean) for a case of CLEAN_CASES"""
    k, thr, seqs, p = CLEAN_CASES[name]()
    km, cnt = U.listing_of(U.count_kmers(seqs, k))
    p = params_of(k, p)
    return k, thr, km, cnt, p, clean(km, cnt, k, thr, *p)


def flat(res):
    """what the library returns for a result of clean(): (bases, offsets, records, link_offsets, links, removed uint8)"""
    buf, off, rec = U.flat(res["strs"], res["recs"])
    loff, lk = UL.flat_links(res["rows"])
    return buf, off, rec, loff, lk, np.array(res["removed"], dtype=np.uint8)
