"""The rule of kmx_unitig_pair_walks (include/kmx.h) restated in plain Python on top of unitig_walk_ref: the anchor of every read,
the class of every pair, the insert-size histogram, the pairs per edge and the merged list of pair links.  With flat(), the check
of the rule's consequences, the mates swapped, a batch cut, the TSV text the facade must write, and the cases the tests share.
Not a test."""
import functools
import random

import numpy as np

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_walk_ref as W
import unitigs_ref as U

PAIR_DTYPE = np.dtype([("walk_a", "<u8"), ("walk_b", "<u8"), ("cls", "<u4"), ("edge", "<u4"), ("oa", "<u4"), ("xa", "<u4"), ("ob", "<u4"), ("xb", "<u4"),
                       ("d", "<i8"), ("frag", "<i8"), ("reserved", "<u8")])
PAIR_LINK_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("n_pairs", "<u8"), ("sum_dist", "<u8"), ("min_dist", "<u4"), ("max_dist", "<u4")])
STAT_FIELDS = ("n_pairs", "n_none", "n_single", "n_same", "n_negative", "n_inverted", "n_link", "n_adjacent", "n_far", "reserved")
PARTS = ("pairs", "plinks", "hist", "pair_hits", "stats")
NONE, SINGLE, SAME, INVERTED, LINK, FAR = range(6)
NO_WALK, NO_EDGE = 2 ** 64 - 1, 2 ** 32 - 1


def anchor(mu, walks, steps, lo, hi, min_mapped):
    """the anchor of the read whose walks are walks[lo:hi]: (index into walks, o, x, n_span) or None"""
    best = None
    for i in range(lo, hi):
        w = walks[i]
        nm, ns = int(w["n_mapped"]), int(w["n_steps"])
        if nm < min_mapped or ns < 1:
            continue
        at = int(w["first_step"]) + ns - 1
        if at >= len(steps):
            continue
        o, x = int(steps[at]), int(w["off_last"])
        if o >= 2 * len(mu) or x >= mu[o >> 1]:
            continue
        if best is None or min(nm, 2 ** 32 - 1) > best[0]:
            best = (min(nm, 2 ** 32 - 1), i, o, x, int(w["n_span"]))
    return best[1:] if best else None


def canonical(oa, ob):
    return min((oa, ob), (ob ^ 1, oa ^ 1))


def pair_walks(k, mu, walks, walk_offsets, steps, rows, min_mapped, max_dist, bin_width, n_bins, plinks=()):
    """-> (pairs as dicts, the merged list as (a, b, n_pairs, sum_dist, min_dist, max_dist) tuples, hist, pair_hits, stats as a
    dict); plinks is the list earlier batches left, as such tuples"""
    assert (len(walk_offsets) - 1) % 2 == 0 and bin_width >= 1 and 1 <= n_bins <= 65536
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    n_pairs = (len(walk_offsets) - 1) // 2
    pairs, hist, hits = [], [0] * n_bins, [0] * loff[-1]
    merged = {(a, b): [n, s, lo, hi] for a, b, n, s, lo, hi in plinks}
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["n_pairs"] = n_pairs
    for p in range(n_pairs):
        A = anchor(mu, walks, steps, int(walk_offsets[2 * p]), int(walk_offsets[2 * p + 1]), min_mapped)
        B = anchor(mu, walks, steps, int(walk_offsets[2 * p + 1]), int(walk_offsets[2 * p + 2]), min_mapped)
        rec = {"walk_a": A[0] if A else NO_WALK, "walk_b": B[0] if B else NO_WALK, "cls": NONE, "edge": NO_EDGE, "oa": 0, "xa": 0, "ob": 0, "xb": 0, "d": 0, "frag": 0, "reserved": 0}
        if A:
            oa, xa = rec["oa"], rec["xa"] = A[1], A[2]
        if B:
            ob, xb = rec["ob"], rec["xb"] = B[1] ^ 1, mu[B[1] >> 1] - 1 - B[2]
        if not A or not B:
            rec["cls"] = SINGLE if A or B else NONE
            st["n_single" if A or B else "n_none"] += 1
        elif oa == ob:
            rec["cls"], rec["d"] = SAME, xb - xa
            rec["frag"] = frag = xb - xa + A[3] + B[3] + k - 2
            st["n_same"] += 1
            if frag < 0:
                st["n_negative"] += 1
            else:
                hist[min(frag // bin_width, n_bins - 1)] += 1
        elif oa == ob ^ 1:
            rec["cls"] = INVERTED
            st["n_inverted"] += 1
        else:
            rec["d"] = dist = (mu[oa >> 1] - 1 - xa) + xb
            if dist > max_dist:
                rec["cls"] = FAR
                st["n_far"] += 1
            else:
                rec["cls"] = LINK
                st["n_link"] += 1
                row = rows[oa][:4]
                if ob in row:
                    rec["edge"] = e = loff[oa] + row.index(ob)
                    hits[e] += 1
                    st["n_adjacent"] += 1
                m = merged.setdefault(canonical(oa, ob), [0, 0, dist, dist])
                m[0], m[1], m[2], m[3] = m[0] + 1, m[1] + dist, min(m[2], dist), max(m[3], dist)
        pairs.append(rec)
    return pairs, [(a, b, *merged[a, b]) for a, b in sorted(merged)], hist, hits, st


def flat(pairs, plinks, hist, hits, st):
    """what the library returns: (PAIR_DTYPE, PAIR_LINK_DTYPE, uint64 [n_bins], uint64 [n_links], uint64 [10] stats)"""
    p = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    for i, g in enumerate(pairs):
        for f, v in g.items():
            p[f][i] = v
    return (p, flat_list(plinks), np.array(hist, dtype=np.uint64), np.array(hits, dtype=np.uint64), np.array([st[f] for f in STAT_FIELDS], dtype=np.uint64))


def flat_list(plinks):
    return np.array([tuple(x) for x in plinks], dtype=PAIR_LINK_DTYPE)


def swapped(walks, walk_offsets):
    """the same batch with the two mates of every pair swapped -> (walks, walk_offsets, old index of every new walk); steps stay"""
    order, wo = [], [0]
    for p in range((len(walk_offsets) - 1) // 2):
        for r in (2 * p + 1, 2 * p):
            order += range(int(walk_offsets[r]), int(walk_offsets[r + 1]))
            wo.append(len(order))
    return [walks[i] for i in order], wo, order


def cut(walks, walk_offsets, p0, p1):
    """the pairs [p0, p1) as a batch of their own -> (walks, walk_offsets); steps stay"""
    lo, hi = int(walk_offsets[2 * p0]), int(walk_offsets[2 * p1])
    return walks[lo:hi], [int(x) - lo for x in walk_offsets[2 * p0:2 * p1 + 1]]


def mirror_hits(rows, hits):
    """every count moved to its edge's mirror"""
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    out = [0] * len(hits)
    for a, row in enumerate(rows):
        for j, b in enumerate(row):
            out[loff[b ^ 1] + rows[b ^ 1].index(a ^ 1)] += hits[loff[a] + j]
    return out


def check(k, mu, walks, walk_offsets, steps, rows, params, mirrored_graph=True):
    """consequences (a), (b) and (c) of the rule, asserted on the restatement's own output for one input"""
    pairs, plinks, hist, hits, st = pair_walks(k, mu, walks, walk_offsets, steps, rows, *params)
    n_pairs = len(pairs)
    # (b)
    assert st["n_none"] + st["n_single"] + st["n_same"] + st["n_inverted"] + st["n_link"] + st["n_far"] == n_pairs == st["n_pairs"]
    assert sum(x[2] for x in plinks) == st["n_link"] and sum(hist) == st["n_same"] - st["n_negative"] and sum(hits) == st["n_adjacent"]
    assert all(x[4] <= x[3] // x[2] <= x[5] <= params[1] for x in plinks) and [x[:2] for x in plinks] == sorted({x[:2] for x in plinks})
    assert all(canonical(a, b) == (a, b) for a, b, *_ in plinks)
    for r in pairs:
        assert (r["cls"] in (NONE, SINGLE)) == (NO_WALK in (r["walk_a"], r["walk_b"])) and (r["edge"] != NO_EDGE) <= (r["cls"] == LINK)
        assert r["cls"] != LINK or 0 <= r["d"] <= params[1]
        assert r["cls"] != FAR or r["d"] > params[1]
    # (a)
    sw, swo, order = swapped(walks, walk_offsets)
    p2, l2, h2, t2, s2 = pair_walks(k, mu, sw, swo, steps, rows, *params)
    assert l2 == plinks and h2 == hist and s2 == st, "consequence (a)"
    if mirrored_graph:
        assert t2 == mirror_hits(rows, hits), "consequence (a): pair_hits move to the mirror edge"
    for r, q in zip(pairs, p2):
        assert r["cls"] == q["cls"] and (r["cls"] != SAME or (r["d"], r["frag"]) == (q["d"], q["frag"])) and (r["cls"] not in (LINK, FAR) or r["d"] == q["d"])
        assert q["walk_a"] == NO_WALK and r["walk_b"] == NO_WALK or order[q["walk_a"]] == r["walk_b"]
    # (c)
    for pieces in ((n_pairs // 3, n_pairs), tuple(range(1, n_pairs + 1)) if n_pairs <= 64 else (1, n_pairs // 2, n_pairs - 1, n_pairs)):
        lst, hs, ts, at, recs = [], [0] * len(hist), [0] * len(hits), 0, []
        tot = dict.fromkeys(STAT_FIELDS, 0)
        for end in pieces:
            if end <= at:
                continue
            cw, cwo = cut(walks, walk_offsets, at, end)
            base = int(walk_offsets[2 * at])
            pp, lst, h, t, s = pair_walks(k, mu, cw, cwo, steps, rows, *params, plinks=lst)
            hs, ts = [x + y for x, y in zip(hs, h)], [x + y for x, y in zip(ts, t)]
            tot = {f: tot[f] + s[f] for f in STAT_FIELDS}
            recs += [dict(r, walk_a=r["walk_a"] + base if r["walk_a"] != NO_WALK else NO_WALK, walk_b=r["walk_b"] + base if r["walk_b"] != NO_WALK else NO_WALK) for r in pp]
            at = end
        assert (lst, hs, ts, tot, recs) == (plinks, hist, hits, st, pairs), "consequence (c)"
    return pairs, plinks, hist, hits, st


def fmt(o):
    return f"u{o >> 1}{'-' if o & 1 else '+'}"


def links_tsv(plinks, rows):
    """the text of KModel::write_pair_links_tsv"""
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    out = []
    for a, b, n, s, lo, hi in plinks:
        q = (s * 10 + n // 2) // n if n else 0
        row = rows[a][:4] if a < len(rows) else []
        e = str(loff[a] + row.index(b)) if b in row else "-"
        out.append(f"{fmt(a)}\t{fmt(b)}\t{n}\t{q // 10}.{q % 10}\t{lo}\t{hi}\t{e}\n")
    return "".join(out)


def insert_tsv(hist, bin_width):
    """the text of KModel::write_insert_hist_tsv"""
    return "".join(f"{i * bin_width}\t{c}\n" for i, c in enumerate(hist))


# ---- the cases from reads: name -> (k, k-mers, counts, unitig strings, interleaved reads, rows, the genome), computed once
FRAG, READ, K = 400, 100, 21
ONE_SEED, TWO_SEED = 11, 12                                     # genomes whose k-mers (and (k - 1)-mers) are all distinct: checked below


def fragments(genome, starts):
    """FR pairs, interleaved: a fragment of FRAG bases from every start, mate 1 its first READ bases, mate 2 the reverse
    complement of its last READ"""
    out = []
    for s in starts:
        out += [genome[s:s + READ], U.rc(genome[s + FRAG - READ:s + FRAG])]
    return out


def kept_starts():
    """case 2: every start of a 2000-base genome whose pair has no read touching [950, 1050)"""
    touches = lambda a: a < 1050 and a + READ > 950
    return [s for s in range(2000 - FRAG + 1) if not touches(s) and not touches(s + FRAG - READ)]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one_unitig":
        genome = U.rand_seq(3000, ONE_SEED)
        reads = fragments(genome, range(3000 - FRAG + 1))
    else:
        assert name == "two_islands"
        genome = U.rand_seq(2000, TWO_SEED)
        reads = fragments(genome, kept_starts())
    km, cnt = U.listing_of(U.count_kmers(reads, K))
    strs, _ = U.unitigs(km, cnt, K, 1)
    rows = L.links(km, cnt, K, 1, strs)
    assert len(strs) == (1 if name == "one_unitig" else 2) and (name == "one_unitig" or not any(rows)), "choose another genome seed"
    return K, km, cnt, strs, reads, rows, genome


READ_CASES = ("one_unitig", "two_islands")
MAX_DIST = 400
READ_PARAMS = (1, MAX_DIST, 10, 64)                             # min_mapped, max_dist, bin_width, n_bins


@functools.lru_cache(maxsize=None)
def walked(name):
    """the case's reads mapped and walked by the restatements -> (walks, walk_offsets, steps)"""
    k, km, cnt, strs, reads, rows, genome = case(name)
    segs, so, _, _ = R.map_reads(km, k, strs, reads)
    walks, wo, steps, _, _ = W.walk_segs(k, strs, segs, so, rows, k, 0)
    return walks, wo, steps


def island_gap(name="two_islands"):
    """G: from the last window of the first island to the first window of the second, in the genome"""
    return 1050 - (950 - K)


# ---- crafted walk arrays: what real reads do not reach.  The unitig set is U random strings with m_u cycling through MS, so that
# a session on them holds these m_u; the rows are made up (the call reads them, it does not ask where they came from)
MS = (1, 2, 7, 64, 300)
CRAFT_U = 100


@functools.lru_cache(maxsize=None)
def craft_set():
    """-> (k, k-mers, unitig strings, m_u)"""
    strs = [U.rand_seq(MS[u % len(MS)] + K - 1, 1000 + u) for u in range(CRAFT_U)]
    km, cnt = U.listing_of(U.count_kmers(strs, K))
    assert len(km) == sum(len(s) - K + 1 for s in strs) and max(cnt) == 1, "a k-mer occurs twice: choose other seeds"
    return K, km, strs, [len(s) - K + 1 for s in strs]


@functools.lru_cache(maxsize=None)
def craft_rows(seed=3):
    """mirror-symmetric rows of at most 4 entries over the 2 U oriented unitigs, many of them full"""
    r = random.Random(seed)
    rows = [[] for _ in range(2 * CRAFT_U)]
    for _ in range(6 * CRAFT_U):
        a, b = r.randrange(2 * CRAFT_U), r.randrange(2 * CRAFT_U)
        ma, mb = b ^ 1, a ^ 1
        if b in rows[a] or len(rows[a]) >= 4 or len(rows[ma]) >= 4 or (a, b) != (ma, mb) and a == ma and len(rows[a]) >= 3:
            continue
        rows[a].append(b)
        if (ma, mb) != (a, b):
            rows[ma].append(mb)
    assert max(map(len, rows)) == 4 and all(a ^ 1 in rows[b ^ 1] for a, row in enumerate(rows) for b in row)
    return rows


def a_walk(n_mapped, n_span, first_step, n_steps, off_last):
    return {"pos": 0, "n_span": n_span, "n_mapped": n_mapped, "n_covered": n_span + K - 1, "first_seg": 0, "first_step": first_step, "n_segs": 1, "n_steps": n_steps, "off_first": 0,
            "off_last": off_last, "n_inside": 0, "n_across": 0, "indel": 0, "reserved": 0}


@functools.lru_cache(maxsize=None)
def crafted(n_pairs, seed):
    """n_pairs random pairs -> (walks, walk_offsets, steps): reads with no walk, with several walks and ties in n_mapped, with
    walks below min_mapped = 5, without steps, with off_last beyond m_u; mates on the same unitig (frag of either sign), inverted,
    adjacent by a row (the fourth entry included), and anywhere (keys of both orders, unitigs 0 and U - 1 among them)"""
    k, km, strs, mu = craft_set()
    rows = craft_rows()
    r = random.Random(seed)
    walks, wo, steps = [], [0], []

    def read(o, x):
        """a read whose anchor ends at (o, x), among decoys"""
        n = r.choice((0, 1, 1, 1, 2, 3, 4))
        best = r.randrange(5, 60)
        at = r.randrange(n) if n else 0
        for i in range(n):
            if i == at:
                nm, ns, oo, xx = best, r.choice((1, 1, 2, 3)), o, x
            else:
                kind = r.randrange(5)
                nm = best if kind == 0 and i > at else r.randrange(0, best)       # a tie behind the anchor loses; a smaller one loses
                ns, oo, xx = r.choice((1, 2)), r.randrange(2 * CRAFT_U), 0
                if kind == 1:
                    nm, ns = best + 7, 0                         # more windows but no step: no candidate
                elif kind == 2:
                    nm, xx = best + 9, mu[oo >> 1] + r.randrange(3)   # off_last beyond the unitig: no candidate
                elif kind == 3:
                    nm = r.randrange(0, 5)                       # below min_mapped
            walks.append(a_walk(nm, r.choice((0, 1, 3, nm, nm + 40)), len(steps), ns, xx))
            steps.extend([r.randrange(2 * CRAFT_U) for _ in range(ns - 1)] + ([oo] if ns else []))
        wo.append(len(walks))

    for p in range(n_pairs):
        kind = r.randrange(8)
        oa = r.choice((0, 1, 2 * CRAFT_U - 2, 2 * CRAFT_U - 1)) if r.randrange(6) == 0 else r.randrange(2 * CRAFT_U)
        if kind <= 1:
            ob = oa
        elif kind == 2:
            ob = oa ^ 1
        elif kind <= 4 and rows[oa]:
            ob = rows[oa][-1] if r.randrange(2) else r.choice(rows[oa])
        else:
            ob = r.randrange(2 * CRAFT_U)
        xa, xb = r.randrange(mu[oa >> 1]), r.randrange(mu[ob >> 1])
        read(oa, xa)
        read(ob ^ 1, mu[ob >> 1] - 1 - xb)
    return walks, wo, steps


CRAFT_SIZES = (1, 255, 256, 257, 513)
CRAFT_PARAMS = ((5, 120, 16, 12), (5, 0, 1, 1), (0, 2 ** 32 - 1, 7, 65536))


def key_pairs(keys, dists):
    """one LINK pair per (oa, ob) with the distance asked for, every read one walk of one step -> (walks, walk_offsets, steps)"""
    k, km, strs, mu = craft_set()
    walks, wo, steps = [], [0], []
    for (oa, ob), d in zip(keys, dists):
        xb = min(d, mu[ob >> 1] - 1)
        xa = mu[oa >> 1] - 1 - (d - xb)
        assert 0 <= xa and oa >> 1 != ob >> 1
        for o, x in ((oa, xa), (ob ^ 1, mu[ob >> 1] - 1 - xb)):
            walks.append(a_walk(30, 30, len(steps), 1, x))
            steps.append(o)
            wo.append(len(walks))
    return walks, wo, steps


@functools.lru_cache(maxsize=None)
def merge_case():
    """5000 distinct keys, given in either order of the two ends, plus 3000 repeats of them at other distances, shuffled; and a
    second batch of 700 keys of which none is among the first -> ((walks, wo, steps) of the first, of the second)"""
    k, km, strs, mu = craft_set()
    r = random.Random(17)
    seen, keys = set(), []
    while len(keys) < 5700:
        oa, ob = r.randrange(2 * CRAFT_U), r.randrange(2 * CRAFT_U)
        if oa >> 1 == ob >> 1 or canonical(oa, ob) in seen:
            continue
        seen.add(canonical(oa, ob))
        keys.append((oa, ob) if r.randrange(2) else (ob ^ 1, oa ^ 1))
    first = keys[:5000] + [r.choice(((a, b), (b ^ 1, a ^ 1))) for a, b in (r.choice(keys[:5000]) for _ in range(3000))]
    r.shuffle(first)
    room = lambda a, b: mu[a >> 1] + mu[b >> 1] - 2
    return (key_pairs(first, [r.randrange(room(a, b) + 1) for a, b in first]), key_pairs(keys[5000:], [r.randrange(room(a, b) + 1) for a, b in keys[5000:]]))
