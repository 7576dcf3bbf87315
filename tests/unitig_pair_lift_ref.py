"""The rule of kmx_unitig_pair_lift (include/kmx.h) restated in plain Python: where an oriented unitig lies in its contig, the
class and the shift of every entry, and the LINK contributions folded in a dictionary and sorted.  With flat(), the check of the
rule's consequences (a) to (c), the TSV text the facade must write, and the cases the tests share.  Not a test."""
import functools
import random

import numpy as np

import unitig_contigs_ref as Cn
import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pair_reduce_ref as X
import unitig_pairs_ref as P
import unitig_walk_ref as W
import unitigs_ref as U

PAIR_LIFT_DTYPE = np.dtype([("cls", "<u4"), ("out", "<u4"), ("A", "<u4"), ("B", "<u4"), ("shift", "<i8"), ("flipped", "<u4"), ("reserved", "<u4")])
STAT_FIELDS = ("n_entries", "n_ignored", "n_same", "n_inverted", "n_link", "n_far", "n_same_back", "n_out", "pairs_ignored", "pairs_same", "pairs_inverted", "pairs_link", "pairs_far",
               "pairs_same_back", "sum_same_d", "reserved")
IGNORED, SAME, INVERTED, LINK, FAR = range(5)
CLASSES = ("IGNORED", "SAME", "INVERTED", "LINK", "FAR")
NO_OUT = 2 ** 32 - 1
M64 = 2 ** 64 - 1
ALL = 2 ** 32 - 1                                               # the max_dist that keeps every entry whose maximum can be stored
s64 = X.s64
plinks_array = X.plinks_array
mirrored = X.mirrored


def lies(mu, place, cm, o):
    """-> (O(o), start(o), tail(o), m) of oriented unitig o < 2 U, or None when it is not placed"""
    oc, off = place[o >> 1]
    c, m = oc >> 1, mu[o >> 1]
    if c >= len(cm) or cm[c] >= 2 ** 32 or off + m > cm[c]:
        return None
    r = (o ^ oc) & 1
    start = cm[c] - off - m if r else off
    return 2 * c + r, start, cm[c] - start - m, m


def lift(mu, place, cm, plinks, max_dist):
    """mu: m_u per unitig; place: (oc, off) per unitig; cm: n_kmers per contig; plinks: tuples (a, b, n_pairs, sum_dist, min_dist,
    max_dist) in list order -> a dict: lrec (dicts), lout (tuples), stats"""
    nu = len(mu)
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["n_entries"] = len(plinks)
    recs, merged = [], {}
    for a, b, n, s, lo, hi in plinks:
        rec = {"cls": IGNORED, "out": NO_OUT, "A": 0, "B": 0, "shift": 0, "flipped": 0, "reserved": 0, "key": None}
        ea = lies(mu, place, cm, a) if a < 2 * nu else None
        eb = lies(mu, place, cm, b) if b < 2 * nu else None
        if a < 2 * nu and b < 2 * nu and a >> 1 != b >> 1 and n != 0 and ea and eb:
            (A, sa, ta, ma), (B, sb, tb, mb) = ea, eb
            rec["A"], rec["B"] = A, B
            if A == B:
                rec["cls"], rec["shift"] = SAME, sb - sa - ma + 1
                if lo + rec["shift"] < 0:
                    st["n_same_back"] += 1
                    st["pairs_same_back"] = (st["pairs_same_back"] + n) & M64
                else:
                    st["sum_same_d"] = s64(st["sum_same_d"] + s + n * rec["shift"])
            elif A == B ^ 1:
                rec["cls"] = INVERTED
            else:
                sh = rec["shift"] = ta + sb
                if lo + sh > max_dist or hi + sh >= 2 ** 32:
                    rec["cls"] = FAR
                else:
                    rec["cls"] = LINK
                    key = P.canonical(A, B)
                    rec["flipped"], rec["key"] = int(key != (A, B)), key
                    m = merged.setdefault(key, [0, 0, lo + sh, hi + sh])
                    m[0], m[1], m[2], m[3] = (m[0] + n) & M64, (m[1] + s + n * sh) & M64, min(m[2], lo + sh), max(m[3], hi + sh)
        st[("n_ignored", "n_same", "n_inverted", "n_link", "n_far")[rec["cls"]]] += 1
        f = "pairs_" + CLASSES[rec["cls"]].lower()
        st[f] = (st[f] + n) & M64
        recs.append(rec)
    keys = sorted(merged)
    at = {key: i for i, key in enumerate(keys)}
    for rec in recs:
        key = rec.pop("key")
        if key is not None:
            rec["out"] = at[key]
    st["n_out"] = len(keys)
    return {"lrec": recs, "lout": [(a, b, *merged[a, b]) for a, b in keys], "stats": st}


def flat(res):
    """what the library returns: (PAIR_LIFT_DTYPE [n], PAIR_LINK_DTYPE [n_out], n_out, the stats as a list of 16 numbers)"""
    rec = np.zeros(len(res["lrec"]), dtype=PAIR_LIFT_DTYPE)
    for i, r in enumerate(res["lrec"]):
        for f in PAIR_LIFT_DTYPE.names:
            rec[f][i] = r[f]
    return rec, plinks_array(res["lout"]), len(res["lout"]), [res["stats"][f] for f in STAT_FIELDS]


def identity_place(mu):
    """the place of a contig call that merged nothing -> (place, cm)"""
    return [(2 * u, 0) for u in range(len(mu))], list(mu)


def is_pair_link(e, nu):
    return e[0] < 2 * nu and e[1] < 2 * nu and e[0] >> 1 != e[1] >> 1 and e[2] >= 1


def check(mu, place, cm, plinks, max_dist, canonical=True):
    """consequences (a) to (c) of the rule, asserted on the restatement's own output for one list -> the result"""
    res = lift(mu, place, cm, plinks, max_dist)
    st, recs, nu = res["stats"], res["lrec"], len(mu)
    # (c)
    assert st["n_ignored"] + st["n_same"] + st["n_inverted"] + st["n_link"] + st["n_far"] == st["n_entries"] == len(plinks)
    assert sum(st["pairs_" + c.lower()] for c in CLASSES) & M64 == sum(e[2] for e in plinks) & M64, "consequence (c): the pairs of the classes"
    assert sum(e[2] for e in res["lout"]) & M64 == st["pairs_link"], "consequence (c): the pairs of the list"
    assert st["n_out"] == len(res["lout"]) == len({r["out"] for r in recs if r["cls"] == LINK}) and st["n_same_back"] <= st["n_same"]
    keys = [e[:2] for e in res["lout"]]
    assert keys == sorted(set(keys)) and all(k == P.canonical(*k) for k in keys)
    for r in recs:
        assert (r["cls"] == LINK) == (r["out"] != NO_OUT) and (r["cls"] == LINK or not r["flipped"]) and (r["cls"] != IGNORED or (r["A"], r["B"], r["shift"]) == (0, 0, 0))
    # (a)
    links = [tuple(e) for e in plinks if is_pair_link(e, nu) and e[5] < 2 ** 32]
    if canonical and links:
        ip, icm = identity_place(mu)
        assert lift(mu, ip, icm, links, ALL)["lout"] == links, "consequence (a)"
    # (b)
    for i in sorted({0, len(plinks) // 2, len(plinks) - 1} | {i for i in range(len(plinks)) if i % 11 == 0}) if plinks else ():
        got = lift(mu, place, cm, [mirrored(e) if j == i else e for j, e in enumerate(plinks)], max_dist)
        assert got["lout"] == res["lout"] and got["stats"] == st, "consequence (b): the list"
        for j, (r, q) in enumerate(zip(recs, got["lrec"])):
            if j != i or r["cls"] == IGNORED:
                assert r == q, "consequence (b): the other records"
            else:
                assert (q["A"], q["B"]) == (r["B"] ^ 1, r["A"] ^ 1) and q["flipped"] == (r["flipped"] ^ 1 if r["cls"] == LINK else 0), "consequence (b): A, B, flipped"
                assert all(r[f] == q[f] for f in ("cls", "out", "shift")), "consequence (b): the record"
    if len(plinks) > 1:
        order = list(range(len(plinks)))
        random.Random(len(plinks)).shuffle(order)
        got = lift(mu, place, cm, [plinks[i] for i in order], max_dist)
        assert got["lout"] == res["lout"] and got["stats"] == st and got["lrec"] == [recs[i] for i in order], "consequence (b): a permutation"
    return res


def lift_tsv(plinks, res):
    """the text of KModel::write_pair_lift_tsv: entry, a, b, pairs, class, A, B, shift, out ("c<contig><+|->", "*" for none)"""
    fc = lambda o: f"c{o >> 1}{'-' if o & 1 else '+'}"
    return "".join(f"{i}\t{P.fmt(e[0])}\t{P.fmt(e[1])}\t{e[2]}\t{CLASSES[r['cls']]}\t{'*' if r['cls'] == IGNORED else fc(r['A'])}\t{'*' if r['cls'] == IGNORED else fc(r['B'])}\t{r['shift']}\t"
                   f"{'*' if r['out'] == NO_OUT else r['out']}\n" for i, (e, r) in enumerate(zip(plinks, res["lrec"])))


# ---- crafted places and lists
def random_places(nu, n_contigs, seed, max_m=200):
    """nu unitigs of random m_u dealt onto n_contigs contigs in a random order and on random strands -> (mu, place, cm)"""
    r = random.Random(seed * 7919 + nu)
    mu = [r.randrange(1, max_m) for _ in range(nu)]
    order = list(range(nu))
    r.shuffle(order)
    cuts = sorted(r.sample(range(1, nu), n_contigs - 1)) if n_contigs > 1 else []
    place, cm = [None] * nu, []
    for c, (lo, hi) in enumerate(zip([0] + cuts, cuts + [nu])):
        off = 0
        for u in order[lo:hi]:
            place[u] = (2 * c + r.randrange(2), off)
            off += mu[u]
        cm.append(off)
    return mu, place, cm


@functools.lru_cache(maxsize=None)
def random_case(n, seed, n_contigs=12):
    """n entries with distinct canonical keys over P.CRAFT_U unitigs on n_contigs contigs -> (mu, place, cm, the list)"""
    import unitig_scaffold_ref as S
    mu, place, cm = random_places(P.CRAFT_U, n_contigs, seed)
    return mu, place, cm, S.random_list(n, seed + n)


RUN_EDGES = (63, 1, 1, 62, 1, 1, 64, 62, 1, 1, 65, 2, 63, 64, 62)   # the runs end at 63, 64, 65, 127, 128, 129, 193, 255, 256, 257, 322, 324, 387, 451, 513


@functools.lru_cache(maxsize=None)
def runs_case(lens, mirror_run=-1, seed=1):
    """one run of key-sharing entries per number in lens: run r joins contig 2 r, which holds lens[r] unitigs on random strands, to
    contig 2 r + 1, which is one unitig; every unitig of the former has one entry to the latter, written so that A = 2 (2 r) and
    B = 2 (2 r + 1).  The keys ascend with r, so the sorted work items of run r follow those of run r - 1.  The entries of run
    mirror_run are given as their mirrors (lens as a tuple) -> (mu, place, cm, the list, strictly ascending)"""
    r = random.Random(seed * 31 + sum(lens) + len(lens))
    mu, place, cm, out = [], [], [], []
    for run, ln in enumerate(lens):
        off, first = 0, len(mu)
        for _ in range(ln):
            m = r.randrange(1, 90)
            mu.append(m)
            place.append((2 * (2 * run) + r.randrange(2), off))
            off += m
        cm.append(off)
        y, sy = len(mu), r.randrange(2)
        mu.append(r.randrange(1, 90))
        place.append((2 * (2 * run + 1) + sy, 0))
        cm.append(mu[y])
        for u in range(first, first + ln):
            c = r.randrange(1, 30)
            d = sorted(r.randrange(0, 300) for _ in range(2))
            e = (2 * u + (place[u][0] & 1), 2 * y + sy, c, d[0] + d[1] * (c - 1), d[0], d[1])
            out.append(mirrored(e) if run == mirror_run else e)
    return mu, place, cm, sorted(out)


def classes_case(unplaced=True):
    """every class by hand on two contigs c0 = (u0 +, u1 -, u2 +) and c1 = (u3 +, u4 -), u5 alone in c2 and u6 not placed (not
    unplaced: u6 does not exist, for the host form, which refuses a place that is not placed)
    -> (mu, place, cm, the list, the classes expected)"""
    mu = [10, 20, 30, 40, 50, 60, 70]
    place = [(0, 0), (1, 10), (0, 30), (2, 0), (3, 40), (4, 0), (6, 0)]
    cm = [60, 90, 60]                                              # contig 3 does not exist: u6 is not placed
    rows = [((0, 4, 3, 90, 20, 40), SAME),                         # u0 + ... u2 +: forward
            ((4, 0, 3, 90, 20, 40), SAME),                         # u2 + ... u0 +: backward, min_dist + shift < 0
            ((0, 3, 2, 10, 5, 5), SAME),                           # u1 - lies along c0 +
            ((0, 2, 2, 10, 5, 5), INVERTED),                       # u1 + lies along c0 -
            ((4, 6, 5, 500, 90, 110), LINK),                       # c0 + -> c1 +: shift = 0 + 0
            ((0, 6, 5, 500, 90, 110), FAR),                        # lo = 90 + 50 > 120
            ((4, 9, 1, 7, 7, 2 ** 32 - 1), FAR),                   # lo = 47, but hi = 2^32 - 1 + 40 >= 2^32
            ((5, 6, 2, 30, 25, 5), LINK),                          # c0 - -> c1 +, min_dist > max_dist taken as it is
            ((7, 1, 4, 40, 10, 10), LINK),                         # the mirror of c0 + -> c1 +: folds into the first LINK
            ((9, 10, 2 ** 63, 2 ** 64 - 3, 1, 2), LINK),           # c1 + -> c2 +: the sum wraps
            ((11, 8, 2 ** 63 + 5, 9, 0, 0), LINK),                 # c2 - -> c1 -, its mirror: n_pairs and the sum wrap in the fold
            ((0, 12, 3, 30, 10, 10), IGNORED),                     # u6 is not placed
            ((13, 2, 3, 30, 10, 10), IGNORED),
            ((0, 14, 3, 30, 10, 10), IGNORED),                     # b >= 2 U
            ((2, 3, 3, 30, 10, 10), IGNORED),                      # one unitig
            ((2, 8, 0, 0, 0, 0), IGNORED)]                         # no pairs
    rows.sort()
    nu = 7 if unplaced else 6
    return mu[:nu], place[:nu], cm, [e for e, _ in rows], [c for _, c in rows]


CLASSES_MAX_DIST = 120


# ---- the closed form: window pairs along a sequence, placed by arithmetic on its unitigs and again on its contigs
def window_pairs(k, pieces, rows_n, pairs, max_dist):
    """pieces: (first window along the text, m, the oriented piece that reads along the text) per unitig or contig; pairs: (p, q,
    reverse) with the two inner windows at p <= q of the text, read from the reverse strand when reverse -> what P.pair_walks
    returns for them, every read one walk of one step"""
    mu = [m for _, m, _ in pieces]

    def at(w):
        i = next(i for i, (s, m, _) in enumerate(pieces) if s <= w < s + m)
        return pieces[i][2], w - pieces[i][0], pieces[i][1]

    walks, wo, steps = [], [0], []
    for p, q, reverse in pairs:
        (oa, xa, ma), (ob, xb, mb) = at(p), at(q)
        if reverse:
            oa, xa, ma, ob, xb, mb = ob ^ 1, mb - 1 - xb, mb, oa ^ 1, ma - 1 - xa, ma
        for o, x in ((oa, xa), (ob ^ 1, mb - 1 - xb)):
            walks.append(P.a_walk(30, 30, len(steps), 1, x))
            steps.append(o)
            wo.append(len(walks))
    return P.pair_walks(k, mu, walks, wo, steps, [[] for _ in range(rows_n)], 1, max_dist, 10, 64)


def chain_pieces(n, k, lens, m):
    """Cn.chain_case(n, k, lens, ring=False, fork_every=m) -> (k, mu, the restatement's place and contig lengths, the unitigs'
    pieces, the contigs' pieces, the windows of the text); a contig's piece is found by searching its string in the text"""
    k, strs, rows, hits, text = Cn.chain_case(n, k, lens, False, m)
    res = Cn.contigs(k, strs, None, rows, hits, 1, 0)
    mu = [len(s) - k + 1 for s in strs]
    upieces, at = [], 0
    for u in range(n):
        upieces.append((at, mu[u], 2 * u + int(strs[u] != text[at:at + len(strs[u])])))
        at += mu[u]
    for u in range(n, len(strs)):                                  # the tips lie beside the text: no window of it is theirs
        upieces.append((-1, 0, 2 * u))
    cpieces = []
    for c, s in enumerate(res["cstrs"]):
        f, b = text.find(s), text.find(U.rc(s))
        cpieces.append((f, len(s) - k + 1, 2 * c) if f >= 0 else (b, len(s) - k + 1, 2 * c + 1) if b >= 0 else (-1, 0, 2 * c))
    upieces = [(s, m if s >= 0 else 0, o) for s, m, o in upieces]
    return k, mu, res["place"], [r["n_kmers"] for r in res["crecs"]], upieces, cpieces, len(text) - k + 1


def same_d(pairs):
    return sum(p["d"] for p in pairs if p["cls"] == P.SAME)


# ---- the acceptance case: the three islands of unitig_pair_reduce_ref, each cut into pieces
ISLAND_MAX_DIST = X.ISLAND_GENOME
ISLAND_CUT_SEED = 1


@functools.lru_cache(maxsize=None)
def island_pieces(seed, holes, cut_seed=ISLAND_CUT_SEED):
    """each island of X.three_islands cut into 3 to 5 pieces that overlap by k - 1, a seeded half reverse-complemented, the CSR by
    hand as Cn.cut_case writes it -> (k, the k-mers of the reads, pieces, rows, the reads, the genome)"""
    k, strs, _, genome = X.three_islands(seed, holes)
    _, reads = X.island_reads(seed, holes)
    km, _ = U.listing_of(U.count_kmers(reads, k))
    r = random.Random(cut_seed)
    pieces, fwd_of = [], []
    for s in strs:
        n = r.randrange(3, 6)
        cuts = sorted(r.sample(range(1, len(s) - k + 1), n - 1))
        flip = set(r.sample(range(n), n // 2))
        fwd = []
        for j, (lo, hi) in enumerate(zip([0] + cuts, cuts + [len(s) - k + 1])):
            t = s[lo:hi + k - 1]
            fwd.append(2 * len(pieces) + int(j in flip))
            pieces.append(U.rc(t) if j in flip else t)
        fwd_of.append(fwd)
    rows = [[] for _ in range(2 * len(pieces))]
    for fwd in fwd_of:
        for a, b in zip(fwd, fwd[1:]):
            rows[a].append(b)
            rows[b ^ 1].append(a ^ 1)
    return k, km, pieces, rows, reads, genome


@functools.lru_cache(maxsize=None)
def islands_lifted(seed, holes, cut_seed=ISLAND_CUT_SEED):
    """the acceptance case through the restatements: the pairs mapped onto the pieces, the contigs from the walks' link hits, the
    lift, and the same pairs mapped onto the contigs.  The preconditions of consequence (d) are asserted
    -> a dict of everything the GPU test compares with"""
    k, km, pieces, rows, reads, genome = island_pieces(seed, holes, cut_seed)
    pp = (1, ISLAND_MAX_DIST, 10, 64)
    mu = [len(s) - k + 1 for s in pieces]
    segs, so, _, _ = R.map_reads(km, k, pieces, reads)
    walks, wo, steps, hits, _ = W.walk_segs(k, pieces, segs, so, rows, k, 0)
    assert all(wo[i + 1] - wo[i] == 1 for i in range(len(reads))), "every read is one walk on the pieces: choose another cut seed"
    upairs, ulist, _, _, ust = P.pair_walks(k, mu, walks, wo, steps, rows, *pp)
    ctg = Cn.contigs(k, pieces, None, rows, hits, 1, 0)
    assert len(ctg["cstrs"]) == 3, "three contigs: choose another cut seed"
    cm = [r["n_kmers"] for r in ctg["crecs"]]
    crows = [[t for t, _ in row] for row in ctg["crows"]]
    csegs, cso, _, _ = R.map_reads(km, k, ctg["cstrs"], reads)
    cwalks, cwo, csteps, _, _ = W.walk_segs(k, ctg["cstrs"], csegs, cso, crows, k, 0)
    assert all(cwo[i + 1] - cwo[i] == 1 for i in range(len(reads))), "every read is one walk on the contigs"
    cpairs, clist, _, _, cst = P.pair_walks(k, cm, cwalks, cwo, csteps, crows, *pp)
    assert ust["n_far"] == 0 == cst["n_far"], "no pair is FAR at either level"
    assert all(u["cls"] == P.LINK for u, c in zip(upairs, cpairs) if c["cls"] == P.LINK), "every contig-level LINK pair is a LINK on the pieces"
    res = check(mu, ctg["place"], cm, ulist, ISLAND_MAX_DIST)
    return dict(k=k, km=km, pieces=pieces, rows=rows, reads=reads, genome=genome, mu=mu, ulist=ulist, upairs=upairs, ctg=ctg, cm=cm, crows=crows, clist=clist, cpairs=cpairs, lifted=res)
