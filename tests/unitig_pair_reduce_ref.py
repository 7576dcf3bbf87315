"""The rule of kmx_unitig_pair_reduce (include/kmx.h) restated in plain Python: eligibility, g, the table of rows with its
duplicates, the side choice with max_row, the witnesses and the verdicts, then the list that stays.  With flat(), the check of the
rule's consequences (a) to (d), the TSV text the facade must write, and the lists the tests share.  Not a test."""
import bisect
import functools
import random

import numpy as np

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pairs_ref as P
import unitig_walk_ref as W
import unitigs_ref as U

PAIR_REDUCE_DTYPE = np.dtype([("verdict", "<u4"), ("via", "<u4"), ("n_via", "<u4"), ("side", "<u4"), ("g", "<i8"), ("delta", "<i8")])
STAT_FIELDS = ("n_entries", "n_ignored", "n_below_min", "n_kept", "n_transitive", "n_complex", "n_out", "n_rows", "n_examined", "reserved")
IGNORED, BELOW_MIN, KEPT, TRANSITIVE, COMPLEX = range(5)
VERDICTS = ("IGNORED", "BELOW_MIN", "KEPT", "TRANSITIVE", "COMPLEX")
NO_VIA = 2 ** 32 - 1
PAR = dict(min_pairs=2, inner=600, tol=0, max_row=64)


def s64(x):
    """x as a wrapping signed 64-bit number"""
    x &= 2 ** 64 - 1
    return x - 2 ** 64 if x >= 2 ** 63 else x


def g_of(entry, inner):
    return s64(inner - 1 - entry[3] // entry[2])


def reduce(mu, plinks, min_pairs, inner, tol, max_row):
    """mu: m_u per unitig; plinks: tuples (a, c, n_pairs, sum_dist, min_dist, max_dist) in list order -> a dict: rrecs (dicts),
    lout (the tuples that stay), origin, stats"""
    assert 1 <= max_row <= 65536
    nu = len(mu)
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["n_entries"] = len(plinks)
    recs, rows = [], []
    for i, e in enumerate(plinks):
        a, c, n = e[:3]
        rec = {"verdict": KEPT, "via": NO_VIA, "n_via": 0, "side": 0, "g": 0, "delta": 0}
        if not (a < 2 * nu and c < 2 * nu and a >> 1 != c >> 1 and n >= 1):
            rec["verdict"] = IGNORED
        elif n < min_pairs:
            rec["verdict"] = BELOW_MIN
        else:
            rec["g"] = g_of(e, inner)
            rows += [(a, c, i), (c ^ 1, a ^ 1, i)]
        recs.append(rec)
    rows.sort()
    st["n_rows"] = len(rows)
    out = lambda o: (bisect.bisect_left(rows, (o,)), bisect.bisect_left(rows, (o + 1,)))

    def first(x, y):
        p = bisect.bisect_left(rows, (x, y))
        return rows[p][2] if p < len(rows) and rows[p][:2] == (x, y) else None

    for i, e in enumerate(plinks):
        rec = recs[i]
        if rec["verdict"] != KEPT:
            continue
        a, c = e[:2]
        (la, ha), (lc, hc) = out(a), out(c ^ 1)
        side = rec["side"] = 0 if ha - la <= hc - lc else 1
        lo, hi = (lc, hc) if side else (la, ha)
        if hi - lo > max_row:
            rec["verdict"] = COMPLEX
            continue
        st["n_examined"] += hi - lo
        wit = []                                                   # (b, delta) of the witness rows, in table order
        for _, dst, j in rows[lo:hi]:
            b = dst ^ 1 if side else dst
            f = first(a, b) if side else first(b, c)
            if f is None:
                continue
            gj, gf = recs[j]["g"], recs[f]["g"]
            delta = s64(rec["g"] - s64((gf if side else gj) + mu[b >> 1] + (gj if side else gf)))
            if -tol <= delta <= tol:
                wit.append((b, delta))
        if wit:
            via = min(b for b, _ in wit)
            of_via = [d for b, d in wit if b == via]
            rec.update(verdict=TRANSITIVE, via=via, n_via=len(wit), delta=of_via[-1] if side else of_via[0])
    for r in recs:
        st[("n_ignored", "n_below_min", "n_kept", "n_transitive", "n_complex")[r["verdict"]]] += 1
    origin = [i for i, r in enumerate(recs) if r["verdict"] != TRANSITIVE]
    st["n_out"] = len(origin)
    return {"rrecs": recs, "lout": [tuple(plinks[i]) for i in origin], "origin": origin, "stats": st}


def plinks_array(plinks):
    return np.array([tuple(x) for x in plinks], dtype=P.PAIR_LINK_DTYPE) if len(plinks) else np.zeros(0, dtype=P.PAIR_LINK_DTYPE)


def flat(res):
    """what the library returns: (PAIR_REDUCE_DTYPE [n], PAIR_LINK_DTYPE [n_out], uint32 origin [n_out], n_out, uint64 [10] stats)"""
    rec = np.zeros(len(res["rrecs"]), dtype=PAIR_REDUCE_DTYPE)
    for i, r in enumerate(res["rrecs"]):
        for f in PAIR_REDUCE_DTYPE.names:
            rec[f][i] = r[f]
    return rec, plinks_array(res["lout"]), np.array(res["origin"], dtype=np.uint32), len(res["origin"]), np.array([res["stats"][f] for f in STAT_FIELDS], dtype=np.uint64)


def mirrored(entry):
    a, c = entry[:2]
    return (c ^ 1, a ^ 1) + tuple(entry[2:])


def check(mu, plinks, par, canonical=True):
    """consequences (a) to (d) of the rule, asserted on the restatement's own output for one list -> the result"""
    res = reduce(mu, plinks, **par)
    st, recs = res["stats"], res["rrecs"]
    # (b)
    assert st["n_ignored"] + st["n_below_min"] + st["n_kept"] + st["n_transitive"] + st["n_complex"] == st["n_entries"] == len(plinks)
    assert st["n_out"] == st["n_entries"] - st["n_transitive"] == len(res["lout"]) == len(res["origin"])
    assert st["n_rows"] == 2 * (st["n_kept"] + st["n_transitive"] + st["n_complex"])
    for r in recs:
        assert (r["verdict"] == TRANSITIVE) == (r["n_via"] >= 1) == (r["via"] != NO_VIA)
        assert r["verdict"] in (KEPT, TRANSITIVE, COMPLEX) or (r["g"], r["delta"], r["side"]) == (0, 0, 0)
        assert -par["tol"] <= r["delta"] <= par["tol"]
    # (a)
    top = max([e[2] for e in plinks], default=0) + 1
    assert reduce(mu, plinks, **dict(par, min_pairs=top))["lout"] == [tuple(e) for e in plinks], "consequence (a): min_pairs above every entry"
    for n in range(min(3, len(plinks) + 1)):
        assert reduce(mu, plinks[:n], **par)["lout"] == [tuple(e) for e in plinks[:n]], "consequence (a): fewer than 3 entries"
    # (d): the same records in input order; a strictly ascending list stays one
    assert res["lout"] == [tuple(plinks[i]) for i in res["origin"]] and res["origin"] == sorted(set(res["origin"]))
    keys = [e[:2] for e in res["lout"]]
    assert not canonical or keys == sorted(set(keys))
    # (c)
    if canonical:
        wits = [witnesses(mu, plinks, i, par) for i, r in enumerate(recs) if r["verdict"] == TRANSITIVE]
        if not any(b ^ 1 in wit for wit in wits for b in wit):     # the premise: no entry has a unitig as a witness in both orientations
            for i in sorted({0, len(plinks) // 2, len(plinks) - 1} | {i for i, r in enumerate(recs) if r["verdict"] == TRANSITIVE and i % 7 == 0}) if plinks else ():
                m = [mirrored(e) if j == i else e for j, e in enumerate(plinks)]
                got = reduce(mu, m, **par)["rrecs"]
                for j, (r, q) in enumerate(zip(recs, got)):
                    assert all(r[f] == q[f] for f in ("verdict", "n_via", "g", "delta")), "consequence (c)"
                    assert q["via"] == (r["via"] ^ 1 if j == i and r["via"] != NO_VIA else r["via"]), "consequence (c): via"
    return res


def witnesses(mu, plinks, i, par):
    """every witness b of entry i over both sides (for the premise of consequence (c))"""
    out = set()
    a, c = plinks[i][:2]
    elig = [e for e in plinks if e[2] >= max(par["min_pairs"], 1)]
    edges = {}
    for e in elig:
        for x, y in ((e[0], e[1]), (e[1] ^ 1, e[0] ^ 1)):
            edges.setdefault((x, y), g_of(e, par["inner"]))
    for (x, b), gj in edges.items():
        if x == a and (b, c) in edges and abs(s64(g_of(plinks[i], par["inner"]) - (gj + mu[b >> 1] + edges[b, c]))) <= par["tol"]:
            out.add(b)
    return out


def fmt_via(v):
    return "*" if v == NO_VIA else f"{'<' if v & 1 else '>'}u{v >> 1}"


def reduce_tsv(plinks, res):
    """the text of KModel::write_pair_reduce_tsv: entry, a, b, pairs, verdict, via, n_via, g, delta"""
    return "".join(f"{i}\t{P.fmt(e[0])}\t{P.fmt(e[1])}\t{e[2]}\t{VERDICTS[r['verdict']]}\t{fmt_via(r['via'])}\t{r['n_via']}\t{r['g']}\t{r['delta']}\n"
                   for i, (e, r) in enumerate(zip(plinks, res["rrecs"])))


# ---- the acceptance case: three islands of one genome, the middle one shorter than the fragment
ISLAND_CASES = ((12, ((900, 910), (1030, 1040))), (12, ((900, 921), (1040, 1075))), (13, ((900, 910), (1030, 1040))), (13, ((900, 921), (1040, 1075))))
ISLAND_GENOME = 2400
SCAFFOLD_PAR = dict(min_pairs=2, ratio=0, inner=221, min_n=0, max_n=1000)
ISLAND_PAR = dict(min_pairs=2, inner=221, tol=P.K, max_row=64)


def island_reads(seed, holes):
    """-> (the genome, the interleaved reads of every fragment no read of which touches a hole)"""
    genome = U.rand_seq(ISLAND_GENOME, seed)
    touches = lambda s: any(s < hi and s + P.READ > lo for lo, hi in holes)
    starts = [s for s in range(ISLAND_GENOME - P.FRAG + 1) if not touches(s) and not touches(s + P.FRAG - P.READ)]
    return genome, P.fragments(genome, starts)


@functools.lru_cache(maxsize=None)
def three_islands(seed, holes):
    """unitig_pairs_ref's library (every fragment no read of which touches a hole) on a genome of ISLAND_GENOME bases, through
    the restatements -> (k, unitig strings, the pair list as tuples, the genome)"""
    k = P.K
    genome, reads = island_reads(seed, holes)
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    strs, _ = U.unitigs(km, cnt, k, 1)
    rows = L.links(km, cnt, k, 1, strs)
    assert len(strs) == 3 and not any(rows), "choose another genome seed"
    segs, so, _, _ = R.map_reads(km, k, strs, reads)
    walks, wo, steps, _, _ = W.walk_segs(k, strs, segs, so, rows, k, 0)
    mu = [len(s) - k + 1 for s in strs]
    out = P.pair_walks(k, mu, walks, wo, steps, rows, *P.READ_PARAMS)
    return k, strs, [tuple(int(x) for x in e) for e in out[1]], genome


# ---- crafted lists
LINE_K, LINE_WINDOW, LINE_INNER = 21, 400, 600
LINE_SEEDS = {3: 9, 40: 1, 300: 1}                              # with noise 1: lists with a tenth TRANSITIVE and a tenth KEPT at tol 0, 1 and 40


def entry(a, c, g, inner, n_pairs=5, rest=0, canonical=True):
    """an entry whose g is exactly g: sum_dist = (inner - 1 - g) * n_pairs + rest with rest < n_pairs"""
    d = inner - 1 - g
    assert d >= 0 and 0 <= rest < n_pairs
    a, c = P.canonical(a, c) if canonical else (a, c)
    return (a, c, n_pairs, d * n_pairs + rest, d, d + (1 if rest else 0))


@functools.lru_cache(maxsize=None)
def line_list(n, seed, noise):
    """n entries over unitigs of random length laid on a line in a random order with random flips: one entry for every two
    unitigs whose facing ends are within LINE_WINDOW bases, its g the true one plus noise in [-noise, noise]; keys canonical,
    the list strictly ascending -> (mu, the list).  The first n entries by their far end are taken."""
    r = random.Random(seed * 1000 + n)
    nu = n + 2
    lens = [r.randrange(LINE_K, LINE_K + 150) for _ in range(nu)]
    pos, at = [], 0
    for ln in lens:
        pos.append(at)
        at += ln + r.randrange(0, 60)
    name = list(range(nu))
    r.shuffle(name)                                                # the unitig at place t of the line is name[t]
    flip = [r.randrange(2) for _ in range(nu)]
    mu = [0] * nu
    for t, u in enumerate(name):
        mu[u] = lens[t] - LINE_K + 1
    out = []
    for s in range(1, nu):                                         # by the far end, so that the first n entries leave no skip without its steps
        for t in range(s):
            gap = pos[s] - pos[t] - lens[t]
            if gap > LINE_WINDOW or len(out) == n:
                continue
            g = gap + LINE_K - 1 + r.randrange(-noise, noise + 1)
            c = r.randrange(2, 10)
            out.append(entry(2 * name[t] + flip[t], 2 * name[s] + flip[s], g, LINE_INNER, c, r.randrange(c)))
    assert len(out) == n and len({e[:2] for e in out}) == n
    return mu, sorted(out)


def hub_list(deg, extra_a=0, extra_c=0, errs=(0, 1, -1, 2, -2, 50)):
    """two hubs A = unitig 0 and C = unitig 1 with the entry A -> C over deg - 1 middle unitigs: A -> mid and mid -> C for each,
    so |out(A)| = |out(C ^ 1)| = deg; extra_a more entries out of A and extra_c more into C go to unitigs of their own.
    delta of A -> C over middle t is -errs[t % len(errs)] -> (mu, the list, the index of A -> C)"""
    r = random.Random(deg)
    nu = 2 + (deg - 1) + extra_a + extra_c
    mu = [30, 40] + [r.randrange(1, 200) for _ in range(nu - 2)]
    inner, G = 2000, 700
    out = [entry(0, 2, G, inner)]
    for t in range(deg - 1):
        u = 2 + t
        o = 2 * u + (t & 1)                                          # both orientations of middles occur
        out += [entry(0, o, 5 + t % 3, inner, 3 + t % 4, t % 3), entry(o, 2, G - (5 + t % 3) - mu[u] + errs[t % len(errs)], inner, 4, t % 4)]
    for t in range(extra_a):
        out.append(entry(0, 2 * (1 + deg + t), 9, inner))
    for t in range(extra_c):
        out.append(entry(2 * (1 + deg + extra_a + t) + 1, 2, 9, inner))
    out.sort()
    return mu, out, [e[:2] for e in out].index(P.canonical(0, 2))
