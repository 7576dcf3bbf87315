"""kmx_unitig_pair_paths restated in plain Python, straight from the rule in include/kmx.h: every prefix of every entry is
enumerated level by level as a list (no depth-first stack, no running W), the hits are those of the definition, and the effects
are the cells of unitig_resolve_ref.through.  check() tests consequences (a) and (b); flat() gives what the library returns;
paths_tsv() the text of KModel::write_pair_paths_tsv; the rest builds the cases the CPU and GPU tests share."""
import functools
import random

import numpy as np

import unitig_links_ref as L
import unitig_pairs_ref as P
import unitig_resolve_ref as RS
import unitigs_ref as U

PAIR_PATH_DTYPE = np.dtype([("verdict", "<u4"), ("n_steps", "<u4"), ("first_step", "<u8"), ("windows", "<u8"), ("n_hits", "<u4"), ("n_visited", "<u4")])
STAT_FIELDS = ("n_entries", "n_ignored", "n_below_min", "n_no_path", "n_adjacent", "n_path", "n_ambiguous", "n_complex", "n_added", "n_missing")
IGNORED, BELOW_MIN, NO_PATH, ADJACENT, PATH, AMBIGUOUS, COMPLEX = range(7)
VERDICTS = ("IGNORED", "BELOW_MIN", "NO_PATH", "ADJACENT", "PATH", "AMBIGUOUS", "COMPLEX")
MAX_STEPS = 16
PAR = dict(min_pairs=2, inner=300, tol=0, max_steps=8, max_visits=4096)


def s64(x):
    """x as a signed 64-bit value (two's complement, wrapping)"""
    x &= 2 ** 64 - 1
    return x - 2 ** 64 if x >> 63 else x


def bounds(entry, inner, tol):
    """-> (g, lo, hi) of an entry with n_pairs >= 1"""
    g = s64(inner - 1 - entry[3] // entry[2])
    return g, s64(g - tol), s64(g + tol)


def row_of(rows, o, n_u):
    """the read entries of row(o): the first 4, those >= 2 U skipped"""
    return [t for t in rows[o][:4] if t < 2 * n_u]


def search(mu, rows, entry, inner, tol, max_steps, max_visits):
    """-> (n_prefix counted up to max_visits + 1, the hits as (steps, W)); every level is the list of all prefixes of that length"""
    n_u = len(mu)
    a, b = entry[0], entry[1]
    g, lo, hi = bounds(entry, inner, tol)
    if hi < 0:
        return 0, []
    level, n_prefix, hits = [((), 0)], 0, []
    for t in range(max_steps + 1):
        n_prefix += len(level)
        if n_prefix > max_visits:
            return max_visits + 1, []
        nxt = []
        for steps, w in level:
            last = steps[-1] if steps else a
            if b in row_of(rows, last, n_u) and w >= lo:
                hits.append((steps, w))
            if t < max_steps:
                nxt += [(steps + (c,), w + mu[c >> 1]) for c in row_of(rows, last, n_u) if w + mu[c >> 1] <= hi]
        level = nxt
    return n_prefix, hits


def cell_of(rows, p, x, n):
    """the through cell of x between p and n, or None when an index is not found (unitig_resolve_ref.through's)"""
    if (p ^ 1) not in rows[x ^ 1][:4] or n not in rows[x][:4]:
        return None
    i_in, i_out = rows[x ^ 1][:4].index(p ^ 1), rows[x][:4].index(n)
    a, b = (i_in, i_out) if not x & 1 else (i_out, i_in)
    return 16 * (x >> 1) + 4 * a + b


def pair_paths(mu, rows, plinks, min_pairs, inner, tol, max_steps, max_visits, through=None, path_hits=None):
    """-> a dict: recs (one tuple in the order of PAIR_PATH_DTYPE per entry), psteps, through [16 U] and path_hits [n_links] as lists
    (added to the arguments when given), stats"""
    n_u = len(mu)
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    t = list(through) if through is not None else [0] * (16 * n_u)
    ph = list(path_hits) if path_hits is not None else [0] * loff[-1]
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["n_entries"] = len(plinks)
    recs, psteps = [], []
    for e in plinks:
        a, b, n = e[0], e[1], e[2]
        if not (a < 2 * n_u and b < 2 * n_u and a >> 1 != b >> 1 and n >= 1):
            recs.append((IGNORED, 0, 0, 0, 0, 0))
        elif n < min_pairs:
            recs.append((BELOW_MIN, 0, 0, 0, 0, 0))
        else:
            n_prefix, hits = search(mu, rows, e, inner, tol, max_steps, max_visits)
            if n_prefix > max_visits:
                recs.append((COMPLEX, 0, 0, 0, 0, max_visits + 1))
            elif len(hits) != 1:
                recs.append((AMBIGUOUS if hits else NO_PATH, 0, 0, 0, len(hits), n_prefix))
            else:
                steps, w = hits[0]
                recs.append((PATH if steps else ADJACENT, len(steps), len(psteps), w, 1, n_prefix))
                full = (a,) + steps + (b,)
                for j in range(1, len(full) - 1):
                    c = cell_of(rows, full[j - 1], full[j], full[j + 1])
                    st["n_added" if c is not None else "n_missing"] += 1
                    if c is not None:
                        t[c] += n
                if steps:
                    for j in range(len(full) - 1):
                        ph[loff[full[j]] + rows[full[j]][:4].index(full[j + 1])] += n
                psteps += list(steps)
        st["n_" + VERDICTS[recs[-1][0]].lower()] += 1
    return {"recs": recs, "psteps": psteps, "through": t, "path_hits": ph, "stats": st}


def flat(res):
    """what the library returns: (PAIR_PATH_DTYPE [n], uint32 psteps, uint64 through, uint64 path_hits, stats as a dict)"""
    return (np.array(res["recs"], dtype=PAIR_PATH_DTYPE).reshape(-1), np.array(res["psteps"], dtype=np.uint32), np.array(res["through"], dtype=np.uint64),
            np.array(res["path_hits"], dtype=np.uint64), dict(res["stats"]))


def plinks_array(plinks):
    a = np.zeros(len(plinks), dtype=P.PAIR_LINK_DTYPE)
    for i, e in enumerate(plinks):
        a[i] = tuple(e)
    return a


def mirrored(entry):
    return (entry[1] ^ 1, entry[0] ^ 1) + tuple(entry[2:])


def mirror_edge(rows, loff, e):
    """the index of the mirror of edge e (the first match in the mirror row)"""
    a = max(o for o in range(len(rows)) if loff[o] <= e)
    while not rows[a]:
        a -= 1
    b = rows[a][e - loff[a]]
    return loff[b ^ 1] + rows[b ^ 1].index(a ^ 1)


def check(mu, rows, plinks, res, par, mirrored_graph=True):
    """consequences (a) and, on a mirrored CSR whose rows hold at most 4 different entries, (b)"""
    st, recs = res["stats"], res["recs"]
    assert sum(st[f] for f in STAT_FIELDS[1:8]) == st["n_entries"] == len(plinks), "consequence (a): the verdicts"
    assert sum(r[1] for r in recs if r[0] == PATH) == len(res["psteps"]) == st["n_added"] + st["n_missing"], "consequence (a): the steps"
    at = 0
    for r in recs:
        assert r[2] == (at if r[0] in (PATH, ADJACENT) else 0) and (r[0] in (PATH, ADJACENT) or r[1:4] == (0, 0, 0))
        at += r[1] if r[0] == PATH else 0
    if not mirrored_graph:
        return
    mir = pair_paths(mu, rows, [mirrored(e) for e in plinks], **par)
    if any(r[0] == COMPLEX for r in recs + mir["recs"]):
        return
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    assert mir["through"] == res["through"] and mir["stats"] == st, "consequence (b): the same cells"
    for r, q in zip(recs, mir["recs"]):
        assert (r[0], r[1], r[3], r[4]) == (q[0], q[1], q[3], q[4]), "consequence (b): verdict, n_hits, windows"
        if r[0] == PATH:
            assert [x ^ 1 for x in reversed(res["psteps"][r[2]:r[2] + r[1]])] == mir["psteps"][q[2]:q[2] + q[1]], "consequence (b): the steps"
    moved = [0] * loff[-1]
    for e, h in enumerate(res["path_hits"]):
        if h:
            moved[mirror_edge(rows, loff, e)] += h
    assert moved == mir["path_hits"], "consequence (b): the mirror edges"


def fmt_steps(steps):
    return "".join(f"{'<' if o & 1 else '>'}u{o >> 1}" for o in steps) or "*"


def paths_tsv(plinks, res):
    """the text of KModel::write_pair_paths_tsv"""
    out = []
    for i, (e, r) in enumerate(zip(plinks, res["recs"])):
        steps = res["psteps"][r[2]:r[2] + r[1]] if r[0] == PATH else []
        out.append(f"{i}\t{P.fmt(e[0])}\t{P.fmt(e[1])}\t{e[2]}\t{VERDICTS[r[0]]}\t{r[3]}\t{fmt_steps(steps)}\n")
    return "".join(out)


# ---- the acceptance case: a 150-base repeat twice in 1800 bases, error-free FR pairs from every start
@functools.lru_cache(maxsize=None)
def acceptance():
    """-> (k, genome, k-mers, counts, unitig strings, interleaved reads, rows)"""
    k = P.K
    genome = RS.planted_genome(2, 150, 500, 77)
    reads = P.fragments(genome, range(len(genome) - P.FRAG + 1))
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    strs, _ = U.unitigs(km, cnt, k, 1)
    rows = L.links(km, cnt, k, 1, strs)
    return k, genome, km, cnt, strs, reads, rows


ACCEPT_PAR = dict(min_pairs=2, inner=221, tol=21, max_steps=8, max_visits=4096)


# ---- crafted graphs over the pair tests' unitig set (U = 100, m_u cycling through 1, 2, 7, 64, 300): the rows are made up
class Graph:
    """rows under construction, kept mirror-symmetric; unitigs are handed out by their m_u"""

    def __init__(self):
        self.k, _, self.strs, self.mu = P.craft_set()
        self.rows = [[] for _ in range(2 * len(self.mu))]
        self.free = {m: [u for u in range(len(self.mu)) if self.mu[u] == m] for m in P.MS}

    def take(self, m, flip=0):
        return 2 * self.free[m].pop(0) + flip

    def edge(self, a, b):
        self.rows[a].append(b)
        if (b ^ 1, a ^ 1) != (a, b):
            self.rows[b ^ 1].append(a ^ 1)
        assert len(self.rows[a]) <= 4 and len(self.rows[b ^ 1]) <= 4

    def chain(self, nodes):
        for a, b in zip(nodes, nodes[1:]):
            self.edge(a, b)


def entry(a, b, windows, inner, n_pairs=5, rest=0):
    """the entry whose g is `windows`: D = inner - 1 - windows, with a sum_dist that floors when rest > 0"""
    return (a, b, n_pairs, (inner - 1 - windows) * n_pairs + rest, 0, 0)


@functools.lru_cache(maxsize=None)
def crafted():
    """-> (graph, the named entries as {name: (entry, parameters that differ from PAR, the verdict to expect)}).  One graph holds
    every gadget; the gadgets share no unitig, so each entry's search stays inside its own."""
    g = Graph()
    inner = PAR["inner"]
    named = {}
    # a 3-hop path: a -> x (7) -> y (64) -> z (2) -> b, one flipped step
    a, x, y, z, b = g.take(300), g.take(7), g.take(64, 1), g.take(2), g.take(300, 1)
    g.chain([a, x, y, z, b])
    named["three_hops"] = (entry(a, b, 73, inner), {}, PATH)
    named["three_hops_floor"] = (entry(a, b, 73, inner, n_pairs=7, rest=6), {}, PATH)        # sum_dist / n_pairs floors
    named["three_hops_short"] = (entry(a, b, 72, inner), {}, NO_PATH)
    named["three_hops_tol"] = (entry(a, b, 70, inner), dict(tol=3), PATH)
    named["adjacent"] = (entry(a, x, 0, inner), {}, ADJACENT)
    named["below_min"] = (entry(a, b, 73, inner, n_pairs=1), {}, BELOW_MIN)
    named["hi_negative"] = ((a, b, 5, 5 * (inner + 4), 0, 0), dict(tol=3), NO_PATH)              # g = -5, hi = -2
    named["same_unitig"] = ((a, a ^ 1, 5, 50, 0, 0), {}, IGNORED)
    named["no_pairs"] = ((a, b, 0, 0, 0, 0), {}, IGNORED)
    named["beyond_2u"] = ((a, 2 * len(g.mu), 5, 50, 0, 0), {}, IGNORED)
    # a bubble with equal arms (7 and 7) and one with unequal arms (7 and 2)
    a, p, q, b = g.take(300), g.take(7), g.take(7), g.take(300)
    g.chain([a, p, b]), g.chain([a, q, b])
    named["bubble_equal"] = (entry(a, b, 7, inner), {}, AMBIGUOUS)
    a, p, q, b = g.take(300), g.take(7), g.take(2, 1), g.take(300)
    g.chain([a, p, b]), g.chain([a, q, b])
    named["bubble_unequal"] = (entry(a, b, 7, inner), {}, PATH)
    named["bubble_unequal_tol"] = (entry(a, b, 7, inner), dict(tol=5), AMBIGUOUS)
    # a ladder of 3 bubbles with arms 1 and 2: 1 + 2 + 4 + ... prefixes; the one path of W = 3 takes the arm of 1 three times
    nodes = [g.take(300)]
    for _ in range(3):
        p, q, nxt = g.take(1), g.take(2), g.take(64 if _ < 2 else 300)
        g.chain([nodes[-1], p, nxt]), g.chain([nodes[-1], q, nxt])
        nodes.append(nxt)
    a, b = nodes[0], nodes[-1]
    lad = entry(a, b, 3 + 128, inner)
    n_prefix, hits = search(g.mu, g.rows, lad, inner, 0, 8, 65536)
    assert len(hits) == 1 and n_prefix > 8
    named["ladder_at"] = (lad, dict(max_visits=n_prefix), PATH)
    named["ladder_below"] = (lad, dict(max_visits=n_prefix - 1), COMPLEX)
    lad2 = entry(a, b, 4 + 128, inner)                                # three ways to take the arm of 2 once
    n2, hits2 = search(g.mu, g.rows, lad2, inner, 0, 8, 65536)
    assert len(hits2) == 3
    named["ladder_ambiguous_at"] = (lad2, dict(max_visits=n2), AMBIGUOUS)
    named["ladder_ambiguous_below"] = (lad2, dict(max_visits=n2 - 1), COMPLEX)
    # a chain of 16 intermediates (the deepest stack) and one of 17, which misses
    for n, name in ((16, "chain16"), (17, "chain17")):
        nodes = [g.take(300)] + [g.take((1, 2, 7)[i % 3], i % 4 == 0) for i in range(n)] + [g.take(300, 1)]
        g.chain(nodes)
        w = sum(g.mu[o >> 1] for o in nodes[1:-1])
        named[name] = (entry(nodes[0], nodes[-1], w, inner), dict(max_steps=16), PATH if n == 16 else NO_PATH)
        named[name + "_one_step"] = (entry(nodes[0], nodes[-1], w, inner), dict(max_steps=1), NO_PATH)
        named[name + "_first"] = (entry(nodes[0], nodes[2], g.mu[nodes[1] >> 1], inner), dict(max_steps=1), PATH)
    # a self-loop unitig gone round twice: a -> s, s -> s, s -> b
    a, s, b = g.take(300), g.take(7), g.take(300)
    g.chain([a, s, b]), g.edge(s, s)
    named["loop_once"] = (entry(a, b, 7, inner), {}, PATH)
    named["loop_twice"] = (entry(a, b, 14, inner), {}, PATH)
    # a hub: 4 ways in -> x -> h -> y -> 4 ways out.  Every one of the 16 keys passes h between x and y: one cell of through and
    # two cells of path_hits take every addition
    x, h, y = g.take(64), g.take(7), g.take(64)
    g.chain([x, h, y])
    ins, outs = [g.take(64) for _ in range(4)], [g.take(64, 1) for _ in range(4)]
    for o in ins:
        g.edge(o, x)
    for o in outs:
        g.edge(y, o)
    named["hub"] = ([entry(i, o, 135, inner, n_pairs=2 + (i + o) % 5) for i in ins for o in outs], {}, PATH)
    return g, named


def crafted_list(n, seed, par):
    """n entries, strictly ascending, mixing the six outcomes: the named entries whose parameters are `par`'s, the hub's 16 keys,
    then random keys over the whole set (most of them NO_PATH, IGNORED or BELOW_MIN)"""
    g, named = crafted()
    r = random.Random(seed)
    pool = {}
    for name, (e, q, _) in named.items():
        if name != "hub" and dict(PAR, **q) == par:
            pool.setdefault((e[0], e[1]), e)
    for e in named["hub"][0]:
        pool.setdefault((e[0], e[1]), e)
    keys = list(pool)
    r.shuffle(keys)
    out = {key: pool[key] for key in keys[:n]}
    nu = len(g.mu)
    while len(out) < n:
        a, b = r.randrange(2 * nu + 2), r.randrange(2 * nu + 2)
        if (a, b) not in out and (a, b) not in pool:
            npairs = r.choice((0, 1, 2, 3, 9, 40))
            out[(a, b)] = (a, b, npairs, npairs * r.choice((0, 10, 150, 290, 299, 400)) + (r.randrange(npairs) if npairs else 0), 0, 0)
    return sorted(out.values())


def hub_list(n=300):
    """n entries that all pass the hub's middle unitig: the 16 keys of the hub over and over, every other round as their mirrors.  A
    key listed several times and a list out of order: only the device form takes it"""
    g, named = crafted()
    base = named["hub"][0]
    return [base[i % 16] if (i // 16) % 2 == 0 else mirrored(base[i % 16]) for i in range(n)]
