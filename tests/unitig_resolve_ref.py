"""The rules of kmx_unitig_walk_through and kmx_unitig_resolve (include/kmx.h) restated in plain Python on top of unitig_walk_ref and
unitig_contigs_ref: the through hits of a batch's walks, the verdict per unitig, and the graph with every resolved unitig split into
one copy per way in.  With flat(), the checks of the rules' consequences and the cases the tests share (the listed cases of the
contigs with their real walks, planted repeats, synthetic through matrices on real graphs, the emit geometry, and the gadgets and
ladders by hand of tests/test_gpu_unitig_scale.py).  Not a test."""
import functools
import hashlib
import random

import numpy as np

import unitig_contigs_ref as G
import unitig_links_ref as L
import unitig_map_ref as R
import unitig_walk_ref as W
import unitigs_ref as U

THROUGH_STAT_FIELDS = ("n_walks", "n_steps", "n_interior", "n_added", "n_missing")
RESOLVE_STAT_FIELDS = ("n_candidates", "n_resolved", "n_crossed", "n_unsupported", "n_ambiguous", "n_copies_added", "n_unitigs_out", "reserved")
RESOLVE_PLACE_DTYPE = np.dtype([("first", "<u4"), ("n_copies", "<u4")])
PARTS = ("rseq", "roffsets", "rrec", "origin", "rplace", "rlink_offsets", "rlinks", "link_origin", "rlink_hits", "stats", "counts")
PARAMS = ((1, 0), (2, 0), (2, 1))                              # (min_reads, max_cross) every case runs at
WALK_PARAMS = ("exact", "bridged")                             # walked at (0, 0) and at (k, 1)


# ---- through hits

def through(walks, steps, rows, n_u, into=None):
    """-> (through [16 U] as a list, added to `into` when given, stats as a dict)"""
    t = list(into) if into is not None else [0] * (16 * n_u)
    st = dict.fromkeys(THROUGH_STAT_FIELDS, 0)
    st["n_walks"], st["n_steps"] = len(walks), len(steps)
    for w in walks:
        mine = steps[w["first_step"]:w["first_step"] + w["n_steps"]]
        for i in range(1, len(mine) - 1):
            x, p, n = mine[i], mine[i - 1], mine[i + 1]
            st["n_interior"] += 1
            if max(x, p, n) >= 2 * n_u or (p ^ 1) not in rows[x ^ 1][:4] or n not in rows[x][:4]:
                st["n_missing"] += 1
                continue
            i_in, i_out = rows[x ^ 1][:4].index(p ^ 1), rows[x][:4].index(n)
            a, b = (i_in, i_out) if not x & 1 else (i_out, i_in)
            t[16 * (x >> 1) + 4 * a + b] += 1
            st["n_added"] += 1
    return t, st


def check_through(rows, n_u, t, st, hits=None):
    """consequences (a) and (c) of the through hits on an output made with the CSR the walks were made with"""
    assert st["n_missing"] == 0 and st["n_interior"] == st["n_added"] == sum(t), "consequence (a)"
    loff = G.offsets_of(rows)
    for u in range(n_u):
        left, right = rows[2 * u + 1], rows[2 * u]
        cell = lambda a, b: t[16 * u + 4 * a + b]
        assert all(cell(a, b) == 0 for a in range(4) for b in range(4) if a >= len(left) or b >= len(right)), "a cell outside the two rows"
        if hits is None:
            continue
        for a in range(len(left)):
            e = loff[2 * u + 1] + a
            assert sum(cell(a, b) for b in range(4)) <= hits[e] + hits[G.mirror_index(rows, loff, 2 * u + 1, a)], "consequence (c), a row"
        for b in range(len(right)):
            e = loff[2 * u] + b
            assert sum(cell(a, b) for a in range(4)) <= hits[e] + hits[G.mirror_index(rows, loff, 2 * u, b)], "consequence (c), a column"


# ---- resolution

def verdict(rows, u, t, min_reads, max_cross):
    """-> (kind, pi): kind None for no candidate, else "crossed", "unsupported", "resolved" or "ambiguous"; pi[a] = b when resolved"""
    left, right = rows[2 * u + 1], rows[2 * u]
    p = len(left)
    if p != len(right) or p < 2 or any(x >> 1 == u for x in left + right):
        return None, None
    cell = [[t[16 * u + 4 * a + b] for b in range(p)] for a in range(p)]
    sup = [[c >= min_reads and c >= 1 for c in row] for row in cell]
    if any(not sup[a][b] and cell[a][b] > max_cross for a in range(p) for b in range(p)):
        return "crossed", None
    if not any(any(row) for row in sup):
        return "unsupported", None
    if all(sum(row) == 1 for row in sup) and all(sum(sup[a][b] for a in range(p)) == 1 for b in range(p)):
        return "resolved", [row.index(True) for row in sup]
    return "ambiguous", None


def resolve(k, strs, recs, rows, hits, t, min_reads, max_cross):
    """-> a dict: the new unitigs (strings, records as dicts or None, origin), rplace, the new rows, link_origin, rlink_hits (or None),
    the stats"""
    n_u = len(strs)
    loff = G.offsets_of(rows)
    st = dict.fromkeys(RESOLVE_STAT_FIELDS, 0)
    pi = [None] * n_u
    for u in range(n_u):
        kind, perm = verdict(rows, u, t, min_reads, max_cross)
        if kind is not None:
            st["n_candidates"] += 1
            st["n_" + kind] += 1
            pi[u] = perm
    copies = [len(pi[u]) if pi[u] is not None else 1 for u in range(n_u)]
    first = [0]
    for c in copies:
        first.append(first[-1] + c)
    st["n_unitigs_out"], st["n_copies_added"] = first[-1], first[-1] - n_u

    def target(o, tgt):
        v, dt = tgt >> 1, tgt & 1
        if pi[v] is None:
            return 2 * first[v] + dt
        i = rows[tgt ^ 1].index(o ^ 1)
        return 2 * (first[v] + (i if dt == 0 else pi[v].index(i))) + dt

    rstrs, rrecs, origin, rrows, lorig = [], ([] if recs is not None else None), [], [], []
    for u in range(n_u):
        for c in range(copies[u]):
            rstrs.append(strs[u])
            origin.append(u)
            if recs is not None:
                r = dict(recs[u])
                if pi[u] is not None:
                    r["n_pred"] = r["n_succ"] = 1
                rrecs.append(r)
            for d in (0, 1):
                o = 2 * u + d
                js = range(len(rows[o])) if pi[u] is None else ([pi[u][c]] if d == 0 else [c])
                rrows.append([target(o, rows[o][j]) for j in js])
                lorig += [loff[o] + j for j in js]
    return {"rstrs": rstrs, "rrecs": rrecs, "origin": origin, "rplace": [(first[u], copies[u]) for u in range(n_u)], "rrows": rrows, "link_origin": lorig,
            "rlink_hits": [hits[e] for e in lorig] if hits is not None else None, "stats": st}


def flat(res):
    """what the library returns: (uint8 rseq, uint64 roffsets [U' + 1], UNITIG_DTYPE [U'] or an empty array, uint32 origin [U'],
    RESOLVE_PLACE_DTYPE [U], uint64 rlink_offsets [2 U' + 1], uint32 rlinks, uint64 link_origin, uint64 rlink_hits or an empty array,
    uint64 [8] stats, uint64 [2] n_unitigs_out, n_bases_out)"""
    buf, off = R.join(res["rstrs"])
    rec = U.flat(res["rstrs"], res["rrecs"])[2] if res["rrecs"] is not None else np.zeros(0, dtype=np.uint8)
    place = np.array(res["rplace"], dtype=np.uint32).reshape(-1, 2).copy().view(RESOLVE_PLACE_DTYPE).reshape(-1)
    loff, lk = L.flat_links(res["rrows"])
    lh = np.array(res["rlink_hits"], dtype=np.uint64) if res["rlink_hits"] is not None else np.zeros(0, dtype=np.uint64)
    st = np.array([res["stats"][f] for f in RESOLVE_STAT_FIELDS], dtype=np.uint64)
    return (buf, off, rec, np.array(res["origin"], dtype=np.uint32), place, loff, lk, np.array(res["link_origin"], dtype=np.uint64), lh, st,
            np.array([len(res["rstrs"]), len(buf)], dtype=np.uint64))


def digest(parts) -> str:
    h = hashlib.sha256()
    for part in parts:
        h.update(np.ascontiguousarray(part).tobytes())
    return h.hexdigest()


def check_resolved(k, strs, rows, res, overlaps_hold=True):
    """consequences (a) and (b) of the resolution on an output: an exact no-op where nothing was resolved, and a graph that
    kmx_unitig_contigs accepts: mirrored, rows of at most 4, no edge twice, the edge count kept, every overlap holding"""
    rrows, rstrs, st = res["rrows"], res["rstrs"], res["stats"]
    assert st["n_candidates"] == st["n_resolved"] + st["n_crossed"] + st["n_unsupported"] + st["n_ambiguous"]
    assert len(rstrs) == st["n_unitigs_out"] == len(strs) + st["n_copies_added"] and len(rrows) == 2 * len(rstrs)
    assert sum(map(len, rrows)) == sum(map(len, rows)) and sorted(res["link_origin"]) == list(range(sum(map(len, rows)))), "every input edge becomes exactly one new edge"
    for u, (f, n) in enumerate(res["rplace"]):
        assert res["origin"][f:f + n] == [u] * n and rstrs[f:f + n] == [strs[u]] * n
    for a, row in enumerate(rrows):
        assert len(row) <= 4 and len(set(row)) == len(row), "rows of at most 4, no edge twice"
        for b in row:
            assert (a ^ 1) in rrows[b ^ 1], "the new CSR is mirrored"
            if overlaps_hold:
                x, y = R.oriented(rstrs, a), R.oriented(rstrs, b)
                assert x[len(x) - (k - 1):] == y[:k - 1]
    if st["n_resolved"] == 0:
        assert rstrs == list(strs) and rrows == [list(r) for r in rows] and res["origin"] == list(range(len(strs))) and res["link_origin"] == list(range(sum(map(len, rows))))


# ---- the cases

_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def rc_any(s):
    """the reverse complement of a read that may hold lower case and other letters (these stay what they are)"""
    return s[::-1].translate(_COMP)


@functools.lru_cache(maxsize=None)
def listed_through(name, which):
    """the through hits of a listed case of the contigs from its real walks -> (through as a tuple, stats)"""
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    walks, _, steps, _, _ = listed_walks(name, which)
    t, st = through(walks, steps, rows, len(strs))
    return tuple(t), st


@functools.lru_cache(maxsize=None)
def listed_walks(name, which, mirrored=False):
    """the walks of a listed case (mirrored: of the reverse complements of its reads) -> what unitig_walk_ref.walk_segs returns"""
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    gap, indel = (0, 0) if which == "exact" else (k, 1)
    if not mirrored and name != G.RING:
        return W.walked(name, gap, indel)
    segs, so, _, _ = R.map_reads(km, k, strs, [rc_any(r) for r in reads] if mirrored else reads)
    return W.walk_segs(k, strs, segs, so, rows, gap, indel)


def planted_genome(n_copies, repeat_len, flank_len, seed):
    """flanks of random bases joined by one repeat string.  The last base of in-flank i is "ACGT"[i] and the first base of the flank
    behind it "ACGT"[(i + 1) % 4]: two flanks that share a boundary base would lengthen the repeat by a base on one side"""
    rep = U.rand_seq(repeat_len, seed)
    flanks = [list(U.rand_seq(flank_len, seed + 1 + i)) for i in range(n_copies + 1)]
    for i in range(n_copies):
        flanks[i][-1] = "ACGT"[i % 4]
        flanks[i + 1][0] = "ACGT"[(i + 1) % 4]
    return rep.join("".join(f) for f in flanks)


PLANTED = {   # name -> (k, copies, repeat length, flank length, read length)
    "k21_2x40": (21, 2, 40, 150, 100), "k21_3x40": (21, 3, 40, 150, 100), "k31_4x45": (31, 4, 45, 150, 100), "k63_3x70": (63, 3, 70, 150, 160),
    "k21_2x120": (21, 2, 120, 150, 100), "k5_2x9": (5, 2, 9, 40, 30),
}


@functools.lru_cache(maxsize=None)
def planted_case(name):
    """-> (k, genome, km, cnt, strs, recs, reads, rows, link hits and through hits of the reads walked at (0, 0))"""
    k, n, rl, fl, read_len = PLANTED[name]
    genome = planted_genome(n, rl, fl, 4000 + 16 * k + n)
    reads = [genome[a:a + read_len] for a in range(0, len(genome) - read_len + 1, 3)]
    reads = [r if i % 2 == 0 else U.rc(r) for i, r in enumerate(reads)]
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    strs, recs = U.unitigs(km, cnt, k, 1)
    rows = L.links(km, cnt, k, 1, strs)
    segs, so, _, _ = R.map_reads(km, k, strs, reads)
    walks, _, steps, hits, _ = W.walk_segs(k, strs, segs, so, rows, 0, 0)
    t, _ = through(walks, steps, rows, len(strs))
    return k, genome, km, cnt, strs, recs, reads, rows, hits, t


def synthetic_through(rows, n_u, seed):
    """per candidate, seeded, one of: a permutation with supports 2 to 4; the same plus one cross cell of 1; plus one of 3; all zero"""
    r = random.Random(seed)
    t = [0] * (16 * n_u)
    for u in range(n_u):
        if verdict(rows, u, t, 1, 0)[0] is None:
            continue
        p = len(rows[2 * u])
        kind = r.randrange(4)
        if kind == 3:
            continue
        perm = list(range(p))
        r.shuffle(perm)
        for a in range(p):
            t[16 * u + 4 * a + perm[a]] = r.randint(2, 4)
        if kind:
            a = r.randrange(p)
            b = r.choice([x for x in range(p) if x != perm[a]])
            t[16 * u + 4 * a + b] = 1 if kind == 1 else 3
    return t


SYNTH_SEED = 11


@functools.lru_cache(maxsize=None)
def synthetic_case(name):
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    return tuple(synthetic_through(rows, len(strs), SYNTH_SEED))


SYNTH_CASES = ("k5_complete", "k31_tangle", "k33_tangle", "k21_every_kind")


def geometry_case(length, shift, k=21):
    """one unitig of `length` bytes with 4 ways in and 4 ways out that pair one to one, behind a neighbour of 21 + shift bytes: the
    CSR and the strings by hand (the overlaps do not hold; the bytes are copied all the same) -> (k, strs, rows, through)"""
    strs = [U.rand_seq(k + shift, 9100 + shift), U.rand_seq(length, 9200 + length)] + [U.rand_seq(k + 2, 9300 + i) for i in range(8)]
    rows = [[] for _ in range(2 * len(strs))]
    for i in range(4):
        rows[2 * (2 + i)].append(2)                              # way in i: unitig 2 + i -> unitig 1
        rows[3].append(2 * (2 + i) + 1)
        rows[2].append(2 * (6 + i))                              # way out i: unitig 1 -> unitig 6 + i
        rows[2 * (6 + i) + 1].append(3)
    t = [0] * (16 * len(strs))
    for a, b in enumerate((2, 0, 3, 1)):
        t[16 + 4 * a + b] = 5
    return k, strs, rows, t


GEOMETRY_LENGTHS = (21, 22, 4 * 16 + 15, 4 * 16 + 16, 4 * 16 + 17, 4095, 4096, 4097, 9000)


def _stored(strs, rows, pairs, seed):
    """the case as the library sees it: a seeded half of the unitigs reverse-complemented, their rows mirrored accordingly, and the
    through hits of `pairs` (centre, oriented way in, oriented way out, count, all as built) counted by the rule of through()
    -> (strs, rows, through)"""
    n_u = len(strs)
    r = random.Random(seed)
    flip = [0] * n_u
    for u in r.sample(range(n_u), n_u // 2):
        flip[u] = 1
    nm = lambda o: o ^ flip[o >> 1]
    out_strs = [U.rc(s) if flip[u] else s for u, s in enumerate(strs)]
    out_rows = [None] * (2 * n_u)
    for o, row in enumerate(rows):
        out_rows[nm(o)] = [nm(t) for t in row]
    t = [0] * (16 * n_u)
    for c, p, n, count in pairs:
        x, p, n = nm(2 * c), nm(p), nm(n)
        i_in, i_out = out_rows[x ^ 1].index(p ^ 1), out_rows[x].index(n)
        a, b = (i_in, i_out) if not x & 1 else (i_out, i_in)
        t[16 * c + 4 * a + b] += count
    return out_strs, out_rows, t


def _arms(k, centre, p, r):
    """p ways in and p ways out of a centre, of k or k + 1 bytes each, whose overlaps with the centre hold"""
    ins = [U.rand_seq(1 + r.randrange(2), r.randrange(1 << 30)) + centre[:k - 1] for _ in range(p)]
    outs = [centre[len(centre) - (k - 1):] + U.rand_seq(1 + r.randrange(2), r.randrange(1 << 30)) for _ in range(p)]
    return ins, outs


def nth_permutation(p, index):
    """permutation number `index` of range(p), in lexicographic order"""
    left, out = list(range(p)), []
    for i in range(p, 0, -1):
        f = 1
        for x in range(2, i):
            f *= x
        out.append(left.pop(index // f))
        index %= f
    return out


GADGET_PIN = (3, 1)                                            # (min_reads, max_cross) at which a gadget's verdict is the planned one
GADGET_GROUP = 192                                             # gadgets per group of the layout


def gadget_plan(n_gadgets, spoil_every):
    """per gadget (p, permutation number, None or the way it is spoiled); p = 2 + g % 3 and the number (g // 3) % p!, so all
    2 + 6 + 24 pairs occur within 72 gadgets; every spoil_every-th one is spoiled, the three ways in rotation"""
    fact = {2: 2, 3: 6, 4: 24}
    return [(2 + g % 3, (g // 3) % fact[2 + g % 3], ("ambiguous", "crossed", "unsupported")[(g // spoil_every) % 3] if spoil_every and g % spoil_every == spoil_every - 1 else None)
            for g in range(n_gadgets)]


@functools.lru_cache(maxsize=None)
def gadget_case(n_gadgets, k, lens, spoil_every, seed=0):
    """disjoint gadgets: gadget g is a centre of lens[g % len(lens)] bytes with p ways in and p ways out (gadget_plan), arms of k or
    k + 1 bytes.  Way in a is paired with way out perm[a] by a count of 3 to 5.  A spoiled gadget, at GADGET_PIN: one count moved to
    another way out (ambiguous), one more cell of 2 (crossed: below min_reads, above max_cross), or every count 1 (unsupported).
    The layout, in groups of GADGET_GROUP gadgets: the group's centres of fewer than 256 bytes, then all its arms, then its long
    centres, so that one tile of the flat input holds hundreds of starts, resolved and unresolved, and long pieces begin in a dense
    tile.  A seeded half of all unitigs is stored reverse-complemented -> (k, strs, rows, through), as geometry_case"""
    r = random.Random(7700 + seed * 977 + n_gadgets * 31 + k)
    plan = gadget_plan(n_gadgets, spoil_every)
    strs, centre_of, arms_of = [], [None] * n_gadgets, [None] * n_gadgets
    seqs = []
    for g, (p, number, spoiled) in enumerate(plan):
        centre = U.rand_seq(lens[g % len(lens)], r.randrange(1 << 30))
        seqs.append((centre,) + _arms(k, centre, p, r))
    for g0 in range(0, n_gadgets, GADGET_GROUP):
        group = range(g0, min(g0 + GADGET_GROUP, n_gadgets))
        for g in group:
            if len(seqs[g][0]) < 256:
                centre_of[g] = len(strs)
                strs.append(seqs[g][0])
        for g in group:
            p = plan[g][0]
            arms_of[g] = (list(range(len(strs), len(strs) + p)), list(range(len(strs) + p, len(strs) + 2 * p)))
            strs += seqs[g][1] + seqs[g][2]
        for g in group:
            if centre_of[g] is None:
                centre_of[g] = len(strs)
                strs.append(seqs[g][0])
    rows = [[] for _ in range(2 * len(strs))]
    pairs = []
    for g, (p, number, spoiled) in enumerate(plan):
        c, (ins, outs) = centre_of[g], arms_of[g]
        for i in range(p):                                       # way in i: ins[i] -> c; way out i: c -> outs[i]; each with its mirror
            rows[2 * ins[i]].append(2 * c)
            rows[2 * c + 1].append(2 * ins[i] + 1)
            rows[2 * c].append(2 * outs[i])
            rows[2 * outs[i] + 1].append(2 * c + 1)
        perm = nth_permutation(p, number)
        cell = {(a, perm[a]): (1 if spoiled == "unsupported" else r.randint(3, 5)) for a in range(p)}
        if spoiled == "ambiguous":
            a = r.randrange(p)
            cell[(a, r.choice([b for b in range(p) if b != perm[a]]))] = cell.pop((a, perm[a]))
        elif spoiled == "crossed":
            a = r.randrange(p)
            cell[(a, r.choice([b for b in range(p) if b != perm[a]]))] = 2
        pairs += [(c, 2 * ins[a], 2 * outs[b], count) for (a, b), count in cell.items()]
    return (k,) + _stored(strs, rows, pairs, 7800 + seed)


@functools.lru_cache(maxsize=None)
def ladder_case(n, k, seed=0):
    """centres c_0 ... c_{n - 1} cut from one random sequence, each with two ways in and two ways out: c_i goes on to c_{i + 1} and to a
    tip, c_{i + 1} is entered from c_i and from a tip (c_0 from two tips, c_{n - 1} goes on to two).  Through pairs centre with centre
    and tip with tip, so every centre is resolved and both ends of every edge between centres are renamed.  The order within a row
    is seeded; a seeded half is stored reverse-complemented -> (k, strs, rows, through)"""
    r = random.Random(7900 + seed * 977 + n * 31 + k)
    lens = [r.choice((k, k + 1, k + 3)) for _ in range(n)]
    text = U.rand_seq(sum(x - k + 1 for x in lens) + k - 1, r.randrange(1 << 30))
    strs, at, centres, tin, tout = [], 0, [], [], []
    for i in range(n):
        centre = text[at:at + lens[i]]
        at += lens[i] - k + 1
        ins, outs = _arms(k, centre, 2, r)
        centres.append(len(strs))
        strs.append(centre)
        tin.append([len(strs) + j for j in range(2 if i == 0 else 1)])
        strs += ins[:len(tin[-1])]
        tout.append([len(strs) + j for j in range(2 if i == n - 1 else 1)])
        strs += outs[:len(tout[-1])]
    rows = [[] for _ in range(2 * len(strs))]
    pairs = []

    def edge(a, b):
        for x, y in ((a, b), (b ^ 1, a ^ 1)):
            if r.random() < 0.5:
                rows[x].append(y)
            else:
                rows[x].insert(0, y)

    for i in range(n):
        c = centres[i]
        ways_in = ([2 * centres[i - 1]] if i else []) + [2 * u for u in tin[i]]
        ways_out = ([2 * centres[i + 1]] if i + 1 < n else []) + [2 * u for u in tout[i]]
        for p in ways_in[1:] if i else ways_in:                  # (the edge from the centre in front was made as its way out)
            edge(p, 2 * c)
        for q in ways_out:
            edge(2 * c, q)
        pairs += [(c, ways_in[0], ways_out[0], r.randint(2, 4)), (c, ways_in[1], ways_out[1], r.randint(2, 4))]
    return (k,) + _stored(strs, rows, pairs, 8000 + seed)


def records_for(strs, rows, k, seed):
    """unitig records and link hits for a case built by hand -> (recs as dicts, hits): seeded counts, n_pred and n_succ from the rows"""
    r = random.Random(seed)
    recs = []
    for u, s in enumerate(strs):
        m = len(s) - k + 1
        lo = r.randint(1, 9)
        hi = lo + r.randint(0, 40)
        recs.append({"n_kmers": m, "sum_count": r.randint(lo * m, hi * m) if m > 1 else lo, "min_count": lo, "max_count": hi if m > 1 else lo, "first_node": r.randrange(1 << 40), "circular": 0,
                     "n_pred": len(rows[2 * u + 1]), "n_succ": len(rows[2 * u]), "first_fwd": r.randrange(2)})
    return recs, [r.randint(1, 1 << 40) for _ in range(sum(map(len, rows)))]


def tile_starts(strs, marked=None, tile=4096):
    """per aligned 4096-byte window of the flat input (a tile of the emit kernels): (unitigs that start in it, those of them in `marked`)"""
    out, at = {}, 0
    for u, s in enumerate(strs):
        a = out.setdefault(at // tile, [0, 0])
        a[0] += 1
        a[1] += int(marked is not None and u in marked)
        at += len(s)
    return [tuple(out.get(i, (0, 0))) for i in range((at + tile - 1) // tile)]


def resolved_tsv(res):
    """unitigs.resolved.tsv of the driver: new unitig, origin, copy"""
    return "".join(f"u{i}\tu{u}\t{i - res['rplace'][u][0]}\n" for i, u in enumerate(res["origin"]))
