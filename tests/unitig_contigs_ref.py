"""The rule of kmx_unitig_contigs (include/kmx.h) restated in plain Python on top of unitig_walk_ref: the support of every edge
between unitigs, the kept edges, the chain links, the contigs with their steps, places and records, and the contig graph.  With
flat(), the check of the rule's consequences, the cases the tests share (those of the walks, ring2tips and the cut cases) and the
text the facade and the driver must write; chain_case: the cut cases at chosen lengths, depths and forks, for tests/test_gpu_unitig_scale.py.
Not a test."""
import functools
import hashlib
import random

import numpy as np

import unitig_clean_ref as UC
import unitig_links_ref as L
import unitig_map_ref as R
import unitig_walk_ref as W
import unitigs_ref as U

CONTIG_FIELDS = (("n_kmers", "<u8"), ("sum_count", "<u8"), ("min_count", "<u4"), ("max_count", "<u4"), ("first_step", "<u8"), ("n_steps", "<u4"),
                 ("circular", "u1"), ("n_pred", "u1"), ("n_succ", "u1"), ("reserved", "u1"), ("min_support", "<u8"), ("sum_support", "<u8"), ("reserved2", "<u8"))
CONTIG_DTYPE = np.dtype(list(CONTIG_FIELDS))
CONTIG_PLACE_DTYPE = np.dtype([("oc", "<u4"), ("off", "<u4")])
STAT_FIELDS = ("n_links", "n_kept", "n_below_min", "n_below_ratio", "n_chain", "n_contigs", "n_circular", "n_multi")
PARTS = ("cseq", "coffsets", "crec", "steps", "place", "clink_offsets", "clinks", "csupport", "stats", "counts")
PARAMS = ((0, 0), (1, 0), (2, 0), (2, 4), (3, 8))            # (min_reads, ratio) every case runs at
M64 = (1 << 64) - 1


def offsets_of(rows):
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    return loff


def mirror_index(rows, loff, a, j):
    """the index of mir(e) for e = entry j of out[a]"""
    b = rows[a][j]
    return loff[b ^ 1] + rows[b ^ 1].index(a ^ 1)


def support(rows, hits):
    loff = offsets_of(rows)
    sup = [0] * loff[-1]
    for a, row in enumerate(rows):
        for j in range(len(row)):
            e, me = loff[a] + j, mirror_index(rows, loff, a, j)
            sup[e] = (hits[e] + (hits[me] if me != e else 0)) & M64
    return sup


def contigs(k, strs, recs, rows, hits, min_reads, ratio):
    """-> a dict: the contigs (strings, records as dicts, steps, places), the contig graph as rows of (target, support), the stats"""
    n_u = len(strs)
    mu = [len(s) - k + 1 for s in strs]
    loff = offsets_of(rows)
    sup = support(rows, hits)
    best = [max((sup[loff[o] + j] for j in range(len(rows[o]))), default=0) for o in range(2 * n_u)]
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["n_links"] = loff[-1]
    out_k = [[] for _ in range(2 * n_u)]                        # (target, support), in row order
    for a, row in enumerate(rows):
        for j, b in enumerate(row):
            s = sup[loff[a] + j]
            if s < min_reads:
                st["n_below_min"] += 1
            elif ratio > 0 and (s * ratio < best[a] or s * ratio < best[b ^ 1]):
                st["n_below_ratio"] += 1
            else:
                st["n_kept"] += 1
                out_k[a].append((b, s))
    nxt = [None] * (2 * n_u)                                    # the chain link out of o: (t, support)
    prv = [None] * (2 * n_u)
    for o in range(2 * n_u):
        if len(out_k[o]) == 1:
            t, s = out_k[o][0]
            if t != o ^ 1 and len(out_k[t ^ 1]) == 1:
                assert out_k[t ^ 1][0][0] == o ^ 1, "kept is not symmetric under mir"
                nxt[o], prv[t] = (t, s), o
                st["n_chain"] += 1
    found, seen = [], set()
    for u in range(n_u):
        if u in seen:
            continue
        x, circular = 2 * u, False
        while prv[x] is not None:                               # back to the first step, or once round
            x = prv[x]
            if x == 2 * u:
                circular = True
                break
        if circular:
            members = [2 * u]
            while nxt[members[-1]][0] != 2 * u:
                members.append(nxt[members[-1]][0])
            start = 2 * min(o >> 1 for o in members)            # on this cycle or on its mirror: the representative starts there
            rep = [start]
            while nxt[rep[-1]][0] != start:
                rep.append(nxt[rep[-1]][0])
        else:
            path = [x]
            while nxt[path[-1]] is not None:
                path.append(nxt[path[-1]][0])
            mirror = [o ^ 1 for o in reversed(path)]
            rep = [2 * u] if len(path) == 1 else (path if path[0] >> 1 < mirror[0] >> 1 else mirror)
        for o in rep:
            assert o >> 1 not in seen, "a component holds both orientations of a unitig"
            seen.add(o >> 1)
        found.append((rep, circular))
    found.sort(key=lambda t: t[0][0] >> 1)
    cstrs, crecs, steps, place = [], [], [], [None] * n_u
    for c, (rep, circular) in enumerate(found):
        sups = [nxt[o][1] for o in rep if nxt[o] is not None]   # a cycle's closing link is the link out of its last step
        off = 0
        for o in rep:
            place[o >> 1] = (2 * c + (o & 1), off & 0xFFFFFFFF)
            off += mu[o >> 1]
        cs = [recs[o >> 1] for o in rep] if recs is not None else None
        crecs.append({"n_kmers": off, "sum_count": sum(r["sum_count"] for r in cs) if cs else 0, "min_count": min(r["min_count"] for r in cs) if cs else 0,
                      "max_count": max(r["max_count"] for r in cs) if cs else 0, "first_step": len(steps), "n_steps": len(rep), "circular": int(circular),
                      "n_pred": len(out_k[rep[0] ^ 1]), "n_succ": len(out_k[rep[-1]]), "reserved": 0, "min_support": min(sups) if sups else 0,
                      "sum_support": sum(sups) & M64, "reserved2": 0})
        cstrs.append(W.spell(strs, rep, k))
        steps += rep
        st["n_circular"] += int(circular)
        st["n_multi"] += int(len(rep) > 1)
    st["n_contigs"] = len(found)
    crows = []
    for c, (rep, circular) in enumerate(found):
        for last in (rep[-1], rep[0] ^ 1):
            row = []
            for t, s in out_k[last]:
                oc = place[t >> 1][0] ^ (t & 1)
                first = found[oc >> 1][0][0] if not oc & 1 else found[oc >> 1][0][-1] ^ 1
                assert first == t, "a kept edge that is no chain link enters a step that is not the first of its oriented contig"
                row.append((oc, s))
            crows.append(row)
    return {"cstrs": cstrs, "crecs": crecs, "steps": steps, "place": place, "crows": crows, "stats": st}


def flat(res):
    """what the library returns: (uint8 cseq, uint64 coffsets [C + 1], CONTIG_DTYPE [C], uint32 steps [U], CONTIG_PLACE_DTYPE [U],
    uint64 clink_offsets [2 C + 1], uint32 clinks, uint64 csupport, uint64 [8] stats, uint64 [3] n_contigs, n_cbases, n_clinks)"""
    buf, off = R.join(res["cstrs"])
    rec = np.zeros(len(res["crecs"]), dtype=CONTIG_DTYPE)
    for i, g in enumerate(res["crecs"]):
        for f, v in g.items():
            rec[f][i] = v
    place = np.array(res["place"], dtype=np.uint32).reshape(-1, 2).copy().view(CONTIG_PLACE_DTYPE).reshape(-1)
    cl_off = np.array(offsets_of(res["crows"]), dtype=np.uint64)
    cl = np.array([t for row in res["crows"] for t, _ in row], dtype=np.uint32)
    cs = np.array([s for row in res["crows"] for _, s in row], dtype=np.uint64)
    st = np.array([res["stats"][f] for f in STAT_FIELDS], dtype=np.uint64)
    return (buf, off, rec, np.array(res["steps"], dtype=np.uint32), place, cl_off, cl, cs, st, np.array([len(rec), len(buf), len(cl)], dtype=np.uint64))


def digest(res) -> str:
    h = hashlib.sha256()
    for part in flat(res):
        h.update(np.ascontiguousarray(part).tobytes())
    return h.hexdigest()


def check(k, strs, recs, rows, res, noop=False, overlaps_hold=True, node_graph=True):
    """consequences (a), (b) and (d) and what a record promises, asserted on an output (of the restatement or of the library)"""
    n_u = len(strs)
    mu = [len(s) - k + 1 for s in strs]
    cstrs, crecs, steps, place, st = res["cstrs"], res["crecs"], res["steps"], res["place"], res["stats"]
    assert st["n_contigs"] == len(cstrs) == len(crecs) and st["n_links"] == st["n_kept"] + st["n_below_min"] + st["n_below_ratio"] == sum(map(len, rows))
    assert len(steps) == n_u == sum(r["n_steps"] for r in crecs) and sorted(o >> 1 for o in steps) == list(range(n_u)), "consequence (d): every unitig lies in one contig, once"
    assert sum(r["n_kmers"] for r in crecs) == sum(mu) and sum(map(len, cstrs)) == sum(mu) + len(cstrs) * (k - 1), "consequence (d)"
    assert st["n_multi"] == sum(r["n_steps"] > 1 for r in crecs) and st["n_circular"] == sum(r["circular"] for r in crecs)
    assert st["n_chain"] == 2 * sum(r["n_steps"] - 1 + r["circular"] for r in crecs), "chain links come in mirror pairs, n_steps - 1 per path and one more per cycle"
    at, firsts = 0, []
    for c, (s, r) in enumerate(zip(cstrs, crecs)):
        mine = steps[r["first_step"]:r["first_step"] + r["n_steps"]]
        assert r["first_step"] == at and r["n_steps"] >= 1
        at += r["n_steps"]
        firsts.append(mine[0] >> 1)
        assert s == W.spell(strs, mine, k) and len(s) == r["n_kmers"] + k - 1
        off = 0
        for o in mine:
            assert place[o >> 1] == (2 * c + (o & 1), off & 0xFFFFFFFF), "consequence (d): place inverts steps"
            off += mu[o >> 1]
        assert off == r["n_kmers"]
        if r["circular"]:
            assert mine[0] == 2 * min(o >> 1 for o in mine) and r["n_pred"] == r["n_succ"] == 1
        elif len(mine) > 1:
            assert mine[0] >> 1 < mine[-1] >> 1, "the representative is the orientation whose first step has the smaller unitig"
        else:
            assert mine[0] & 1 == 0
        if recs is not None:
            cs = [recs[o >> 1] for o in mine]
            assert (r["sum_count"], r["min_count"], r["max_count"]) == (sum(x["sum_count"] for x in cs), min(x["min_count"] for x in cs), max(x["max_count"] for x in cs))
        else:
            assert (r["sum_count"], r["min_count"], r["max_count"]) == (0, 0, 0)
        if r["n_steps"] == 1 and not r["circular"]:
            assert r["min_support"] == r["sum_support"] == 0
    assert firsts == sorted(firsts), "contigs come in ascending unitig index of the first step"
    crows = res["crows"]
    assert len(crows) == 2 * len(cstrs) and sum(map(len, crows)) == st["n_kept"] - st["n_chain"] + 2 * st["n_circular"]
    for oc, row in enumerate(crows):
        assert len(row) == (crecs[oc >> 1]["n_pred"] if oc & 1 else crecs[oc >> 1]["n_succ"]) <= 4
        for t, s in row:
            assert (oc ^ 1, s) in crows[t ^ 1], "the contig graph is symmetric under mir, support included"
            if overlaps_hold:
                a = cstrs[oc >> 1] if not oc & 1 else U.rc(cstrs[oc >> 1])
                b = cstrs[t >> 1] if not t & 1 else U.rc(cstrs[t >> 1])
                assert a[len(a) - (k - 1):] == b[:k - 1]
        if crecs[oc >> 1]["circular"]:
            assert [t for t, _ in row] == [oc]
    if overlaps_hold and node_graph:                            # consequence (b): a contig is a path of the node graph
        win_u = {U.canon(s[j:j + k]) for s in strs for j in range(len(s) - k + 1)}
        win_c = [U.canon(s[j:j + k]) for s in cstrs for j in range(len(s) - k + 1)]
        assert len(win_c) == len(set(win_c)) == len(win_u) and set(win_c) == win_u, "consequence (b)"
    if noop:                                                    # consequence (a)
        assert cstrs == list(strs) and steps == [2 * u for u in range(n_u)] and [[t for t, _ in row] for row in crows] == [list(r) for r in rows]
        assert st["n_kept"] == st["n_links"] and st["n_multi"] == 0
        # an isolated unitig whose only edge is its self-loop o -> o (a homopolymer run that nothing else touches) is no circular
        # unitig, since a self-loop of the node graph is never a link, but it is a cycle of one step here
        loops = [u for u in range(n_u) if list(rows[2 * u]) == [2 * u] and list(rows[2 * u + 1]) == [2 * u + 1]]
        assert st["n_chain"] == 2 * len(loops) == 2 * st["n_circular"]
        if recs is not None:
            assert all(recs[u]["circular"] or recs[u]["n_kmers"] == 1 for u in loops) and all(u in loops for u in range(n_u) if recs[u]["circular"])
            for u, (r, q) in enumerate(zip(crecs, recs)):
                assert all(r[f] == q[f] for f in ("n_kmers", "sum_count", "min_count", "max_count", "n_pred", "n_succ")) and r["circular"] == int(u in loops)


def rc_spelled(strs, steps, k):
    """the steps' strings spelled with an explicit reverse complement per step, independent of unitig_map_ref.oriented"""
    out = ""
    for i, o in enumerate(steps):
        s = strs[o >> 1]
        if o & 1:
            s = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in s[::-1])
        out += s if i == 0 else s[k - 1:]
    return out


def paths_tsv(res):
    """contigs.paths.tsv of the driver: contig, step, unitig, strand, offset"""
    out = []
    for c, r in enumerate(res["crecs"]):
        for i, o in enumerate(res["steps"][r["first_step"]:r["first_step"] + r["n_steps"]]):
            out.append(f"c{c}\t{i}\tu{o >> 1}\t{'-' if o & 1 else '+'}\t{res['place'][o >> 1][1]}\n")
    return "".join(out)


def fasta(res):
    return "".join(f">c{c} n_kmers={r['n_kmers']} n_steps={r['n_steps']} circular={r['circular']}\n{s}\n" for c, (s, r) in enumerate(zip(res["cstrs"], res["crecs"])))


def gfa(res, k, strs=None, recs=None):
    """the GFA 1 text of KModel::write_contigs_gfa: an edge a -> b is written iff (a, b) <= (b ^ 1, a ^ 1) as pairs; with the unitig
    strings, their segments and one P line per contig"""
    out = ["H\tVN:Z:1.0\n"]
    if strs is not None:
        for u, s in enumerate(strs):
            out.append(f"S\tu{u}\t{s}\tLN:i:{len(s)}\tKC:i:{recs[u]['sum_count'] if recs is not None else 0}\n")
    for c, (s, r) in enumerate(zip(res["cstrs"], res["crecs"])):
        out.append(f"S\tc{c}\t{s}\tLN:i:{len(s)}\tKC:i:{r['sum_count']}\n")
    for a, row in enumerate(res["crows"]):
        for b, s in row:
            if (a, b) <= (b ^ 1, a ^ 1):
                out.append(f"L\tc{a >> 1}\t{'-' if a & 1 else '+'}\tc{b >> 1}\t{'-' if b & 1 else '+'}\t{k - 1}M\tRC:i:{s}\n")
    if strs is not None:
        for c, r in enumerate(res["crecs"]):
            mine = res["steps"][r["first_step"]:r["first_step"] + r["n_steps"]]
            out.append(f"P\tc{c}\t{','.join(f'u{o >> 1}' + ('-' if o & 1 else '+') for o in mine)}\t{','.join([f'{k - 1}M'] * (len(mine) - 1)) or '*'}\n")
    return "".join(out)


# ---- the cases: name -> (k, strs, recs, rows, {hits name: hits}); computed once, the caller must not change them
RING = "ring2tips"
CUT_N = (1, 2, 3, 4, 7, 8, 16, 17, 64, 1000)
CUT_K = (5, 31, 63)


def _ring2tips():
    """k = 21: a 300-base circular sequence, two 60-base tips that share 20 bases with it at two places, 40 reads of 100 bases round
    the ring in alternating strands, and the two tips as reads -> (k, km, cnt, reads)"""
    k = 21
    ring = U.rand_seq(300, 901)
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]       # a tip leaves the ring at once: its first own base is not the ring's
    tips = [ring[50:70] + other(ring[70]) + U.rand_seq(39, 902), U.rand_seq(39, 903) + other(ring[199]) + ring[200:220]]
    twice = ring + ring
    reads = []
    for i in range(40):
        a = (i * 37) % 300
        r = twice[a:a + 100]
        reads.append(r if i % 2 == 0 else U.rc(r))
    reads += tips
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    return k, km, cnt, reads


@functools.lru_cache(maxsize=None)
def listed_case(name):
    """a case with a listing -> (k, km, cnt, thr, strs, recs, reads, rows)"""
    if name == RING:
        k, km, cnt, reads = _ring2tips()
        thr = 1
        strs, recs = U.unitigs(km, cnt, k, thr)
        rows = L.links(km, cnt, k, thr, strs)
        return k, km, cnt, thr, strs, recs, reads, rows
    k, km, cnt, thr, strs, reads, rows = W.case(name)
    if name == "k21_noisy_clean":
        res = UC.clean(km, cnt, k, thr)
        recs = res["recs"]
    else:
        s2, recs = U.unitigs(km, cnt, k, thr)
        assert s2 == strs
    return k, km, cnt, thr, strs, recs, reads, rows


LISTED_CASES = list(W.WALK_CASES) + [RING]


@functools.lru_cache(maxsize=None)
def hits_of(name, which):
    """link_hits of a listed case: "exact" = walked at (0, 0), "bridged" = walked at (k, 1)"""
    k, km, cnt, thr, strs, recs, reads, rows = listed_case(name)
    gap, indel = (0, 0) if which == "exact" else (k, 1)
    if name == RING:
        segs, so, _, _ = R.map_reads(km, k, strs, reads)
        return tuple(W.walk_segs(k, strs, segs, so, rows, gap, indel)[3])
    return tuple(W.walked(name, gap, indel)[3])


def mirrored_hits(rows, hits):
    """every edge's hits on its mirror instead"""
    loff = offsets_of(rows)
    out = [0] * len(hits)
    for a, row in enumerate(rows):
        for j in range(len(row)):
            out[mirror_index(rows, loff, a, j)] = hits[loff[a] + j]
    return out


@functools.lru_cache(maxsize=None)
def cut_case(n, k, ring):
    """a random sequence (ring: a circular one) cut into n unitigs that overlap by k - 1, those of a seeded random half
    reverse-complemented, the CSR by hand with one hit per edge -> (k, strs, rows, hits, sequence)"""
    r = random.Random(n * 1000 + k * 2 + int(ring))
    lens = [r.choice((k, k + 1, 2 * k, 5000)) for _ in range(n)]
    ms = [x - k + 1 for x in lens]
    total = sum(ms)
    seq = U.rand_seq(total, 7000 + n * 64 + k + int(ring)) if ring else U.rand_seq(total + k - 1, 7000 + n * 64 + k)
    text = (seq * (2 + k // total))[:total + k - 1] if ring else seq     # a ring shorter than k - 1 goes round more than once
    flip = set(r.sample(range(n), n // 2))
    strs, at = [], 0
    for u in range(n):
        s = text[at:at + lens[u]]
        strs.append(U.rc(s) if u in flip else s)
        at += ms[u]
    rows = [[] for _ in range(2 * n)]
    fwd = [2 * u + (1 if u in flip else 0) for u in range(n)]    # the orientation that reads along the sequence
    for u in range(n if ring else n - 1):
        a, b = fwd[u], fwd[(u + 1) % n]
        rows[a].append(b)
        if (b ^ 1, a ^ 1) != (a, b):
            rows[b ^ 1].append(a ^ 1)
    hits = [1] * sum(map(len, rows))
    return k, strs, rows, hits, text


def cut_expected(n, k, ring):
    """the one contig of a cut case, as the rule's representative decides: a line starts at unitig 0 and reads along the sequence;
    a ring starts at unitig 0 as it is stored, so where that one was reverse-complemented the contig is the reverse complement of
    the ring read from unitig 1 on"""
    k, strs, rows, hits, text = cut_case(n, k, ring)
    if not ring or strs[0] == text[:len(strs[0])]:
        return text
    m0, total = len(strs[0]) - k + 1, len(text) - k + 1
    return U.rc((text[:total] * (3 + k // total))[m0:m0 + total + k - 1])


@functools.lru_cache(maxsize=None)
def chain_case(n, k, lens, ring, fork_every=0, seed=0):
    """cut_case with the lengths given: unitig u < n has lens[u % len(lens)] bytes, so a tile of the flat input holds as many starts
    as the lengths allow (4096 / 5 at k = 5) and n decides the depth of the doubling.  With fork_every = m > 0 the junction behind
    every m-th unitig (behind unitigs m - 1, 2 m - 1, ...) gets a second successor, a tip of k bytes stored behind the n chain
    unitigs, with its mirror edge: the chain breaks there and both edges stay in the contig graph
    -> (k, strs, rows, hits, sequence); strs holds the n chain unitigs, then the tips"""
    r = random.Random(seed * 1000003 + n * 1000 + k * 2 + int(ring))
    ul = [lens[u % len(lens)] for u in range(n)]
    assert min(ul) >= k
    ms = [x - k + 1 for x in ul]
    total = sum(ms)
    seq = U.rand_seq(total if ring else total + k - 1, 8000 + seed * 131 + n * 64 + k + int(ring))
    text = (seq * (2 + k // total))[:total + k - 1] if ring else seq
    flip = set(r.sample(range(n), n // 2))
    strs, at, ends = [], 0, []
    for u in range(n):
        s = text[at:at + ul[u]]
        strs.append(U.rc(s) if u in flip else s)
        at += ms[u]
        ends.append(at)                                          # the next unitig along the sequence starts here
    fwd = [2 * u + (1 if u in flip else 0) for u in range(n)]    # the orientation that reads along the sequence
    forks = [j for j in range(n if ring else n - 1) if fork_every and (j + 1) % fork_every == 0]
    rows = [[] for _ in range(2 * (n + len(forks)))]
    for u in range(n if ring else n - 1):
        a, b = fwd[u], fwd[(u + 1) % n]
        rows[a].append(b)
        if (b ^ 1, a ^ 1) != (a, b):
            rows[b ^ 1].append(a ^ 1)
    for i, j in enumerate(forks):                                # the tip: the k - 1 bytes both successors share, then a base the sequence does not go on with
        e = ends[j]
        follows = text[e + k - 1] if e + k - 1 < len(text) else text[e + k - 1 - total]      # (a ring goes on at its start)
        tip = text[e:e + k - 1] + "ACGT"[("ACGT".index(follows) + 1 + r.randrange(3)) % 4]
        back = r.random() < 0.5
        strs.append(U.rc(tip) if back else tip)
        t = 2 * (n + i) + int(back)
        if r.random() < 0.5:
            rows[fwd[j]].append(t)
        else:
            rows[fwd[j]].insert(0, t)
        rows[t ^ 1].append(fwd[j] ^ 1)
    hits = [1] * sum(map(len, rows))
    return k, strs, rows, hits, text


def chain_expected(n, k, lens, ring, seed=0):
    """the one contig of a chain case without forks, by cut_expected's closed form"""
    k, strs, rows, hits, text = chain_case(n, k, lens, ring, 0, seed)
    if not ring or strs[0] == text[:len(strs[0])]:
        return text
    m0, total = len(strs[0]) - k + 1, len(text) - k + 1
    return U.rc((text[:total] * (3 + k // total))[m0:m0 + total + k - 1])


def fork_counts(n, m, ring):
    """what a chain case with fork_every = m >= 2 must give, by arithmetic: F junctions fork (those behind unitigs m - 1, 2 m - 1, ...;
    a line has n - 1 junctions, a ring n).  Every fork ends a piece of the chain and adds a tip, so a line falls into F + 1 pieces and
    a ring into F (F >= 1), each a contig, beside F tips.  Every piece holds m unitigs or more, but a line's last one, which holds
    n - F m >= 1.  At a fork two edges and their two mirrors are kept and are no chain links: 4 F edges of the contig graph
    -> (n_contigs, n_multi, contig-graph edges)"""
    assert m >= 2
    f = n // m if ring else (n - 1) // m
    assert f >= 1
    if ring:
        return 2 * f, f, 4 * f
    return 2 * f + 1, f + int(n - f * m > 1), 4 * f


@functools.lru_cache(maxsize=None)
def want_chain(n, k, lens, ring, fork_every=0, seed=0):
    k, strs, rows, hits, text = chain_case(n, k, lens, ring, fork_every, seed)
    return contigs(k, strs, None, rows, hits, 1, 0)


@functools.lru_cache(maxsize=None)
def want(name, which, min_reads, ratio):
    k, km, cnt, thr, strs, recs, reads, rows = listed_case(name)
    return contigs(k, strs, recs, rows, list(hits_of(name, which)), min_reads, ratio)


@functools.lru_cache(maxsize=None)
def want_cut(n, k, ring):
    k, strs, rows, hits, text = cut_case(n, k, ring)
    return contigs(k, strs, None, rows, hits, 1, 0)
