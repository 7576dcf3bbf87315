"""A plain-Python restatement of the scaffold rule of include/kmx.h (kmx_unitig_scaffold): pair links -> kept edges -> chain
links -> scaffolds spelled with runs of N.  Sequential: it follows the links step by step, where the library ranks by pointer
doubling.  Shared by test_unitig_scaffold_cpu.py and test_gpu_unitig_scaffold.py."""
import functools
import random

import numpy as np

import unitig_pairs_ref as P
import unitigs_ref as U

SCAFFOLD_DTYPE = np.dtype([("n_bases", "<u8"), ("n_kmers", "<u8"), ("sum_count", "<u8"), ("min_count", "<u4"), ("max_count", "<u4"), ("first_step", "<u4"), ("n_steps", "<u4"),
                           ("n_gap_bases", "<u8"), ("min_pairs", "<u8"), ("sum_pairs", "<u8")])
STEP_DTYPE = np.dtype([("o", "<u4"), ("n_gap", "<u4"), ("est", "<i8")])
PLACE_DTYPE = np.dtype([("os", "<u4"), ("step", "<u4"), ("off", "<u8")])
CIRCULAR = 0x80000000
STAT_FIELDS = ("n_entries", "n_links", "n_ignored", "n_below_min", "n_below_ratio", "n_kept", "n_chain", "n_scaffolds", "n_circular", "n_multi")


def oriented(s, d):
    return U.rc(s) if d else s


def gap_of(k, entry, inner, min_n, max_n):
    """(est, n_gap) of a pair link, in wrapping signed 64-bit arithmetic"""
    a, b, n, sm, _, _ = entry
    est = (inner - 1 - sm // n - (k - 1)) & (2 ** 64 - 1)
    if est >= 2 ** 63:
        est -= 2 ** 64
    return est, min(max(est, min_n), max_n)


def scaffold(k, strs, recs, plinks, min_pairs, ratio, inner, min_n, max_n):
    """strs: the unitig strings; recs: None or (sum_count, min_count, max_count) per unitig; plinks: tuples (a, b, n_pairs,
    sum_dist, min_dist, max_dist) in list order -> a dict: sstrs, srecs (dicts with circular apart), steps [(o, n_gap, est)],
    place [(os, step, off)], stats"""
    nu = len(strs)
    islink = [a < 2 * nu and b < 2 * nu and a >> 1 != b >> 1 and n >= 1 for a, b, n, _, _, _ in plinks]
    best = [0] * (2 * nu)
    for e, ok in zip(plinks, islink):
        if ok:
            best[e[0]] = max(best[e[0]], e[2])
            best[e[1] ^ 1] = max(best[e[1] ^ 1], e[2])
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["n_entries"] = len(plinks)
    nk = [0] * (2 * nu)
    kept = []
    for i, (e, ok) in enumerate(zip(plinks, islink)):
        a, b, n = e[:3]
        if not ok:
            st["n_ignored"] += 1
            continue
        st["n_links"] += 1
        if n < min_pairs:
            st["n_below_min"] += 1
        elif ratio > 0 and (n * ratio < best[a] or n * ratio < best[b ^ 1]):
            st["n_below_ratio"] += 1
        else:
            st["n_kept"] += 1
            kept.append(i)
            nk[a] += 1
            nk[b ^ 1] += 1
    nxt, prv = {}, {}                                             # o -> (the next / the previous oriented unitig, the entry)
    for i in kept:
        a, b = plinks[i][:2]
        if nk[a] == 1 and nk[b ^ 1] == 1:
            st["n_chain"] += 1
            nxt[a], prv[b] = (b, i), (a, i)
            nxt[b ^ 1], prv[a ^ 1] = (a ^ 1, i), (b ^ 1, i)
    seen = [False] * nu
    found = []                                                    # (the steps, circular)
    for u in range(nu):
        if seen[u]:
            continue
        o, circular = 2 * u, False
        while o in prv:                                           # back to the head, or once round
            o = prv[o][0]
            if o == 2 * u:
                circular = True
                break
        path = [o]
        while path[-1] in nxt and nxt[path[-1]][0] != path[0]:
            path.append(nxt[path[-1]][0])
        if not circular and len(path) > 1 and (path[-1] >> 1) < (path[0] >> 1):
            path = [x ^ 1 for x in reversed(path)]               # the mirror starts at the smaller unitig
        for x in path:
            assert not seen[x >> 1]
            seen[x >> 1] = True
        found.append((path, circular))
    found.sort(key=lambda pc: pc[0][0] >> 1)
    sstrs, srecs, steps, place = [], [], [], [None] * nu
    for s, (path, circular) in enumerate(found):
        r = {"n_bases": 0, "n_kmers": 0, "sum_count": 0, "min_count": 0, "max_count": 0, "first_step": len(steps), "n_steps": len(path), "circular": int(circular), "n_gap_bases": 0,
             "min_pairs": 0, "sum_pairs": 0}
        parts, off, pairs = [], 0, []
        for j, o in enumerate(path):
            est = n_gap = 0
            if o in prv and (j > 0 or circular):
                entry = plinks[prv[o][1]]
                est, n_gap = gap_of(k, entry, inner, min_n, max_n)
                pairs.append(entry[2])
            if j > 0:
                parts.append("N" * n_gap)
                off += n_gap
                r["n_gap_bases"] += n_gap
            steps.append((o, n_gap, est))
            place[o >> 1] = (2 * s + (o & 1), j, off)
            parts.append(oriented(strs[o >> 1], o & 1))
            off += len(strs[o >> 1])
            r["n_kmers"] += len(strs[o >> 1]) - k + 1
        r["n_bases"] = off
        if pairs:
            r["min_pairs"], r["sum_pairs"] = min(pairs), sum(pairs) & (2 ** 64 - 1)
        if recs is not None:
            cs = [recs[o >> 1] for o in path]
            r["sum_count"], r["min_count"], r["max_count"] = sum(c[0] for c in cs) & (2 ** 64 - 1), min(c[1] for c in cs), max(c[2] for c in cs)
        sstrs.append("".join(parts))
        srecs.append(r)
    st["n_scaffolds"] = len(found)
    st["n_circular"] = sum(c for _, c in found)
    st["n_multi"] = sum(len(p) > 1 for p, _ in found)
    return {"sstrs": sstrs, "srecs": srecs, "steps": steps, "place": place, "stats": st}


def flat(res):
    """the result as the library lays it out -> (uint8 bases, uint64 soffsets, SCAFFOLD_DTYPE, STEP_DTYPE, PLACE_DTYPE, stats)"""
    sseq = np.frombuffer("".join(res["sstrs"]).encode(), dtype=np.uint8)
    soffs = np.cumsum([0] + [len(s) for s in res["sstrs"]], dtype=np.uint64).astype(np.uint64)
    srec = np.zeros(len(res["srecs"]), dtype=SCAFFOLD_DTYPE)
    for i, r in enumerate(res["srecs"]):
        for f in SCAFFOLD_DTYPE.names:
            srec[i][f] = r[f] | (CIRCULAR if r["circular"] else 0) if f == "n_steps" else r[f]
    steps = np.array(res["steps"], dtype=STEP_DTYPE) if res["steps"] else np.zeros(0, dtype=STEP_DTYPE)
    place = np.array(res["place"], dtype=PLACE_DTYPE) if res["place"] else np.zeros(0, dtype=PLACE_DTYPE)
    return sseq, soffs, srec, steps, place, res["stats"]


def check(k, strs, plinks, res, max_n):
    """consequence (c) and the sizes the header promises"""
    nu = len(strs)
    assert sum(r["n_steps"] for r in res["srecs"]) == nu == len(res["steps"])
    assert sorted(o >> 1 for o, _, _ in res["steps"]) == list(range(nu))
    nb = sum(map(len, strs))
    assert sum(r["n_bases"] for r in res["srecs"]) == nb + sum(r["n_gap_bases"] for r in res["srecs"]) == sum(map(len, res["sstrs"]))
    assert nu == 0 or sum(map(len, res["sstrs"])) <= nb + (nu - 1) * max_n
    for s, r in enumerate(res["srecs"]):
        assert res["sstrs"][s].count("N") == r["n_gap_bases"] and len(res["sstrs"][s]) == r["n_bases"]
        for j in range(r["n_steps"]):
            o, n_gap, est = res["steps"][r["first_step"] + j]
            os_, step, off = res["place"][o >> 1]
            assert (os_ >> 1, os_ & 1, step) == (s, o & 1, j)                                   # place inverts steps
            assert res["sstrs"][s][off:off + len(strs[o >> 1])] == oriented(strs[o >> 1], o & 1)
            assert j == 0 or res["sstrs"][s][off - n_gap:off] == "N" * n_gap
    firsts = [res["steps"][r["first_step"]][0] >> 1 for r in res["srecs"]]
    assert firsts == sorted(firsts)


def mirrored(entry):
    a, b = entry[:2]
    return (b ^ 1, a ^ 1) + tuple(entry[2:])


def plinks_array(plinks):
    return np.array(plinks, dtype=P.PAIR_LINK_DTYPE) if len(plinks) else np.zeros(0, dtype=P.PAIR_LINK_DTYPE)


# ---- the text files of the facade and the driver
def fasta(res):
    return "".join(f">s{s} n_bases={r['n_bases']} n_steps={r['n_steps']} n_gap_bases={r['n_gap_bases']} circular={r['circular']}\n{t}\n" for s, (t, r) in enumerate(zip(res["sstrs"], res["srecs"])))


def paths_tsv(res):
    """scaffolds.paths.tsv: scaffold, step, unitig, strand, base offset, the N in front, the estimate"""
    out = []
    for s, r in enumerate(res["srecs"]):
        for j in range(r["n_steps"]):
            o, n_gap, est = res["steps"][r["first_step"] + j]
            out.append(f"s{s}\t{j}\tu{o >> 1}\t{'-' if o & 1 else '+'}\t{res['place'][o >> 1][2]}\t{n_gap}\t{est}\n")
    return "".join(out)


def agp(res, strs):
    """scaffolds.agp, AGP 2.1: a W line per unitig, an N line per spelled gap (none for a gap of no base)"""
    out = ["##agp-version\t2.1\n"]
    for s, r in enumerate(res["srecs"]):
        part = 0
        for j in range(r["n_steps"]):
            o, n_gap, _ = res["steps"][r["first_step"] + j]
            off, ln = res["place"][o >> 1][2], len(strs[o >> 1])
            if j > 0 and n_gap > 0:
                part += 1
                out.append(f"s{s}\t{off - n_gap + 1}\t{off}\t{part}\tN\t{n_gap}\tscaffold\tyes\tpaired-ends\n")
            part += 1
            out.append(f"s{s}\t{off + 1}\t{off + ln}\t{part}\tW\tu{o >> 1}\t1\t{ln}\t{'-' if o & 1 else '+'}\n")
    return "".join(out)


# ---- cases
def two_islands():
    """the pair tests' case through the restatements -> (k, unitig strings, the pair list, the genome)"""
    k, km, cnt, strs, reads, rows, genome = P.case("two_islands")
    walks, wo, steps = P.walked("two_islands")
    mu = [len(s) - k + 1 for s in strs]
    out = P.pair_walks(k, mu, walks, wo, steps, rows, *P.READ_PARAMS)
    return k, strs, [tuple(int(x) for x in e) for e in out[1]], genome


TWO_ISLANDS_PARAMS = dict(min_pairs=2, ratio=0, inner=221, min_n=0, max_n=1000)


def random_list(n, seed, nu=P.CRAFT_U, max_pairs=40):
    """n distinct canonical keys over nu unitigs, strictly ascending, both orientations, small random counts and distances"""
    r = random.Random(seed)
    keys = set()
    while len(keys) < n:
        a, b = r.randrange(2 * nu), r.randrange(2 * nu)
        if a >> 1 != b >> 1:
            keys.add(P.canonical(a, b))
    out = []
    for a, b in sorted(keys):
        c = r.randrange(1, max_pairs)
        d = [r.randrange(0, 400) for _ in range(min(c, 3))]
        out.append((a, b, c, sum(d) + (c - len(d)) * d[0], min(d), max(d)))
    return out


def chain_list(order, flips, closed, n_pairs=5, dist=50, canonical=True):
    """the entries that chain the unitigs `order` in orientations `flips` into one path (closed: into one cycle), sorted"""
    steps = [2 * u + d for u, d in zip(order, flips)]
    out = []
    for i in range(len(steps) - (0 if closed else 1)):
        a, b = steps[i], steps[(i + 1) % len(steps)]
        a, b = P.canonical(a, b) if canonical else (a, b)
        out.append((a, b, n_pairs + i % 3, (n_pairs + i % 3) * (dist + i % 7), dist, dist + 6))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def deep_chain(n, k, closed, seed=5):
    """n unitigs of k + 2 bytes in shuffled order and random orientation, chained into one path or one cycle"""
    r = random.Random(seed)
    strs = [U.rand_seq(k + 2, 7000 + u) for u in range(n)] if n <= 5000 else _cheap_strs(n, k + 2, seed)
    order = list(range(n))
    r.shuffle(order)
    flips = [r.randrange(2) for _ in range(n)]
    return strs, chain_list(order, flips, closed)


def _cheap_strs(n, ln, seed):
    b = np.random.default_rng(seed).integers(0, 4, size=n * ln, dtype=np.uint8)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[b].tobytes().decode()
    return [s[i * ln:(i + 1) * ln] for i in range(n)]
