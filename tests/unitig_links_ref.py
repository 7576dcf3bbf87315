"""The rule of kmx_unitig_graph (include/kmx.h) restated in plain Python on top of unitigs_ref: the edges between oriented
unitigs from the unitigs' own strings, a dict from every oriented unitig's first k-mer to its number, then the four questions
per end.  With the checks of an output and the GFA text the facade must write.  Not a test."""
import numpy as np

import unitigs_ref as U


def oriented(strs):
    """[s_0, rc(s_0), s_1, rc(s_1), ...]: the string of o = 2 u + d at index o"""
    out = []
    for s in strs:
        out += [s, U.rc(s)]
    return out


def links(kmers, counts, k: int, thr: int, strs):
    """-> rows: rows[o] = the targets o' of the edges out of oriented unitig o, in the order of the appended base"""
    g = U.Graph(kmers, counts, k, thr)
    ori = oriented(strs)
    first = {}
    for o, s in enumerate(ori):
        assert s[:k] not in first, "two oriented unitigs start with the same k-mer"
        first[s[:k]] = o
    rows = []
    for s in ori:
        row = []
        for c in "ACGT":
            y = s[-k:][1:] + c
            if U.canon(y) in g.idx:
                row.append(first[y])                           # (a KeyError here: the rule's "o' always exists" is broken)
        rows.append(row)
    return rows


def flat_links(rows):
    """(uint64 link_offsets [2 U + 1], uint32 links): what the library returns for these rows"""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    return off, np.array([t for r in rows for t in r], dtype=np.uint32)


def rows_of(off, lk):
    off = [int(x) for x in off]
    lk = [int(x) for x in lk]
    return [lk[off[o]:off[o + 1]] for o in range(len(off) - 1)]


def check_links(kmers, counts, k: int, thr: int, strs, recs, off, lk):
    """every consequence the rule lists, asserted on an output (of the restatement or of the library)"""
    g = U.Graph(kmers, counts, k, thr)
    n_u = len(strs)
    assert len(off) == 2 * n_u + 1 and int(off[0]) == 0 and int(off[-1]) == len(lk)
    assert all(int(a) <= int(b) for a, b in zip(off, off[1:]))
    rows = rows_of(off, lk)
    ori = oriented(strs)
    total = 0
    edges = set()
    for u, r in enumerate(recs):
        assert len(rows[2 * u]) == r["n_succ"] and len(rows[2 * u + 1]) == r["n_pred"], "out-degrees are not the record's"
        total += r["n_pred"] + r["n_succ"]
    assert len(lk) == total, "n_links is not the sum of the degrees"
    for a, row in enumerate(rows):
        want = [ori[a][-k:][1:] + c for c in "ACGT" if U.canon(ori[a][-k:][1:] + c) in g.idx]
        assert len(row) == len(want)
        for b, y in zip(row, want):                            # the order of c, the target's first k-mer, the k - 1 overlap
            assert 0 <= b < 2 * n_u and ori[b][:k] == y
            assert ori[a][-(k - 1):] == ori[b][:k - 1]
            assert (a, b) not in edges, "an edge twice"
            edges.add((a, b))
    for a, b in edges:
        assert (b ^ 1, a ^ 1) in edges, "the mirror edge is missing"
    for u, r in enumerate(recs):
        if r["circular"]:
            assert rows[2 * u] == [2 * u] and rows[2 * u + 1] == [2 * u + 1]
    # the oriented edges of the node graph are exactly the links inside unitigs plus these edges
    inside = set()
    for s in ori:
        ks = [s[p:p + k] for p in range(len(s) - k + 1)]
        inside.update(zip(ks, ks[1:]))
    between = {(ori[a][-k:], ori[b][:k]) for a, b in edges}
    assert len(between) == len(edges) and not (inside & between)
    node_edges = {(x, y) for z in g.idx for x in (z, U.rc(z)) for y in g.succ(x)}
    assert inside | between == node_edges, "the edges of the node graph are not the links inside unitigs plus the reported ones"


def gfa(strs, recs, off, lk, k: int) -> str:
    """the GFA 1 text of KModel::write_unitigs_gfa: an edge a -> b is written iff (a, b) <= (b ^ 1, a ^ 1) as pairs"""
    out = ["H\tVN:Z:1.0\n"]
    for u, (s, r) in enumerate(zip(strs, recs)):
        out.append(f"S\tu{u}\t{s}\tLN:i:{len(s)}\tKC:i:{int(r['sum_count'])}\n")
    for a, row in enumerate(rows_of(off, lk)):
        for b in row:
            if (a, b) <= (b ^ 1, a ^ 1):
                out.append(f"L\tu{a >> 1}\t{'-' if a & 1 else '+'}\tu{b >> 1}\t{'-' if b & 1 else '+'}\t{k - 1}M\n")
    return "".join(out)


def case_links(name):
    """-> (k, thr, k-mers, counts, strs, recs, link_offsets, links) of the restatement for a case of unitigs_ref.CASES"""
    k, thr, km, cnt, strs, recs = U.case(name)
    off, lk = flat_links(links(km, cnt, k, thr, strs))
    return k, thr, km, cnt, strs, recs, off, lk
