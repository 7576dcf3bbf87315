"""Writes unitig_contigs_golden.json: digests of the output of the plain-Python restatement (tests/unitig_contigs_ref.py) on its
cases, with the counts that say what a case is.  Run from the repository root: python tests/golden/make_unitig_contigs_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import unitig_contigs_ref as G  # noqa: E402


def listed(name):
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    out = {"k": k, "n_unitigs": len(strs), "n_links": sum(map(len, rows)), "hits": {w: sum(G.hits_of(name, w)) for w in ("exact", "bridged")}}
    for which in ("exact", "bridged"):
        for pair in G.PARAMS:
            res = G.want(name, which, *pair)
            out[f"{which} {pair[0]},{pair[1]}"] = [res["stats"][f] for f in G.STAT_FIELDS] + [G.digest(res)]
    return out


def cut(n, k, ring):
    res = G.want_cut(n, k, ring)
    return [len(res["cstrs"][0]), sum(o & 1 for o in res["steps"]), G.digest(res)]


if __name__ == "__main__":
    out = {"listed": {name: listed(name) for name in G.LISTED_CASES},
           "cut": {f"{'ring' if ring else 'line'} k{k} n{n}": cut(n, k, ring) for ring in (False, True) for k in G.CUT_K for n in G.CUT_N}}
    with open(os.path.join(HERE, "unitig_contigs_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
