"""Writes tests/golden/unitig_resolve_golden.json from the restatement (tests/unitig_resolve_ref.py): run it from the repository root
with tests/ on the path, and only when the rule changes on purpose."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import unitig_contigs_ref as G      # noqa: E402
import unitig_resolve_ref as X      # noqa: E402


def entry(k, strs, recs, rows, hits, t):
    out = {"through": [sum(1 for x in t if x), sum(t), X.digest([X.np.array(t, dtype=X.np.uint64)])]}
    for p in X.PARAMS:
        res = X.resolve(k, strs, recs, rows, hits, list(t), *p)
        out[f"{p[0]},{p[1]}"] = [res["stats"][f] for f in X.RESOLVE_STAT_FIELDS] + [X.digest(X.flat(res))]
    return out


def main():
    doc = {"listed": {}, "planted": {}, "synthetic": {}}
    for name in G.LISTED_CASES:
        k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
        doc["listed"][name] = {which: entry(k, strs, recs, rows, list(G.hits_of(name, which)), X.listed_through(name, which)[0]) for which in X.WALK_PARAMS}
    for name in X.PLANTED:
        k, genome, km, cnt, strs, recs, reads, rows, hits, t = X.planted_case(name)
        doc["planted"][name] = entry(k, strs, recs, rows, hits, t)
    for name in X.SYNTH_CASES:
        k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
        doc["synthetic"][name] = entry(k, strs, recs, rows, None, X.synthetic_through(rows, len(strs), X.SYNTH_SEED))
    with open(os.path.join(HERE, "unitig_resolve_golden.json"), "w") as f:
        json.dump(doc, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
