#!/usr/bin/env python3
"""Generate tests/golden/unitig_clean_golden.json: what kmx_unitig_graph_clean must return (ops = 7, caps 2 k, 16 rounds) for the
cases of tests/unitigs_ref.py (CASES: pinned by seed; thr raised to 1 where a case has 0; the reads also at thr = 2) and for the
hand-built shapes of tests/unitig_clean_ref.py, computed by that restatement alone.  Per case: the statistics, the per-round
log, unitigs and N50 before and after, and the sha256 of the six flat outputs.  Data only."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unitig_clean_ref as CL  # noqa: E402
import unitigs_ref as U  # noqa: E402

PARTS = ("bases", "offsets", "records", "link_offsets", "links", "removed")


def listing(name):
    c = U.CASES[name]()
    if len(c) == 3:
        k, thr, seqs = c
        km, cnt = U.listing_of(U.count_kmers(seqs, k))
    else:
        k, thr, km, cnt = c
    return k, max(thr, 1), km, cnt


def entry(k, thr, km, cnt, res):
    strs0, _ = U.unitigs(km, cnt, k, thr)
    return {"k": k, "thr": thr, "stats": res["stats"], "log": res["log"], "unitigs_before": len(strs0), "n50_before": CL.n50(strs0),
            "unitigs_after": len(res["strs"]), "n50_after": CL.n50(res["strs"]),
            **{p + "_sha256": hashlib.sha256(a.tobytes()).hexdigest() for p, a in zip(PARTS, CL.flat(res))}}


def names():
    """golden key -> (case of U.CASES, thr or None) or (case of CLEAN_CASES, "crafted")"""
    out = {name: (name, None) for name in U.CASES}
    out["reads_thr1_at_thr2"] = ("reads_thr1", 2)
    out.update({"crafted_" + name: (name, "crafted") for name in CL.CLEAN_CASES})
    return out


def compute(key):
    """-> (k, thr, k-mers, counts, params, result) for a golden key"""
    name, how = names()[key]
    if how == "crafted":
        return CL.clean_case(name)
    k, thr, km, cnt = listing(name)
    thr = thr if how is None else how
    p = CL.params_of(k, None)
    return k, thr, km, cnt, p, CL.clean(km, cnt, k, thr, *p)


def main():
    cases = {}
    for key in names():
        k, thr, km, cnt, _, res = compute(key)
        cases[key] = entry(k, thr, km, cnt, res)
    out = {"generator": "tests/golden/make_unitig_clean_golden.py", "cases": cases}
    with open(os.path.join(HERE, "unitig_clean_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: [v["unitigs_before"], v["unitigs_after"], v["stats"]["rounds_run"]] for k, v in cases.items()}), flush=True)


if __name__ == "__main__":
    main()
