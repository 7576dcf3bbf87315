#!/usr/bin/env python3
"""Generate tests/golden/unitigs_golden.json: what kmx_unitigs must return for the cases of tests/unitigs_ref.py (CASES: pinned
by seed), computed by that restatement of the rule alone.  Per case: k, thr, the tallies, and the sha256 of the listing and of
the flat output (bases, offsets, records); the small cases also carry their k-mers, counts, strings and records in full.
Data only."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unitigs_ref as U  # noqa: E402

FULL_BELOW = 500                                                # listing entries


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def entry(name):
    import numpy as np
    k, thr, km, cnt, strs, recs = U.case(name)
    buf, off, rec = U.flat(strs, recs)
    e = {"k": k, "thr": thr, "n": len(km), "nodes": sum(c >= thr for c in cnt), "unitigs": len(strs), "bases": int(off[-1]),
         "longest": max(r["n_kmers"] for r in recs), "circular": sum(r["circular"] for r in recs),
         "listing_sha256": sha(np.ascontiguousarray(U.pack(km, k), dtype="<u8"), np.asarray(cnt, dtype="<u4")),
         "bases_sha256": sha(buf), "offsets_sha256": sha(off), "records_sha256": sha(rec)}
    if len(km) < FULL_BELOW:
        e.update({"kmers": km, "counts": cnt, "strings": strs, "records": recs})
    return e


def main():
    out = {"generator": "tests/golden/make_unitigs_golden.py", "cases": {name: entry(name) for name in U.CASES}}
    with open(os.path.join(HERE, "unitigs_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: [v["n"], v["unitigs"], v["longest"], v["circular"]] for k, v in out["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
