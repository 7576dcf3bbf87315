"""Writes unitig_map_golden.json: the output of the plain-Python restatement (tests/unitig_map_ref.py) on its cases.
Run from the repository root: python tests/golden/make_unitig_map_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import unitig_map_ref as R  # noqa: E402


def record(name):
    k, km, cnt, thr, strs, reads = R.case(name)
    segs, so, recs, hits = R.map_reads(km, k, strs, reads)
    return {"k": k, "thr": thr, "n_listed": len(km), "n_unitigs": len(strs), "reads": reads,
            "segments": [[s["pos"], s["n_windows"], s["o"], s["off"]] for s in segs], "seg_offsets": so,
            "records": [[r[f] for f in R.REC_FIELDS] for r in recs], "hits": hits}


if __name__ == "__main__":
    out = {name: record(name) for name in R.MAP_CASES}
    with open(os.path.join(HERE, "unitig_map_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
