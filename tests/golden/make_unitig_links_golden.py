#!/usr/bin/env python3
"""Generate tests/golden/unitig_links_golden.json: what kmx_unitig_graph must return beside the unitigs for the cases of
tests/unitigs_ref.py (CASES: pinned by seed), computed by the restatement tests/unitig_links_ref.py alone.  Per case: the
number of links and the sha256 of link_offsets (uint64) and links (uint32).  Data only."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unitig_links_ref as UL  # noqa: E402
import unitigs_ref as U  # noqa: E402


def sha(a) -> str:
    return hashlib.sha256(a.tobytes()).hexdigest()


def entry(name, computed=None):
    """computed: UL.case_links(name) where the caller has it already"""
    import numpy as np
    _, _, _, _, strs, _, off, lk = computed or UL.case_links(name)
    return {"unitigs": len(strs), "n_links": int(len(lk)), "link_offsets_sha256": sha(np.ascontiguousarray(off, dtype="<u8")),
            "links_sha256": sha(np.ascontiguousarray(lk, dtype="<u4"))}


def main():
    out = {"generator": "tests/golden/make_unitig_links_golden.py", "cases": {name: entry(name) for name in U.CASES}}
    with open(os.path.join(HERE, "unitig_links_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: [v["unitigs"], v["n_links"]] for k, v in out["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
