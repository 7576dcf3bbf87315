#!/usr/bin/env python3
"""Generate tests/golden/seq_extend_golden.json: what kmx_extend_seqs must return for seeds over the GENOME_CASES genomes.

Every answer comes from the CPU oracle, the rule from tests/seq_extend_ref.py.  The seeds of a case are the reads of
seq_reads.make_reads (they hold N, lowercase, IUPAC, short and empty reads: a walk starts at a read's last k bytes) and clean
k-mers cut from the genome.  Recorded per case and depth in {0, 2} (thr = ci, max_ext = 300): the tallies per stop code, the
rows the rule asked about, and the sha256 of the rows of appended bases and of the records.  REFUSES to write unless the
result is not degenerate.  Data only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import seq_extend_ref as X  # noqa: E402
import seq_reads as R  # noqa: E402
from common import GENOME_CASES  # noqa: E402
from make_seq_correct_golden import oracle_of  # noqa: E402,F401

RECIPE = {"n_reads": 1500, "n_clean": 500, "clean_seed": 47, "max_ext": 300, "depths": [0, 2]}


def seeds_of(case, n_reads=RECIPE["n_reads"], n_clean=RECIPE["n_clean"], clean_seed=RECIPE["clean_seed"]):
    """(uint8 bases, uint64 offsets) of a case's seeds: the reads, then clean k-mers of the genome"""
    _, k, _, _, _, _, n_bases = case
    g = R.genome_ascii(n_bases)
    rng = np.random.default_rng(clean_seed)
    clean = [g[a:a + k].tobytes() for a in rng.integers(0, n_bases - k, size=n_clean).tolist()]
    return R.flatten(R.make_reads(n_bases, k, n_reads=n_reads) + clean)


def entry(case, o):
    _, k, ci, _, _, _, _ = case
    buf, off = seeds_of(case)
    e = {"thr": ci, "max_ext": RECIPE["max_ext"], "n_seeds": len(off) - 1, "depth": {}}
    for depth in RECIPE["depths"]:
        ext, rec, nq = X.oracle_extend(o, buf, off, k, ci, RECIPE["max_ext"], depth)
        t = X.tallies(rec)
        e["depth"][str(depth)] = {"tallies": t, "rows_asked": nq, "ext_sha256": X.sha_ext(ext), "records_sha256": X.sha_records(rec)}
    t0, t2 = e["depth"]["0"]["tallies"], e["depth"]["2"]["tallies"]
    if not (t2["max_ext"] >= 500 and t2["bad_seed"] >= 100 and t2["n_lookahead"] >= 1000 and t2["n_ext"] > 5 * t0["n_ext"] and t0["branch"] + t0["join"] >= 500):
        sys.exit(f"{case[0]}: degenerate result {t0} {t2}")
    return e


def main():
    out = {"generator": "tests/golden/make_seq_extend_golden.py", "recipe": RECIPE, "cases": {c[0]: entry(c, oracle_of(c)) for c in GENOME_CASES}}
    with open(os.path.join(HERE, "seq_extend_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: {d: v["tallies"] for d, v in e["depth"].items()} for k, e in out["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
