#!/usr/bin/env python3
"""Generate tests/golden/seq_polish_golden.json: what kmx_polish_seqs must return for reads of the GENOME_CASES genomes with
substitutions, lost and surplus bases (tests/seq_edit_reads.py, n_reads = 600: 608 reads with the special ones).

Every pass is tests/seq_edit_ref.py's rule driven by the CPU oracle, the loop tests/seq_polish_ref.py's.  Recorded per case
(thr = ci, min_support = 1, ops = 7) and per max_passes in 1, 2, 8: the sha256 of the polished bases, of offsets_out and of
the records, and the tallies (sums of the records, passes run, reads examined and edited per pass, reads that differ from
their truth after each pass).  Data only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seq_edit_ref as E  # noqa: E402
import seq_polish_ref as P  # noqa: E402
from common import GENOME_CASES  # noqa: E402
from make_seq_correct_golden import oracle_of  # noqa: E402
from make_seq_edit_golden import reads_of  # noqa: E402

TEST_READS = 600
MAX_PASSES = (1, 2, 8)


def entry(case, o, cache=None):
    k, ci = case[1], case[2]
    reads, truths, buf, off = reads_of(case, n_reads=TEST_READS)
    fn = P.oracle_fn(o, k, ci, 1, 7, {} if cache is None else cache)
    e = {"thr": ci, "min_support": 1, "ops": 7, "n_reads": len(reads), "reads_wrong_before": P.wrong(reads, truths), "max_passes": {}}
    for mp in MAX_PASSES:
        res = P.polish(fn, buf, off, mp)
        e["max_passes"][str(mp)] = {"bases_sha256": E.sha(res["bases"]), "offsets_sha256": E.sha(res["offsets"]), "records_sha256": E.sha(res["records"]),
                                    "tallies": P.tallies(res, truths)}
    return e


def main():
    out = {"generator": "tests/golden/make_seq_polish_golden.py", "recipe": {"n_reads": TEST_READS}, "cases": {c[0]: entry(c, oracle_of(c)) for c in GENOME_CASES}}
    with open(os.path.join(HERE, "seq_polish_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: v["max_passes"]["8"]["tallies"] for k, v in out["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
