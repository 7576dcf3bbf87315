#!/usr/bin/env python3
"""Generate tests/golden/seq_edit_golden.json: what kmx_edit_seqs / kmx_apply_edits must return for reads of the GENOME_CASES
genomes with substitutions, lost and surplus bases (tests/seq_edit_reads.py).

The per-base answers and the candidate windows' answers come from the CPU oracle, the rule from tests/seq_edit_ref.py.
Recorded per case (thr = ci, min_support = 1, ops = 7, n_reads = 2000): the tallies the tests assert on the oracle's result,
the verification windows asked, the floors of the non-degeneracy test, and the sha256 of the edit list, the records and the
applied bases; the tallies alone for the other (thr, min_support, ops) the GPU test runs.  REFUSES to write unless the result
is not degenerate.  Data only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import seq_edit_reads as ER  # noqa: E402
import seq_edit_ref as E  # noqa: E402
import seq_reads as R  # noqa: E402
from common import GENOME_CASES  # noqa: E402
from make_seq_correct_golden import oracle_of  # noqa: E402

TEST_READS = 2000
FLOORS = {"n_sub": 400, "n_del": 250, "n_ins": 200, "n_ambiguous": 1, "edits_in_dirty_reads": 100}


def reads_of(case, **recipe):
    """(reads, truths, bases, offsets) of the recipe"""
    _, k, _, _, _, _, n_bases = case
    reads, truths = ER.make_reads(n_bases, k, **recipe)
    return (reads, truths) + R.flatten(reads)


def measures(reads, truths, buf, off, edits, rec):
    """the tallies plus what the non-degeneracy test asks of the oracle's result"""
    out, off2 = E.apply_edits(buf, off, edits)
    fixed = [out[int(off2[i]):int(off2[i + 1])].tobytes() for i in range(len(reads))]
    t = E.tallies(rec, edits)
    seq_of = np.searchsorted(off.astype(np.int64), (edits >> np.uint64(8)).astype(np.int64), side="right") - 1
    t["edits_in_dirty_reads"] = int(ER.dirty_reads(reads)[seq_of].sum())
    t["reads_wrong_before"] = sum(r != x for r, x in zip(reads, truths))
    t["reads_wrong_after"] = sum(f != x for f, x in zip(fixed, truths))
    t["reads_broken"] = sum(r == x and f != x for r, f, x in zip(reads, fixed, truths))
    return t, out


def entry(case, o):
    k, ci = case[1], case[2]
    reads, truths, buf, off = reads_of(case, n_reads=TEST_READS)
    edits, rec, nq = E.oracle_edit(o, buf, off, k, ci, 1, 7)
    t, out = measures(reads, truths, buf, off, edits, rec)
    if not (all(t[f] >= v for f, v in FLOORS.items()) and t["reads_broken"] == 0):
        sys.exit(f"{case[0]}: degenerate result {t}")
    e = {"thr": ci, "min_support": 1, "ops": 7, "tallies": t, "floors": FLOORS, "verify_windows": nq, "edits_sha256": E.sha(edits), "records_sha256": E.sha(rec),
         "bases_sha256": E.sha(out), "variants": {}}
    for thr, ms in ((ci, 1), (ci, 4), (ci + 1, 1)):
        for ops in (7, 1, 6):
            if (thr, ms, ops) != (ci, 1, 7):
                e2, r2, _ = E.oracle_edit(o, buf, off, k, thr, ms, ops)
                e["variants"][f"thr{thr}_ms{ms}_ops{ops}"] = E.tallies(r2, e2)
    return e


def main():
    out = {"generator": "tests/golden/make_seq_edit_golden.py", "recipe": {"n_reads": TEST_READS}, "cases": {c[0]: entry(c, oracle_of(c)) for c in GENOME_CASES}}
    with open(os.path.join(HERE, "seq_edit_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: v["tallies"] for k, v in out["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
