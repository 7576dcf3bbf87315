#!/usr/bin/env python3
"""Generate tests/golden/seq_summary_golden.json: what kmx_summarise_seqs must return for the reads of seq_golden.json.

  1. recomputes the per-base answers of the tests/seq_reads.py recipe with the CPU oracle and REFUSES to go on unless their
     digest is the reference's, as recorded in seq_golden.json (make_seq_golden.py wrote it from the real reference);
  2. reduces them per read with tests/seq_summary_ref.py, thr = (1, 3, 8), and REFUSES to write unless the records add up to
     the fixture's own figures (n_windows, n_nonzero);
  3. records the sha256 of the record bytes (64 per read) and, for the reads of the GPU test (every GENOME_CASES case,
     n_reads = 2000), the per-read tallies the test asserts on the oracle's records.
Data only: no reference program text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import seq_reads as R  # noqa: E402
import seq_summary_ref as S  # noqa: E402
from common import GENOME_CASES, sha_occ  # noqa: E402
from kmcex_amd import synth  # noqa: E402

THR = [1, 3, 8]
TEST_READS = 2000


def oracle_records(case, **recipe):
    """(records, per-base answers) of the CPU oracle for reads of a GENOME_CASES case"""
    _, k, ci, cs, nh, nb, n_bases = case
    km, cnt = synth.genome_stream(n_bases, k, ci, cs)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    buf, offsets = R.flatten(R.make_reads(n_bases, k, **recipe))
    occ = R.oracle_per_base(o, buf, offsets, k)
    return S.summarise(occ, offsets, k, THR), occ


def main():
    with open(os.path.join(HERE, "seq_golden.json")) as f:
        g = json.load(f)
    case = next(c for c in GENOME_CASES if c[0] == g["case"])
    rec, occ = oracle_records(case, **g["recipe"])
    if sha_occ(occ) != g["per_base_sha256"]:
        sys.exit("the oracle's per-base answers are not the reference's (seq_golden.json)")
    if int(rec["n_windows"].sum()) != g["n_windows"] or int(rec["n_ge"][:, 0].sum()) != g["n_nonzero"]:
        sys.exit("the records do not add up to seq_golden.json's n_windows / n_nonzero")
    out = {"generator": "tests/golden/make_seq_summary_golden.py", "case": g["case"], "recipe": g["recipe"], "thr": THR,
           "n_reads": int(len(rec)), "records_sha256": S.sha_records(rec),
           "test_reads": TEST_READS, "tallies": {c[0]: S.tallies(oracle_records(c, n_reads=TEST_READS)[0]) for c in GENOME_CASES}}
    with open(os.path.join(HERE, "seq_summary_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(out["case"], "ok:", out["n_reads"], "records", out["records_sha256"][:16], out["tallies"], flush=True)


if __name__ == "__main__":
    main()
