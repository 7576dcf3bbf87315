#!/usr/bin/env python3
"""Generate tests/golden/seq_correct_golden.json: what kmx_correct_seqs must return for reads of the GENOME_CASES genomes.

The per-base answers and the candidate windows' answers come from the CPU oracle, the rule from tests/seq_correct_ref.py.
Recorded per case (thr = ci, min_support = 1, seq_reads.make_reads(n_reads = 2000)): the tallies the GPU test asserts on the
oracle's result, the verification windows asked, and the sha256 of the corrected bases and of the records; the tallies
alone for min_support = 4 and thr = ci + 1.  REFUSES to write unless the result is not degenerate.  Data only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import seq_correct_ref as S  # noqa: E402
import seq_reads as R  # noqa: E402
from common import GENOME_CASES  # noqa: E402
from kmcex_amd import synth  # noqa: E402

TEST_READS = 2000


def oracle_of(case):
    _, k, ci, cs, nh, nb, n_bases = case
    km, cnt = synth.genome_stream(n_bases, k, ci, cs)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    return o


def result(case, o, thr, min_support, **recipe):
    """(bases in, offsets, corrected bases, records, verification windows) of the oracle-driven rule"""
    _, k, _, _, _, _, n_bases = case
    buf, offsets = R.flatten(R.make_reads(n_bases, k, **recipe))
    out, rec, nq = S.oracle_correct(o, buf, offsets, k, thr, min_support)
    return buf, offsets, out, rec, nq


def entry(case, o):
    ci = case[2]
    buf, off, out, rec, nq = result(case, o, ci, 1, n_reads=TEST_READS)
    t = S.tallies(rec, buf, out, off)
    if not (t["n_corrected"] >= 2000 and t["n_unfixable"] >= 500 and t["corrected_non_acgt"] >= 100 and t["reads_changed"] >= 1000):
        sys.exit(f"{case[0]}: degenerate result {t}")
    e = {"thr": ci, "min_support": 1, "tallies": t, "verify_windows": nq, "bases_sha256": S.sha_bases(out), "records_sha256": S.sha_records(rec), "variants": {}}
    for thr, ms in ((ci, 4), (ci + 1, 1)):
        b2, o2, out2, rec2, _ = result(case, o, thr, ms, n_reads=TEST_READS)
        e["variants"][f"thr{thr}_ms{ms}"] = S.tallies(rec2, b2, out2, o2)
    return e


def main():
    out = {"generator": "tests/golden/make_seq_correct_golden.py", "recipe": {"n_reads": TEST_READS}, "cases": {c[0]: entry(c, oracle_of(c)) for c in GENOME_CASES}}
    with open(os.path.join(HERE, "seq_correct_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: v["tallies"] for k, v in out["cases"].items()}), flush=True)


if __name__ == "__main__":
    main()
