#!/usr/bin/env python3
"""Generate tests/golden/count_golden.json from the REAL reference (oracle/_ref/ref_driver, built by build() where the
reference sources are present).

For every case of tests/count_reads.py GOLDEN_CASES:
  1. cuts the reads of the tests/seq_reads.py generator (N runs, lowercase stretches, IUPAC letters, reads of length 0,
     k - 1, k and k + 1) into windows and counts them by the numpy restatement of the counting rule (tests/count_reads.py);
  2. writes that listing as a KMC1 database (kmcex_amd.kmcdb) and has the reference build its model from it
     (get_model -> init -> save, kmodel.hpp:674,57,173);
  3. REFUSES to write unless the CPU oracle (oracle/kmx_oracle.c) built from the same listing saves the same three files;
  4. records the recipe, the windows / distinct / listed k-mers, the sha256 of the listing and of the three files: what
     kmx_count_* and kmx_build_from_reads must produce from those reads.
Data only: no reference program text.
"""
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import count_reads as CR  # noqa: E402
import oracle_lib as O  # noqa: E402
import seq_reads as R  # noqa: E402
from common import sha_file  # noqa: E402
from kmcex_amd import kmcdb  # noqa: E402


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref/ref_driver missing: run `make -C oracle ref` where the reference sources are present")
    tmp = tempfile.mkdtemp(prefix="kmx_count_golden_")
    out = {"generator": "tests/golden/make_count_golden.py", "cases": {}}
    try:
        for name, k, ci, cs, nh, nb, n_bases, args in CR.GOLDEN_CASES:
            buf, off = R.flatten(R.make_reads(n_bases, k, **args))
            km, cnt = CR.count(buf, off, k, ci, cs)
            db = os.path.join(tmp, name)
            kmcdb.write_kmc1(db, km, cnt, k, ci, cs)
            O.ref_build(db, db + ".ref", ci, cs, nh, nb)
            o = O.OracleModel(ci, cs, nh, nb)
            o.build(k, km, cnt)
            o.save(db + ".ora")
            files = {}
            for f in ("header", "km.bin", "rest.bin"):
                files[f] = sha_file(f"{db}.ref/{f}")
                if files[f] != sha_file(f"{db}.ora/{f}"):
                    sys.exit(f"{name}: oracle {f} differs from the reference")
            out["cases"][name] = {"k": k, "ci": ci, "cs": cs, "nh": nh, "nb": nb, "genome_bases": n_bases, "reads": args,
                                  "n_reads": int(len(off) - 1), "n_bases": int(len(buf)),
                                  "n_windows": int(len(CR.window_starts(buf, off, k))),
                                  "n_distinct": int(len(CR.count(buf, off, k, 1, 2 ** 32 - 1)[0])), "n_listed": int(len(km)),
                                  "listing_sha256": CR.listing_sha(km, cnt), "files": files}
            print(name, "ok:", out["cases"][name]["n_windows"], "windows,", out["cases"][name]["n_listed"], "listed", flush=True)
        with open(os.path.join(HERE, "count_golden.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
