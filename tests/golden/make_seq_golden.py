#!/usr/bin/env python3
"""Generate tests/golden/seq_golden.json from the REAL reference (oracle/_ref/ref_driver, built by build() where the
reference sources are present).

  1. writes the genome_k31_ci1 KMC1 database (kmcex_amd.synth.genome_stream + kmcex_amd.kmcdb) and has the reference
     build its model from it (get_model -> init -> save, kmodel.hpp:674,57,173);
  2. cuts the reads of the tests/seq_reads.py recipe into their k-mer window strings and has the reference answer them
     (get_model(dir) -> kmer_to_occ(vector<string>), kmodel.hpp:680,90);
  3. REFUSES to write unless the CPU oracle (oracle/kmx_oracle.c) gives the same model files and the same answers;
  4. records the recipe, the window and dirty-window counts and the sha256 of the per-base int32 answer vector (-1 where
     no window of a read starts): what kmx_query_seqs must return for those reads.
Data only: no reference program text.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import seq_reads as R  # noqa: E402
from common import GENOME_CASES, sha_file, sha_occ  # noqa: E402
from kmcex_amd import kmcdb, synth  # noqa: E402

CASE_NAME = "genome_k31_ci1"


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref/ref_driver missing: run `make -C oracle ref` where the reference sources are present")
    name, k, ci, cs, nh, nb, n_bases = next(c for c in GENOME_CASES if c[0] == CASE_NAME)
    tmp = tempfile.mkdtemp(prefix="kmx_seq_golden_")
    try:
        km, cnt = synth.genome_stream(n_bases, k, ci, cs)
        db = os.path.join(tmp, name)
        kmcdb.write_kmc1(db, km, cnt, k, ci, cs)
        O.ref_build(db, db + ".ref", ci, cs, nh, nb)
        o = O.OracleModel(ci, cs, nh, nb)
        o.build(k, km, cnt)
        o.save(db + ".ora")
        for f in ("header", "km.bin", "rest.bin"):
            if sha_file(f"{db}.ref/{f}") != sha_file(f"{db}.ora/{f}"):
                sys.exit(f"{name}: oracle {f} differs from the reference")
        buf, offsets = R.flatten(R.make_reads(n_bases, k, **R.RECIPE))
        valid = R.valid_mask(offsets, k)
        starts = np.nonzero(valid)[0]
        windows = [buf[p:p + k].tobytes().decode("latin-1") for p in starts]
        ref = np.full(len(buf), -1, dtype=np.int32)
        ref[starts] = O.ref_query(db + ".ref", windows, db)
        if not np.array_equal(ref, R.oracle_per_base(o, buf, offsets, k)):
            sys.exit(f"{name}: oracle answers differ from the reference's")
        out = {"generator": "tests/golden/make_seq_golden.py", "case": name, "recipe": R.RECIPE,
               "n_reads": int(len(offsets) - 1), "n_bases": int(len(buf)), "n_windows": int(valid.sum()),
               "n_dirty_windows": R.dirty_windows(buf, offsets, k), "n_nonzero": int((ref > 0).sum()),
               "per_base_sha256": sha_occ(ref)}
        with open(os.path.join(HERE, "seq_golden.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        print(name, "ok:", out["n_windows"], "windows,", out["n_dirty_windows"], "dirty,", out["n_nonzero"], "non-zero", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
