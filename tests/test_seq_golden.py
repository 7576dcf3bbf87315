"""CPU side of the sequence query (kmx_query_seqs): the fixture tests/golden/seq_golden.json still describes what the CPU
oracle answers for the read recipe of tests/seq_reads.py, synth.genome_bases is genome_stream's sequence, and the C++
facade's seq_to_occ compiles with the reference's flags."""
import json
import os
import subprocess

import numpy as np

import oracle_lib as O
import seq_reads as R
from common import GENOME_CASES, sha_occ
from kmcex_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_answers_match_the_reference_golden():
    with open(os.path.join(ROOT, "tests", "golden", "seq_golden.json")) as f:
        g = json.load(f)
    name, k, ci, cs, nh, nb, n_bases = next(c for c in GENOME_CASES if c[0] == g["case"])
    km, cnt = synth.genome_stream(n_bases, k, ci, cs)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    buf, offsets = R.flatten(R.make_reads(n_bases, k, **g["recipe"]))
    assert (len(offsets) - 1, len(buf)) == (g["n_reads"], g["n_bases"])
    assert int(R.valid_mask(offsets, k).sum()) == g["n_windows"]
    assert R.dirty_windows(buf, offsets, k) == g["n_dirty_windows"]
    occ = R.oracle_per_base(o, buf, offsets, k)
    assert int((occ > 0).sum()) == g["n_nonzero"]
    assert sha_occ(occ) == g["per_base_sha256"]


def test_genome_bases_is_the_sequence_of_genome_stream():
    k, n = 21, 5000
    b = synth.genome_bases(n)
    assert b.dtype == np.uint64 and b.shape == (n,) and b.max() <= 3
    v = np.zeros(n - k + 1, dtype=np.uint64)
    for j in range(k):
        v = (v << np.uint64(2)) | b[j:j + n - k + 1]
    km, _ = synth.genome_stream(n, k, 1, 1023)
    assert np.array_equal(km, synth.sort_unique(synth.canonical(v, k)))


def test_valid_mask_marks_every_window_inside_its_sequence():
    offsets = np.array([0, 0, 2, 3, 8, 8, 12], dtype=np.uint64)
    assert R.valid_mask(offsets, 3).tolist() == [False, False, False, True, True, True, False, False, True, True, False, False]


def test_facade_seq_program_compiles(tmp_path):
    api.load_library()
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", str(tmp_path / "facade_seq")])
