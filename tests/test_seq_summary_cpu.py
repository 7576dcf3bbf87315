"""CPU side of the per-sequence summary (kmx_summarise_seqs): the record's layout in the header, the ctypes mirror and the
NumPy dtype agree; the NumPy reference (tests/seq_summary_ref.py) against hand-written records; the fixture
tests/golden/seq_summary_golden.json still describes what the CPU oracle's answers reduce to; the C++ facade's seq_summary
compiles with the reference's flags."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

import seq_reads as R
import seq_summary_ref as S
from common import GENOME_CASES, sha_occ
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
FIELDS = ["n_windows", "sum", "min", "max", "n_ge", "first_below", "last_below"]


def test_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %d", sizeof(kmx_seq_summary), KMX_SEQ_THRESHOLDS);\n'
                   + "".join(f' printf(" %zu", offsetof(kmx_seq_summary, {f}));\n' for f in FIELDS) + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, n_thr, *offs = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == 64 and n_thr == 3 == api.SEQ_THRESHOLDS
    assert ctypes.sizeof(api.SeqSummary) == 64 and api.SEQ_SUMMARY_DTYPE.itemsize == 64 and S.DTYPE == api.SEQ_SUMMARY_DTYPE
    assert [f for f, _ in api.SeqSummary._fields_] == FIELDS == list(api.SEQ_SUMMARY_DTYPE.names)
    assert offs == [getattr(api.SeqSummary, f).offset for f in FIELDS] == [api.SEQ_SUMMARY_DTYPE.fields[f][1] for f in FIELDS]
    assert offs == [0, 8, 16, 20, 24, 48, 56]                    # no padding


def _rec(n_windows, total, mn, mx, n_ge, first, last):
    r = np.zeros(1, dtype=S.DTYPE)
    r[0] = (n_windows, total, mn, mx, n_ge, first, last)
    return r


def _one(answers, length, k, thr):
    """a single sequence of `length` bases whose windows have these answers"""
    pb = np.full(length, -1, dtype=np.int32)
    pb[:len(answers)] = answers
    return S.summarise(pb, np.array([0, length], dtype=np.uint64), k, thr)


def test_reference_against_hand_written_records():
    k = 5
    cases = [
        # (answers, length, thr, the record written by hand)
        ([], 0, (1, 3, 8), (0, 0, -1, -1, [0, 0, 0], 0, 0)),                              # an empty read
        ([], k - 1, (1, 3, 8), (0, 0, -1, -1, [0, 0, 0], 0, 0)),                          # k - 1 bases: no window
        ([7], k, (1, 3, 8), (1, 7, 7, 7, [1, 1, 0], 1, 1)),                               # k bases: one window, none below
        ([0, 9], k + 1, (1, 3, 8), (2, 9, 0, 9, [1, 1, 1], 0, 0)),                        # k + 1 bases
        ([0, 0, 0], k + 2, (1, 3, 8), (3, 0, 0, 0, [0, 0, 0], 0, 2)),                     # every window below
        ([5, 6, 7], k + 2, (1, 3, 8), (3, 18, 5, 7, [3, 3, 0], 3, 3)),                    # none below: both = n_windows
        ([5, 0, 7, 0, 2], k + 4, (), (5, 14, 0, 7, [0, 0, 0], 5, 5)),                     # n_thr = 0
        ([5, 0, 7, 0, 2], k + 4, (3,), (5, 14, 0, 7, [2, 0, 0], 1, 4)),                   # one threshold
        ([5, 0, 7, 0, 2], k + 4, (1, 3, 8), (5, 14, 0, 7, [3, 2, 0], 1, 3)),              # n_thr = 3
        ([5, 0, 7, 0, 2], k + 4, (8, 1, 3), (5, 14, 0, 7, [0, 3, 2], 0, 4)),              # thresholds need not ascend
        ([5, 0, 7, 0, 2], k + 4, (0, -4, 6), (5, 14, 0, 7, [5, 5, 1], 5, 5)),             # thresholds <= 0: nothing is below
        ([3, 3, 2, 3], k + 3, (3, 3, 3), (4, 11, 2, 3, [3, 3, 3], 2, 2)),                 # equal thresholds, one weak window
    ]
    for answers, length, thr, want in cases:
        got = _one(answers, length, k, thr)
        assert S.same(got, _rec(*want)), (answers, thr, got, want)
    # several sequences, empty ones between them, in one call
    pb = np.array([4, 0, -1, -1, -1, -1, 9, -1, -1, -1, -1, -1, -1, -1], dtype=np.int32)
    offsets = np.array([0, 0, 6, 6, 11, 14, 14], dtype=np.uint64)   # lengths 0 6 0 5 3 0
    got = S.summarise(pb, offsets, k, (1, 5))
    want = np.concatenate([_rec(0, 0, -1, -1, [0, 0, 0], 0, 0), _rec(2, 4, 0, 4, [1, 0, 0], 1, 1), _rec(0, 0, -1, -1, [0, 0, 0], 0, 0),
                           _rec(1, 9, 9, 9, [1, 1, 0], 1, 1), _rec(0, 0, -1, -1, [0, 0, 0], 0, 0), _rec(0, 0, -1, -1, [0, 0, 0], 0, 0)])
    assert S.same(got, want)


def test_records_of_the_reference_golden():
    """the oracle's answers for the recipe still have the reference's digest, and reduce to the committed records"""
    import make_seq_summary_golden as G
    with open(os.path.join(ROOT, "tests", "golden", "seq_golden.json")) as f:
        g = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "seq_summary_golden.json")) as f:
        sg = json.load(f)
    assert (sg["case"], sg["recipe"], sg["thr"]) == (g["case"], g["recipe"], [1, 3, 8])
    case = next(c for c in GENOME_CASES if c[0] == g["case"])
    rec, occ = G.oracle_records(case, **g["recipe"])
    assert sha_occ(occ) == g["per_base_sha256"]
    assert len(rec) == g["n_reads"] == sg["n_reads"]
    assert int(rec["n_windows"].sum()) == g["n_windows"] == 491442
    assert int(rec["n_ge"][:, 0].sum()) == g["n_nonzero"] == 337093
    assert S.sha_records(rec) == sg["records_sha256"]
    for c in GENOME_CASES:
        assert S.tallies(G.oracle_records(c, n_reads=sg["test_reads"])[0]) == sg["tallies"][c[0]], c[0]


def test_facade_seq_summary_program_compiles(tmp_path):
    api.load_library()
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_summary.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", str(tmp_path / "facade_seq_summary")])
