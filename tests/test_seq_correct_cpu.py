"""CPU side of the read correction (kmx_correct_seqs): the record's layout in the header and the NumPy dtype agree; the
reference rule (tests/seq_correct_ref.py) against hand-built cases for every row of the shape table, gap closing,
min_support, an N and a forced ambiguous site; the rule driven by the CPU oracle restores known substitutions without
miscorrecting; the fixture tests/golden/seq_correct_golden.json still describes the oracle's result; the facade compiles."""
import json
import os
import subprocess
import sys

import numpy as np

import count_reads as CR
import oracle_lib as O
import seq_correct_ref as S
import seq_reads as R
from common import GENOME_CASES
from kmcex_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
K = 5


def test_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu", sizeof(kmx_seq_correction));\n'
                   + "".join(f' printf(" %zu", offsetof(kmx_seq_correction, {f}));\n' for f in S.FIELDS) + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *offs = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == 64 == api.SEQ_CORRECTION_DTYPE.itemsize and S.DTYPE == api.SEQ_CORRECTION_DTYPE
    assert offs == [8 * i for i in range(8)] == [api.SEQ_CORRECTION_DTYPE.fields[f][1] for f in S.FIELDS]
    assert "kmx_correct_seqs" in api.ABI_SYMBOLS and "kmx_correct_seqs_dev" in api.ABI_SYMBOLS


def _sites(weak_windows, nw, min_support=1, k=K):
    """the tried sites of one sequence with nw windows of which these are weak (answer 0 against thr 1)"""
    pb = np.full(nw + k - 1, -1, dtype=np.int32)
    pb[:nw] = 1
    pb[list(weak_windows)] = 0
    rec, sites = S.plan(pb, np.array([0, nw + k - 1], dtype=np.uint64), k, 1, min_support)
    return [s[1:] for s in sites], rec[0]


def test_every_row_of_the_shape_table():
    nw = 30
    assert _sites(range(nw), nw)[0] == []                                        # neither hasL nor hasR
    assert _sites(range(0, 3), nw)[0] == [(2, 0, 2)]                             # hasR only, shorter than k
    assert _sites(range(0, 9), nw)[0] == [(8, 4, 8)]                             # hasR only, longer than k: the last k windows
    assert _sites(range(27, nw), nw)[0] == [(31, 27, 29)]                        # hasL only: b = s + k - 1
    assert _sites(range(20, nw), nw)[0] == [(24, 20, 24)]                        # hasL only, long: the first k windows
    assert _sites(range(10, 14), nw)[0] == []                                    # both, len < k
    assert _sites(range(10, 15), nw)[0] == [(14, 10, 14)]                        # both, len = k: one substitution at base 14
    assert _sites(range(10, 17), nw)[0] == [(14, 10, 11), (16, 15, 16)]          # both, len = k + 2: clipped apart
    assert _sites(range(10, 25), nw)[0] == [(14, 10, 14), (24, 20, 24)]          # both, len >= 2k: k windows each
    s, r = _sites(list(range(2, 7)) + list(range(12, 17)), nw)                   # two runs in one sequence
    assert s == [(6, 2, 6), (16, 12, 16)] and (int(r["n_runs"]), int(r["n_weak"]), int(r["n_windows"])) == (2, 10, nw)
    # shorter than k, exactly k
    assert _sites([], 0)[0] == [] and _sites([0], 1)[0] == []


def test_gap_closing_and_min_support():
    nw = 30
    # one window answered > 0 inside the k weak windows of one error: closed, the run matches len = k again
    s, r = _sites([10, 11, 13, 14], nw)
    assert s == [(14, 10, 14)] and int(r["n_runs"]) == 1 and int(r["n_weak"]) == 4
    # a gap of two is not closed; closing is judged on `weak`, not on closed flags (10 . 12 . 14 closes 11 and 13 only)
    assert _sites([10, 13, 14], nw)[1]["n_runs"] == 2
    assert _sites([10, 12, 14], nw)[0] == [(14, 10, 14)]
    # the sequence's first and last window are never closed
    assert _sites([1], nw)[1]["n_runs"] == 1 and _sites([1], nw)[0] == []
    # min_support on both sides of |V|
    assert _sites(range(0, 3), nw, min_support=3)[0] == [(2, 0, 2)] and _sites(range(0, 3), nw, min_support=4)[0] == []
    s, r = _sites(range(10, 17), nw, min_support=3)                               # |V| = 2 at both ends: none tried, the run counted
    assert s == [] and int(r["n_runs"]) == 1


def _model(seqs, k=K, ci=1):
    """a CPU oracle holding every k-mer of these sequences"""
    buf, off = R.flatten(seqs)
    km, cnt = CR.count(buf, off, k, ci, 1023)
    o = O.OracleModel(ci, 1023, 7, 5)
    o.build(k, km, cnt)
    return o


def test_substitution_n_and_ambiguous_on_a_small_model():
    k = 21
    g = R.genome_ascii(3000, seed=5).tobytes()
    o = _model([g], k)
    read = bytearray(g[100:220])
    truth = bytes(read)
    read[60] = ord("A") if truth[60] != ord("A") else ord("C")                    # a substitution in the middle
    read[5] = ord("N")                                                            # an N near the start (hasR only)
    buf, off = R.flatten([bytes(read)])
    out, rec, _ = S.oracle_correct(o, buf, off, k, 1, 1)
    assert out.tobytes() == truth and int(rec["n_corrected"][0]) == 2 and int(rec["n_sites"][0]) == 2 and int(rec["n_runs"][0]) == 2
    # two alleles of one position in the model, the read carries a third: both pass, nothing changes
    alt = bytearray(g)
    others = [c for c in b"ACGT" if c != g[160]]
    alt[160] = others[0]
    o2 = _model([g, bytes(alt)], k)
    read = bytearray(g[100:220])
    read[60] = others[1]
    buf, off = R.flatten([bytes(read)])
    out, rec, _ = S.oracle_correct(o2, buf, off, k, 1, 1)
    assert out.tobytes() == bytes(read) and int(rec["n_ambiguous"][0]) == 1 and int(rec["n_corrected"][0]) == 0
    # two substitutions 3 bases apart: one run of k + 3 windows, each end verified on the 3 windows free of the other error
    read = bytearray(g[100:220])
    for p in (60, 63):
        read[p] = ord("A") if g[100 + p] != ord("A") else ord("C")
    buf, off = R.flatten([bytes(read)])
    out, rec, _ = S.oracle_correct(o, buf, off, k, 1, 1)
    assert (int(rec["n_runs"][0]), int(rec["n_weak"][0]), int(rec["n_sites"][0])) == (1, k + 3, 2)
    assert out.tobytes() == g[100:220] and int(rec["n_corrected"][0]) == 2
    _, rec, _ = S.oracle_correct(o, buf, off, k, 1, 4)                             # min_support 4 > |V| = 3: not tried
    assert int(rec["n_sites"][0]) == 0 and int(rec["n_runs"][0]) == 1


def test_known_substitutions_are_restored_not_miscorrected():
    """reads cut from the GENOME_CASES genomes with known substitutions: at least half restored, miscorrected <= 1 % of the
    corrected (1500 reads of 80-300 bases, 1 % substitutions, thr = ci, min_support = 1)"""
    import make_seq_correct_golden as G
    for case in GENOME_CASES:
        _, k, ci, cs, nh, nb, n_bases = case
        o = G.oracle_of(case)
        g = R.genome_ascii(n_bases)
        rng = np.random.default_rng(3)
        truth, reads = [], []
        for i in range(1500):
            ln = int(rng.integers(80, 301))
            a = int(rng.integers(0, n_bases - ln))
            r = g[a:a + ln].copy()
            if i % 2:
                r = R._COMP[r[::-1]]
            t = r.copy()
            subs = np.nonzero(rng.random(ln) < 0.01)[0]
            r[subs] = R.ACGT[(np.searchsorted(R.ACGT, r[subs]) + rng.integers(1, 4, size=len(subs))) % 4]
            truth.append(t.tobytes())
            reads.append(r.tobytes())
        buf, off = R.flatten(reads)
        tb, _ = R.flatten(truth)
        out, rec, _ = S.oracle_correct(o, buf, off, k, ci, 1)
        errors = int((buf != tb).sum())
        restored = int(((buf != tb) & (out == tb)).sum())
        mis = int(((out != buf) & (out != tb)).sum())
        corrected = int(rec["n_corrected"].sum())
        print(case[0], "errors", errors, "restored", restored, "miscorrected", mis, "corrected", corrected)
        assert errors > 2000 and 2 * restored >= errors and 100 * mis <= corrected and corrected == int((out != buf).sum())


def test_result_of_the_golden():
    import make_seq_correct_golden as G
    with open(os.path.join(ROOT, "tests", "golden", "seq_correct_golden.json")) as f:
        sg = json.load(f)
    assert sorted(sg["cases"]) == sorted(c[0] for c in GENOME_CASES)
    for case in GENOME_CASES:
        assert G.entry(case, G.oracle_of(case)) == sg["cases"][case[0]], case[0]
    t = sg["cases"]["genome_k31_ci1"]["tallies"]
    assert (t["n_windows"], t["n_weak"], t["n_runs"], t["n_sites"], t["n_corrected"], t["n_ambiguous"], t["n_unfixable"]) == (326362, 101447, 3324, 3718, 2593, 4, 1121)


def test_facade_seq_correct_program_compiles(tmp_path):
    api.load_library()
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_correct.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", str(tmp_path / "facade_seq_correct")])
