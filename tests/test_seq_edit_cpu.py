"""CPU side of kmx_edit_seqs / kmx_apply_edits: the record's layout in the header and the NumPy dtype agree; the reference rule
(tests/seq_edit_ref.py) with ops = SUB equals tests/seq_correct_ref.py; hand-built reads, one per row of the shape table, get
exactly the expected edit from the rule driven by the CPU oracle; the oracle's result on the recipe's reads is not degenerate
and is the one tests/golden/seq_edit_golden.json describes; kmx_apply_edits (host only) against the NumPy apply."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import seq_correct_ref as S
import seq_edit_reads as ER
import seq_edit_ref as E
import seq_reads as R
from common import GENOME_CASES
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
K = 21
A, C, G, T = b"ACGT"


def test_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu", sizeof(kmx_seq_edits), sizeof(kmx_edit));\n'
                   + "".join(f' printf(" %zu", offsetof(kmx_seq_edits, {f}));\n' for f in E.FIELDS)
                   + ' printf(" %d %d %d %d %d %d\\n", KMX_EDIT_OPS_SUB, KMX_EDIT_OPS_DEL, KMX_EDIT_OPS_INS, KMX_EDIT_SUB, KMX_EDIT_DEL, KMX_EDIT_INS); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, esize, *rest = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == 80 == api.SEQ_EDITS_DTYPE.itemsize and esize == 8 and E.DTYPE == api.SEQ_EDITS_DTYPE
    assert rest[:10] == [8 * i for i in range(10)] == [api.SEQ_EDITS_DTYPE.fields[f][1] for f in E.FIELDS]
    assert rest[10:] == [E.OPS_SUB, E.OPS_DEL, E.OPS_INS, E.SUB, E.DEL, E.INS] == [api.EDIT_OPS_SUB, api.EDIT_OPS_DEL, api.EDIT_OPS_INS, api.EDIT_SUB, api.EDIT_DEL, api.EDIT_INS]
    for s in ("kmx_edit_seqs", "kmx_edit_seqs_dev", "kmx_apply_edits", "kmx_apply_edits_dev"):
        assert s in api.ABI_SYMBOLS


@pytest.mark.parametrize("case", GENOME_CASES, ids=[c[0] for c in GENOME_CASES])
def test_ops_sub_is_the_substitution_corrector(case):
    """ops = KMX_EDIT_OPS_SUB: changed bytes, n_sites and the corrected / ambiguous / unfixable counts of seq_correct_ref"""
    import make_seq_correct_golden as G
    _, k, ci, _, _, _, n_bases = case
    o = G.oracle_of(case)
    buf, off = R.flatten(R.make_reads(n_bases, k, n_reads=2000))
    for thr, ms in ((ci, 1), (ci + 1, 4)):
        w_out, w_rec, w_nq = S.oracle_correct(o, buf, off, k, thr, ms)
        edits, rec, nq = E.oracle_edit(o, buf, off, k, thr, ms, E.OPS_SUB)
        out, off2 = E.apply_edits(buf, off, edits)
        assert np.array_equal(out, w_out) and np.array_equal(off2, off) and nq == w_nq and len(edits) == int((w_out != buf).sum())
        for a, b in (("n_windows",) * 2, ("n_weak",) * 2, ("n_runs",) * 2, ("n_sites",) * 2, ("n_sub", "n_corrected"), ("n_ambiguous",) * 2, ("n_unfixable",) * 2):
            assert np.array_equal(rec[a], w_rec[b]), (a, thr, ms)
        assert not rec["n_del"].any() and not rec["n_ins"].any() and np.array_equal(rec["out_len"], np.diff(off))


# ---- the shape table on synthetic weak flags

def _cands(weak_windows, x, k=5, ops=7):
    """the candidates (op, position, code, v0, v1) of every run of a sequence x of which these windows are weak"""
    x = np.frombuffer(x, dtype=np.uint8)
    flags = np.zeros(len(x) - k + 1, dtype=bool)
    flags[list(weak_windows)] = True
    return [E.sites_of_run(s, e, x, k, ops) for s, e in S.runs_of(S.close_gaps(flags))]


def test_every_row_of_the_shape_table():
    x = b"ACGTACGTACGTACGTACGTACGTACGTACGTAC"                      # L = 34, k = 5: 30 windows; no two neighbours equal
    sub = lambda p, v0, v1: [(E.SUB, p, ci, v0, v1) for ci in range(4) if x[p] != b"ACGT"[ci]]
    ins = lambda j, v0, v1, codes=range(4): [(E.INS, j, ci, v0, v1) for ci in codes]
    assert _cands(range(30), x) == [[]]                                                       # neither hasL nor hasR
    assert _cands(range(0, 3), x) == [[sub(2, 0, 2) + [(E.DEL, 2, 0, 0, 1)] + ins(3, 0, 3)]]    # hasR only: a = e, j = e + 1
    assert _cands(range(0, 9), x) == [[sub(8, 4, 8) + [(E.DEL, 8, 0, 4, 7)] + ins(9, 5, 9)]]    # hasR only, longer than k: still all three kinds
    assert _cands([0], x) == [[sub(0, 0, 0) + [(E.DEL, 0, 0, 0, -1)] + ins(1, 0, 1)]]           # a surplus first base: DEL has no window
    assert _cands(range(27, 30), x) == [[sub(31, 27, 29) + [(E.DEL, 31, 0, 27, 28)] + ins(31, 27, 30)]]   # hasL only: a = j = s + k - 1
    assert _cands(range(20, 30), x) == [[sub(24, 20, 24) + [(E.DEL, 24, 0, 20, 23)] + ins(24, 20, 24)]]
    assert _cands(range(10, 17), x) == [[sub(14, 10, 11), sub(16, 15, 16)]]                     # both, len > k: the two SUB sites and nothing else
    assert _cands(range(10, 25), x) == [[sub(14, 10, 14), sub(24, 20, 24)]]
    assert _cands(range(10, 15), x) == [[sub(14, 10, 14) + [(E.DEL, 14, 0, 10, 13)]]]           # both, len = k: h = 1, SUB and DEL at e
    assert _cands(range(10, 14), x) == [[ins(14, 10, 14)]]                                      # len = k - 1: core x[13..14] = "CG": no DEL, INS for all four
    assert _cands(range(10, 13), x) == [[ins(13, 9, 13, [1])]]                                  # len = k - 2: core "ACG": the single INS of x[e + 1] = C
    y = bytearray(x)
    y[13] = y[14] = A                                                                           # core "AA": DEL at e, INS for all four
    assert _cands(range(10, 14), bytes(y)) == [[[(E.DEL, 13, 0, 9, 12)] + ins(14, 10, 14)]]
    y = bytearray(x)
    y[13] = T                                                                                   # core x[12..14] = "ATG": the single INS of x[e + 1] = T
    assert _cands(range(10, 13), bytes(y)) == [[ins(13, 9, 13, [3])]]
    y[13] = ord("N")                                                                            # an N in the core: none
    assert _cands(range(10, 13), bytes(y)) == [[[]]]
    y[12] = y[13] = y[14] = C                                                                   # core "CCC": DEL at e and the single INS of C
    assert _cands(range(10, 13), bytes(y)) == [[[(E.DEL, 12, 0, 8, 11)] + ins(13, 9, 13, [1])]]
    y = bytearray(x)
    y[12:15] = b"GTT"                                                                           # len < k, h = 4, core x[11..14] = "TGTT": no homopolymer, x[12..13] differ: no candidate
    assert _cands(range(10, 12), bytes(y)) == [[[]]]
    assert _cands(range(10, 14), bytes(y), ops=E.OPS_SUB) == [[[]]] and _cands(range(0, 3), x, ops=E.OPS_DEL | E.OPS_INS) == [[[(E.DEL, 2, 0, 0, 1)] + ins(3, 0, 3)]]


# ---- hand-built reads over a small genome, the rule driven by the CPU oracle

def _genome():
    return R.genome_ascii(6000, seed=5).tobytes()


def _model(g, k=K):
    buf, off = R.flatten([g])
    km, cnt = CR.count(buf, off, k, 1, 1023)
    o = O.OracleModel(1, 1023, 7, 5)
    o.build(k, km, cnt)
    return o


def _homopolymer(g, h, lo):
    """the first position p >= lo where exactly h equal bytes start"""
    for p in range(lo, len(g) - h - 1):
        if g[p - 1] != g[p] and all(g[p + j] == g[p] for j in range(h)) and g[p + h] != g[p]:
            return p
    raise AssertionError("no such homopolymer")


def _run(o, read, ms=1, ops=7, k=K):
    buf, off = R.flatten([read])
    edits, rec, _ = E.oracle_edit(o, buf, off, k, 1, ms, ops)
    out, _ = E.apply_edits(buf, off, edits)
    return [(int(e) >> 8, (int(e) >> 4) & 15, int(e) & 15) for e in edits], rec[0], out.tobytes()


def _other(*bases):
    return next(c for c in b"ACGT" if c not in bases)


def _surplus(g, p, h):
    """the base that, put in front of g[p], gives a homopolymer of h bytes there (h = 1: a base unlike both neighbours)"""
    return g[p] if h > 1 else _other(g[p - 1], g[p])


def _place(g, o, lost, n):
    """a position whose error makes exactly the windows the rule's comment names weak (the model answers a few absent k-mers
    with a count; such a place would show another run shape): judged on the oracle's answers to the INPUT"""
    p = 1000
    while True:
        p = _homopolymer(g, n + 1 if lost else max(n - 1, 1), p + 1)
        truth = g[p - 100:p + 100]
        read = truth[:100] + truth[101:] if lost else truth[:100] + bytes([_surplus(g, p, n)]) + truth[100:]
        buf, off = R.flatten([read])
        pb = R.oracle_per_base(o, buf, off, K)
        if int(((pb >= 0) & (pb < 1)).sum()) == (K - 1 - n if lost else K - n + 1):
            return p


def test_one_read_per_shape():
    g = _genome()
    o = _model(g)
    code = lambda c: b"ACGT".index(c)
    for h in (1, 2, 3):                                              # a surplus base: the read's homopolymer has h bytes, the truth's h - 1
        p = _place(g, o, False, h)
        for where in ("inside", "start", "end"):
            cut0, cut1 = {"inside": (p - 100, p + 100), "start": (p - 6, p + 100), "end": (p - 100, p + 5 + h)}[where]
            truth = g[cut0:cut1]
            q = p - cut0                                             # the read's homopolymer is x[q .. q + h - 1]
            read = truth[:q] + bytes([_surplus(g, p, h)]) + truth[q:]
            edits, rec, out = _run(o, read)
            want = q + h - 1 if where == "end" else q                # the anchor of a run at the read's end is the last byte of the homopolymer
            assert edits == [(want, E.DEL, 0)] and out == truth, (where, h, edits)
            assert (int(rec["n_runs"]), int(rec["n_sites"]), int(rec["n_del"]), int(rec["out_len"])) == (1, 1, 1, len(truth)), (where, h)
            if where == "inside":
                assert int(rec["n_weak"]) == K - h + 1
    for m in (0, 1, 2):                                              # a lost base: its homopolymer keeps m bytes in the read
        p = _place(g, o, True, m)
        for where in ("inside", "start", "end"):
            cut0, cut1 = {"inside": (p - 100, p + 100), "start": (p - 6, p + 100), "end": (p - 100, p + 6 + m)}[where]
            truth = g[cut0:cut1]
            q = p - cut0
            read = truth[:q] + truth[q + 1:]
            edits, rec, out = _run(o, read)
            want = q + m if where == "end" else q                    # before the kept bytes; at the read's end behind them: the same string
            assert edits == [(want, E.INS, code(g[p]))] and out == truth, (where, m, edits)
            assert (int(rec["n_runs"]), int(rec["n_sites"]), int(rec["n_ins"]), int(rec["out_len"])) == (1, 1, 1, len(truth)), (where, m)
            if where == "inside":
                assert int(rec["n_weak"]) == K - 1 - m


def test_edges_of_the_rule_on_reads():
    g = _genome()
    o = _model(g)
    truth = g[3000:3200]
    # a surplus first base: the deletion has no window, so with ops = DEL the site is not tried; with every kind it is, and the
    # one candidate that passes is the substitution that turns the base into the genome's base before the read
    read = bytes([_other(g[2999], g[3000])]) + truth
    edits, rec, _ = _run(o, read, ops=E.OPS_DEL)
    assert edits == [] and (int(rec["n_runs"]), int(rec["n_sites"])) == (1, 0)
    edits, rec, _ = _run(o, read)
    assert edits == [(0, E.SUB, b"ACGT".index(g[2999]))] and (int(rec["n_sites"]), int(rec["n_sub"]), int(rec["n_del"])) == (1, 1, 0)
    # two surplus bases 5 apart: one run longer than k, two substitution sites, no indel is tried
    read = truth[:100] + bytes([_other(truth[99], truth[100])]) + truth[100:105] + bytes([_other(truth[104], truth[105])]) + truth[105:]
    edits, rec, out = _run(o, read)
    assert (int(rec["n_runs"]), int(rec["n_weak"]), int(rec["n_sites"]), int(rec["n_del"]), int(rec["n_ins"])) == (1, K + 6, 2, 0, 0) and len(out) == len(read)
    # a surplus N is deleted, a base that became N is restored (four candidates)
    def n_at(make):                                                      # the first place where the N makes exactly its k windows weak
        for pos in range(100, 150):
            buf, off = R.flatten([make(pos)])
            pb = R.oracle_per_base(o, buf, off, K)
            if np.array_equal(np.nonzero((pb >= 0) & (pb < 1))[0], np.arange(pos - K + 1, pos + 1)):
                return pos, make(pos)
    pos, read = n_at(lambda p: truth[:p] + b"N" + truth[p:])
    assert _run(o, read)[0] == [(pos, E.DEL, 0)]
    pos, read = n_at(lambda p: truth[:p] + b"N" + truth[p + 1:])
    assert _run(o, read)[0] == [(pos, E.SUB, b"ACGT".index(truth[pos]))]
    # min_support around |V|: a surplus base inside has k windows for its substitutions, k - 1 for its deletion
    read = truth[:100] + bytes([_other(truth[99], truth[100])]) + truth[100:]
    edits, rec, _ = _run(o, read, ms=K - 1)
    assert edits == [(100, E.DEL, 0)] and int(rec["n_sites"]) == 1
    edits, rec, _ = _run(o, read, ms=K)                                  # only the substitutions are tried, none passes
    assert edits == [] and (int(rec["n_sites"]), int(rec["n_unfixable"])) == (1, 1)
    edits, rec, _ = _run(o, read, ms=K + 1)
    assert edits == [] and (int(rec["n_sites"]), int(rec["n_runs"])) == (0, 1)


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "seq_edit_golden.json")) as f:
        return json.load(f)


def test_result_is_not_degenerate_and_is_the_golden():
    """2000 reads, thr = ci, min_support = 1, ops = 7, judged on the ORACLE's result: enough edits of every kind, an ambiguous
    site, edits in reads with dirty bytes, and no read that equalled its truth differs from it afterwards"""
    import make_seq_edit_golden as G
    sg = _golden()
    assert sorted(sg["cases"]) == sorted(c[0] for c in GENOME_CASES)
    for case in GENOME_CASES:
        e = G.entry(case, G.oracle_of(case))
        t = e["tallies"]
        print(case[0], t)
        assert e["floors"] == {"n_sub": 400, "n_del": 250, "n_ins": 200, "n_ambiguous": 1, "edits_in_dirty_reads": 100}
        assert t["n_sub"] >= 400 and t["n_del"] >= 250 and t["n_ins"] >= 200 and t["n_ambiguous"] >= 1 and t["edits_in_dirty_reads"] >= 100
        assert t["reads_broken"] == 0 and t["reads_wrong_after"] < t["reads_wrong_before"]
        assert e == sg["cases"][case[0]], case[0]


def test_apply_edits_host():
    """kmx_apply_edits (needs no GPU) against the NumPy apply on the oracle's lists, and its error codes"""
    import make_seq_edit_golden as G
    case = GENOME_CASES[0]
    k, ci = case[1], case[2]
    reads, _, buf, off = G.reads_of(case, n_reads=600)
    edits, rec, _ = E.oracle_edit(G.oracle_of(case), buf, off, k, ci, 1, 7)
    assert len(edits) > 300 and rec["n_del"].sum() > 50 and rec["n_ins"].sum() > 50
    w_out, w_off = E.apply_edits(buf, off, edits)
    out, off2 = api.apply_edits(buf, off, edits)
    assert np.array_equal(out, w_out) and np.array_equal(off2, w_off) and np.array_equal(np.diff(off2), rec["out_len"])
    none = api.apply_edits(buf, off, np.zeros(0, np.uint64))
    assert np.array_equal(none[0], buf) and np.array_equal(none[1], off)
    both = np.array([E.edit(7, E.DEL, 0), E.edit(7, E.INS, 2), E.edit(9, E.SUB, 3), E.edit(9, E.INS, 0)], dtype=np.uint64)   # INS beside SUB / DEL at one position
    got = api.apply_edits(buf, off, both)
    assert np.array_equal(got[0], E.apply_edits(buf, off, both)[0]) and got[0][7:12].tobytes() == b"G" + bytes([buf[8]]) + b"AT" + bytes([buf[10]])
    L = api.load_library()
    n = int(off[-1])

    def rc(ed, cap=None):
        ed = np.asarray(ed, dtype=np.uint64)
        o = np.full(n + len(ed) + 8, 0x5A, dtype=np.uint8)
        oo = np.zeros(len(off), dtype=np.uint64)
        return L.kmx_apply_edits(buf.ctypes.data, off.ctypes.data, len(off) - 1, ed.ctypes.data, len(ed), o.ctypes.data, len(o) if cap is None else cap, oo.ctypes.data)

    assert rc(edits) == 0
    assert rc(edits[::-1]) == -1 and rc(np.concatenate([edits[:5], edits[4:]])) == -1                   # not strictly ascending
    assert rc([E.edit(n, E.SUB, 0)]) == -1 and rc([E.edit(n - 1, E.SUB, 0)]) == 0                        # pos >= n_bases
    assert rc([E.edit(5, 0, 0)]) == -1 and rc([E.edit(5, 4, 0)]) == -1 and rc([E.edit(5, E.SUB, 4)]) == -1 and rc([E.edit(5, E.DEL, 1)]) == -1
    assert rc([E.edit(5, E.SUB, 0), E.edit(5, E.DEL, 0)]) == -1                                          # SUB and DEL at one position
    need = len(w_out)
    assert rc(edits, cap=need - 1) == -5 and rc(edits, cap=need) == 0                                    # capacity one short
    bad_off = off.copy()
    bad_off[0] = 1
    o = np.zeros(n + 8, dtype=np.uint8)
    assert L.kmx_apply_edits(buf.ctypes.data, bad_off.ctypes.data, len(off) - 1, None, 0, o.ctypes.data, len(o), np.zeros(len(off), np.uint64).ctypes.data) == -1


def test_facade_seq_edit_program_compiles(tmp_path):
    api.load_library()
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_edit.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", str(tmp_path / "facade_seq_edit")])
