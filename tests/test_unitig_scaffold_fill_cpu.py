"""CPU: the plain-Python restatement of kmx_unitig_scaffold_fill (tests/unitig_scaffold_fill_ref.py) on the acceptance case (a
repeat of 25 bases once in each of two genome pieces, which every fragment spans) turns the scaffolds' runs of N into the
genome's own bases, leaves the two islands as they are, and satisfies the consequences include/kmx.h states on the crafted
inputs the GPU tests compare the library with; the structs of kmx.h are laid out as the ctypes and NumPy mirrors say; the entry
points refuse a null handle."""
import ctypes as C
import os
import subprocess

import pytest

import unitig_pair_paths_ref as Q
import unitig_pairs_ref as P
import unitig_scaffold_fill_ref as F
import unitig_scaffold_ref as S
import unitigs_ref as U
from kmcex_amd import api
from kmcex_amd.api import FILL_STEP_DTYPE, SCAFFOLD_FILL_DTYPE, FillParams, FillStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def checked(c, kinds=3, **kw):
    res = F.fill_of(c, kinds)
    F.check(c["k"], c["strs"], c["srecs"], c["steps"], c["plinks"], c["precs"], c["psteps"], kinds, res, **kw)
    return res


def test_the_acceptance_case():
    """k = 21; two pieces A x B and C x D of 1025 bases, x of 25 bases (5 windows), flanks of 500; 626 fragments of 400 bases from
    each.  5 unitigs: four of 520 bytes and x of 25; the graph's edges are A -> x, C -> x, x -> B, x -> D and their mirrors.  The
    pair list holds 6 entries: A -> B and C -> D with 216 pairs each (sum_dist 46440, D = 215) and four entries that end on x with 5
    pairs each, so min_pairs = 6.  The scaffold rule chains A -> B and C -> D with est = 221 - 1 - 215 - 20 = -15, hence min_n = 10
    N each: 1050 bytes.  pair_paths (tol = k) gives PATH with one step, x, and 5 windows for both.  The filled scaffolds are the two
    pieces byte for byte: 1025 bytes, 0 N, 5 filled bytes each; 20 N removed in all; x stays a scaffold of its own."""
    a = F.acceptance()
    k, strs, plinks = a["k"], a["strs"], a["plinks"]
    assert k == 21 and [len(g) for g in a["pieces"]] == [1025, 1025] and sorted(len(s) for s in strs) == [25, 520, 520, 520, 520] and len(a["reads"]) == 2 * 2 * 626
    x = a["rep"]
    assert sum(len(r) for r in a["rows"]) == 8 and sorted(len(a["rows"][2 * x + d]) for d in (0, 1)) == [2, 2]
    assert len(plinks) == 6 and sorted(e[2] for e in plinks) == [5, 5, 5, 5, 216, 216] and a["min_pairs"] == 6
    scf, pth, res = F.through_restatements(k, strs, a["rows"], plinks, a["par"], a["path_par"])
    assert sorted((r["n_steps"], r["n_bases"], r["n_gap_bases"]) for r in scf["srecs"]) == [(1, 25, 0), (2, 1050, 10), (2, 1050, 10)]
    assert [s[1:] for s in scf["steps"] if s[1]] == [(10, -15), (10, -15)]
    path = [r for r in pth["recs"] if r[0] == Q.PATH]
    assert len(path) == 2 and all(r[1] == 1 and r[3] == 5 for r in path) and {v >> 1 for v in pth["psteps"]} == {x} and pth["stats"]["n_below_min"] == 4
    F.check(k, strs, F.srecs_of(scf), scf["steps"], plinks, pth["recs"], pth["psteps"], 3, res, sstrs=scf["sstrs"], true_overlaps=True)
    long = [t for t in res["fstrs"] if len(t) > 25]
    assert len(long) == 2 and all("N" not in t for t in long)
    assert sorted(min(t, U.rc(t)) for t in long) == sorted(min(g, U.rc(g)) for g in a["pieces"])
    assert res["stats"] == dict(n_head=3, n_path=2, n_adjacent=0, n_n=0, n_no_entry=0, n_mirror=0, n_removed=20, n_filled=10)
    assert [(r["n_bases"], r["n_gap_bases"], r["n_fill_bases"], r["n_pieces"]) for r in res["frecs"]] == [(1025, 0, 5, 1), (1025, 0, 5, 1), (25, 0, 0, 0)]
    for kinds in (0, 2):                                          # nothing is ADJACENT here: the scaffolds as they were
        assert F.through_restatements(k, strs, a["rows"], plinks, a["par"], a["path_par"], kinds)[2]["fstrs"] == scf["sstrs"]
    assert F.fasta(res, F.srecs_of(scf)).startswith(">s0 n_bases=1025 n_steps=2 n_gap_bases=0 n_fill_bases=5 circular=0\n")
    assert F.fill_tsv(res, F.srecs_of(scf)).splitlines()[1].split("\t")[4:] == ["PATH", "0", "505", "5", f"{'<' if pth['psteps'][0] & 1 else '>'}u{x}"]


def test_two_islands_stay_as_they_are():
    """no path crosses the hole: the filled output is the scaffold's, with its 100 N"""
    k, strs, plinks, genome = S.two_islands()
    k2, km, cnt, strs2, reads, rows, _ = P.case("two_islands")
    q = S.TWO_ISLANDS_PARAMS
    scf, pth, res = F.through_restatements(k, strs, rows, plinks, q, dict(min_pairs=q["min_pairs"], inner=q["inner"], tol=k, max_steps=8, max_visits=4096))
    assert [r[0] for r in pth["recs"]] == [Q.NO_PATH]
    F.check(k, strs, F.srecs_of(scf), scf["steps"], plinks, pth["recs"], pth["psteps"], 3, res, sstrs=scf["sstrs"])
    assert res["fstrs"] == scf["sstrs"] == [U.rc(genome[1050:]) + "N" * 100 + U.rc(genome[:950])]
    assert res["stats"] == dict(n_head=1, n_path=0, n_adjacent=0, n_n=1, n_no_entry=0, n_mirror=0, n_removed=0, n_filled=0) and res["fsteps"][1] == (2, F.N, 0, 0, 1050, 100)


@pytest.mark.parametrize("kinds", (0, 1, 2, 3))
def test_consequences_on_the_mixed_set(kinds):
    c = F.mixed()
    res = checked(c, kinds)
    st = res["stats"]
    assert st["n_path"] == (7 if kinds & 1 else 0) and st["n_adjacent"] == (2 if kinds & 2 else 0) and st["n_no_entry"] == 1 and st["n_head"] == len(c["srecs"])
    if kinds == 3:
        assert st["n_mirror"] == 4 and st["n_n"] == 6 and sorted(f[3] for f in res["fsteps"] if f[1] == F.PATH) == [1, 1, 1, 3, 3, 4, 16]
        hub = 2 * 9 + 1
        assert sum(v >> 1 == hub >> 1 for v in res["pieces"]) == 5 and any(f[0] == hub for f in res["fsteps"])
        assert any(len(c["strs"][v >> 1]) == c["k"] for v in res["pieces"])


@pytest.mark.parametrize("seed", range(6))
def test_consequences_on_random_crafted_inputs(seed):
    for c in (F.mixed(seed + 20), F.chain(30 + seed, seed=seed), F.alignments(seed)):
        for kinds in (0, 3):
            checked(c, kinds)


def test_the_geometry_cases_are_what_they_say():
    c = F.tile_of_small_pieces()
    res = checked(c)
    assert len(res["pieces"]) == 4160 and res["stats"]["n_filled"] == 4160 and res["stats"]["n_mirror"] == 130
    c = F.long_pieces()
    res = checked(c)
    m = sorted(len(c["strs"][v >> 1]) - 20 for v in res["pieces"])
    assert m[0] == 4086 and m[-1] == 9001 and {v & 1 for v in res["pieces"]} == {0, 1}
    for nu in (255, 256, 257):
        assert checked(F.chain(nu))["stats"]["n_head"] == 1


def test_mirror_invariance_of_a_path_through_a_true_graph():
    """three unitigs cut from one string overlap by k - 1: through F and through M the filled scaffold is that string, and every
    step's whole string lies at its off (consequence (b))"""
    k = 21
    g = U.rand_seq(300, 9)
    strs = [g[:100], U.rc(g[80:160]), g[140:300]]
    for via in "FM":
        c = F.Craft(k, [k], 1)
        c.strs = strs
        c.scaffold([0, 4], [dict(via=via, path=[3])])
        b = c.build()
        res = F.fill_of(b)
        F.check(k, strs, b["srecs"], b["steps"], b["plinks"], b["precs"], b["psteps"], 3, res, true_overlaps=True)
        assert res["fstrs"][0] == g and res["pieces"] == [3] and res["stats"]["n_mirror"] == (via == "M")


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(FillParams) == 8 and C.sizeof(FillStats) == 80 and [f for f, _ in FillStats._fields_[:8]] == list(F.STAT_FIELDS)
    assert SCAFFOLD_FILL_DTYPE == F.SCAFFOLD_FILL_DTYPE and SCAFFOLD_FILL_DTYPE.itemsize == 64 and FILL_STEP_DTYPE == F.FILL_STEP_DTYPE and FILL_STEP_DTYPE.itemsize == 32
    assert [api.FILL_KINDS[i] for i in range(4)] == list(F.KINDS) and api.FILL_NO_ENTRY == F.NO_ENTRY
    fields = [("kmx_scaffold_fill", f) for f in SCAFFOLD_FILL_DTYPE.names] + [("kmx_fill_step", f) for f in FILL_STEP_DTYPE.names] + [("kmx_fill_stats", f) for f in F.STAT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %zu %d %d %d %d %u", sizeof(kmx_fill_params), sizeof(kmx_scaffold_fill), '
                   'sizeof(kmx_fill_step), sizeof(kmx_fill_stats), KMX_FILL_HEAD, KMX_FILL_N, KMX_FILL_ADJACENT, KMX_FILL_PATH, KMX_FILL_NO_ENTRY);\n' +
                   "".join(f' printf(" %zu", offsetof({s}, {f}));\n' for s, f in fields) + " return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:9] == [8, 64, 32, 80, F.HEAD, F.N, F.ADJACENT, F.PATH, F.NO_ENTRY]
    want = [SCAFFOLD_FILL_DTYPE.fields[f][1] for f in SCAFFOLD_FILL_DTYPE.names] + [FILL_STEP_DTYPE.fields[f][1] for f in FILL_STEP_DTYPE.names] + [getattr(FillStats, f).offset for f in F.STAT_FIELDS]
    assert got[9:] == want == list(range(0, 64, 8)) + [0, 4, 8, 12, 16, 24] + list(range(0, 64, 8))


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    n, par, st = C.c_uint64(0), FillParams(3, 0), FillStats()
    args = (21, None, None, 0, None, 0, None, None, 0, None, None, 0, C.byref(par), None, 0, None, None, None, None, 0, C.byref(n), C.byref(n), C.byref(st))
    assert L.kmx_unitig_scaffold_fill(None, *args) == -1
    assert L.kmx_unitig_scaffold_fill_dev(None, *args[:4], 0, *args[4:]) == -1
    assert L.kmx_unitig_scaffold_fill_last_phases(None, None) == -1


def test_facade_writers(tmp_path):
    """tests/facade_unitig_scaffold_fill.cpp compiles against include/kmodel.hpp with the reference's flags; its two writers, which
    need no device, give the restatement's text for a hand-made result (also under the host sanitizers)"""
    res = {"fstrs": ["ACGTACGTACNNAC", "GGCC"], "pieces": [6, 11, 12],
           "frecs": [dict(n_bases=14, n_gap_bases=2, n_fill_bases=5, n_pieces=3, first_piece=0), dict(n_bases=4, n_gap_bases=0, n_fill_bases=0, n_pieces=0, first_piece=3)],
           "fsteps": [(3, F.HEAD, F.NO_ENTRY, 0, 0, 0), (0, F.PATH, 7, 3, 5, 5), (4, F.ADJACENT, 2, 0, 6, 0), (9, F.N, F.NO_ENTRY, 0, 12, 2), (10, F.HEAD, F.NO_ENTRY, 0, 0, 0)]}
    srecs = [(0, 4 | S.CIRCULAR), (4, 1)]
    text = F.fasta(res, srecs) + "#\n" + F.fill_tsv(res, srecs)
    assert text.splitlines()[0] == ">s0 n_bases=14 n_steps=4 n_gap_bases=2 n_fill_bases=5 circular=1" and text.splitlines()[6] == "s0\t1\tu0\t+\tPATH\t7\t5\t5\t>u3<u5>u6"
    assert text.splitlines()[8] == "s0\t3\tu4\t-\tN\t*\t12\t2\t*"
    for name, extra in (("plain", ()), ("san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_unitig_scaffold_fill.cpp"),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        assert subprocess.check_output([exe, "--text-only"]).decode() == text, name
